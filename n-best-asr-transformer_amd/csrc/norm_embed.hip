// HBM-bound row kernels: LayerNorm fwd/bwd (K5), embedding gather+LN fwd/bwd (K1/K1b), column sums
// (bias gradients), CLS-gradient scatter, fp32->bf16 arena cast.
//
// Layout: activations [M][H] row-major.  One wave64 owns one row at a time and keeps it in
// registers (H/4 float4 chunks, chunk c on lane c%64) - a row is read from HBM exactly once per
// pass; statistics are wave-shuffle reductions in fp32.  Loads are 16 B (fp32) / 8 B (bf16) per lane.
// Column reductions (dgamma, dbeta, bias gradients) are deterministic: per-block partial rows in a
// workspace + a finalize kernel (no float atomics on the gradient of a parameter).
#include "common.h"

namespace {

constexpr int kMaxRowredBlocks = 512;
constexpr int kMaxLnBwdBlocks = 1024;   // the LayerNorm backward may use more, smaller row blocks (workspace is sized for it)
static inline int rowred_blocks(int64_t M) {
  int64_t b = (M + 31) / 32;
  if (b < 1) b = 1;
  if (b > kMaxRowredBlocks) b = kMaxRowredBlocks;
  return (int)b;
}

__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// ------------------------------------------------------------------------------------------------
template <typename T, int VPL>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y,
                                                     float* __restrict__ stats, int64_t M, int H, float eps) {
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6, nvec = H >> 2;
  const float invH = 1.0f / (float)H;
  for (int64_t row = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * wpb) {
    const T* xr = x + row * H;
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) { v[i] = Vec4<T>::load(xr + 4 * c); s += sum4(v[i]); } else v[i] = f32x4{0, 0, 0, 0};
    }
    const float mean = wave_sum(s) * invH;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) { f32x4 d = v[i] - mean; q += sum4(d * d); }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * invH + eps);
    T* yr = y + row * H;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        f32x4 g = *(const f32x4*)(gamma + 4 * c), b = *(const f32x4*)(beta + 4 * c);
        Vec4<T>::store(yr + 4 * c, (v[i] - mean) * rstd * g + b);
      }
    }
    if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
  }
}

// bf16 fast path of the LayerNorm forward (H == VPL*256): no bounds checks, gamma / beta in registers, the next row
// in flight while this one is reduced, DPP reductions.  Two-pass variance as the generic kernel.
__device__ __forceinline__ f32x2 unpack2(uint32_t w) {
  return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xFFFF0000u)};
}
__device__ __forceinline__ uint32_t pack2(f32x2 v) {
  bf16x2 o;
  o[0] = (bf16)v[0]; o[1] = (bf16)v[1];
  return __builtin_bit_cast(uint32_t, o);
}
template <int VPL>
__global__ __launch_bounds__(256) void ln_fwd_fast_kernel(const bf16* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, bf16* __restrict__ y,
                                                          float* __restrict__ stats, int64_t M, float eps,
                                                          uint8_t* __restrict__ y8,      // optional e4m3 copy of y (fp8 forward):
                                                          const uint32_t* __restrict__ a_prev, uint32_t* __restrict__ a_new) {
  // y8 = e4m3(y * s), s = 2^floor(log2(224 / amax)) from the amax y had in the previous pass (delayed scaling, common.h
  // fp8_ascale_of); this pass's amax goes to a_new.  Both null: unit scale.
  const float s8 = fp8_act_scale(a_prev);
  float amax8 = 0.f;
  constexpr int H = VPL * 256;
  constexpr float invH = 1.0f / (float)H;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  f32x2 gm[VPL][2], bt[VPL][2];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const f32x4 g4 = *(const f32x4*)(gamma + 4 * (lane + 64 * i)), b4 = *(const f32x4*)(beta + 4 * (lane + 64 * i));
    gm[i][0] = f32x2{g4[0], g4[1]}; gm[i][1] = f32x2{g4[2], g4[3]};
    bt[i][0] = f32x2{b4[0], b4[1]}; bt[i][1] = f32x2{b4[2], b4[3]};
  }
  uint2 nx[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) nx[i] = *(const uint2*)(x + row * H + 4 * (lane + 64 * i));
  for (; row < M; row += stride) {
    uint2 cx[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) cx[i] = nx[i];
    const int64_t nrow = (row + stride < M) ? row + stride : row;
#pragma unroll
    for (int i = 0; i < VPL; ++i) nx[i] = *(const uint2*)(x + nrow * H + 4 * (lane + 64 * i));
    f32x2 v[VPL][2];
    f32x2 ps = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      v[i][0] = unpack2(cx[i].x); v[i][1] = unpack2(cx[i].y);
      ps += v[i][0]; ps += v[i][1];
    }
    const float mean = wave_sum_dpp(ps[0] + ps[1]) * invH;
    f32x2 pq = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      v[i][0] = v[i][0] - mean; v[i][1] = v[i][1] - mean;
      pq += v[i][0] * v[i][0]; pq += v[i][1] * v[i][1];
    }
    const float rstd = 1.0f / sqrtf(wave_sum_dpp(pq[0] + pq[1]) * invH + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const f32x2 o0 = v[i][0] * rstd * gm[i][0] + bt[i][0], o1 = v[i][1] * rstd * gm[i][1] + bt[i][1];
      const uint2 pk = uint2{pack2(o0), pack2(o1)};
      *(uint2*)(y + row * H + 4 * (lane + 64 * i)) = pk;
      if (y8) {   // e4m3 of the bf16 value that was just stored (what a cast of y would give), times the tensor's scale
        const f32x2 r0 = unpack2(pk.x), r1 = unpack2(pk.y);
        if (a_new) amax8 = fmaxf(fmaxf(amax8, fmaxf(fabsf(r0[0]), fabsf(r0[1]))), fmaxf(fabsf(r1[0]), fabsf(r1[1])));
        const float q[4] = {r0[0] * s8, r0[1] * s8, r1[0] * s8, r1[1] * s8};
        *(uint32_t*)(y8 + row * H + 4 * (lane + 64 * i)) = fp8_pack4(q);
      }
    }
    if (lane == 0) *(f32x2*)(stats + 2 * row) = f32x2{mean, rstd};
  }
  if (y8 && a_new) {
    amax8 = wave_max(amax8);
    if (lane == 0) amax_update(a_new, amax8);
  }
}

// partials layout: part[k][blk][H], k = 0 dgamma, 1 dbeta, 2 dbias(sum of dx)
// PARAMS = false (nbest_encoder_desc.no_param_grad): dx / dx_drop only - no column sums, no LDS, no partial rows, no barrier
template <typename T, int VPL, bool PARAMS = true>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const float* __restrict__ stats, const float* __restrict__ gamma,
                                                     T* __restrict__ dx, T* __restrict__ dx_drop, float* __restrict__ part,
                                                     int64_t M, int H, int rows_per_block, int with_dbias, DropCfg drop) {
  extern __shared__ __attribute__((aligned(16))) float acc[];  // [3][H]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6, nvec = H >> 2;
  const float invH = 1.0f / (float)H;
  if constexpr (PARAMS) {
    for (int i = threadIdx.x; i < 3 * H; i += blockDim.x) acc[i] = 0.f;
    __syncthreads();
  }
  f32x4 ag[VPL], ab[VPL], ad[VPL], gm[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    ag[i] = ab[i] = ad[i] = f32x4{0, 0, 0, 0};
    const int c = lane + 64 * i;
    gm[i] = (c < nvec) ? *(const f32x4*)(gamma + 4 * c) : f32x4{0, 0, 0, 0};
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < M) ? r0 + rows_per_block : M;
  // software prefetch: the (packed) x / dy of the NEXT row are in flight while this row is reduced
  typename Vec4<T>::raw_t nx[VPL], nd[VPL];
  float nmean = 0.f, nrstd = 0.f;
  {
    const int64_t row = r0 + wave;
    if (row < r1) {
      nmean = stats[2 * row]; nrstd = stats[2 * row + 1];
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) { nx[i] = Vec4<T>::raw_load(x + row * H + 4 * c); nd[i] = Vec4<T>::raw_load(dy + row * H + 4 * c); }
      }
    }
  }
  for (int64_t row = r0 + wave; row < r1; row += wpb) {
    const float mean = nmean, rstd = nrstd;
    typename Vec4<T>::raw_t cx[VPL], cd[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) { cx[i] = nx[i]; cd[i] = nd[i]; }
    const int64_t nrow = row + wpb;
    if (nrow < r1) {
      nmean = stats[2 * nrow]; nrstd = stats[2 * nrow + 1];
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) { nx[i] = Vec4<T>::raw_load(x + nrow * H + 4 * c); nd[i] = Vec4<T>::raw_load(dy + nrow * H + 4 * c); }
      }
    }
    f32x4 xh[VPL], g[VPL], d[VPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        xh[i] = (Vec4<T>::cvt(cx[i]) - mean) * rstd;
        d[i] = Vec4<T>::cvt(cd[i]);
        g[i] = d[i] * gm[i];
        s1 += sum4(g[i]);
        s2 += sum4(g[i] * xh[i]);
      } else {
        xh[i] = g[i] = d[i] = f32x4{0, 0, 0, 0};
      }
    }
    s1 = wave_sum(s1) * invH;
    s2 = wave_sum(s2) * invH;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        f32x4 o = (g[i] - s1 - xh[i] * s2) * rstd;
        Vec4<T>::store(dx + row * H + 4 * c, o);
        if constexpr (PARAMS) {
          ag[i] += d[i] * xh[i];
          ab[i] += d[i];
        }
        if (drop.thr16) {  // gradient that flows into the dense layer under the (regenerated) dropout mask
          const uint32_t k = nb_keep4(drop, (uint32_t)(row * H + 4 * c));
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (k >> e & 1) ? o[e] * drop.scale : 0.f;
          Vec4<T>::store(dx_drop + row * H + 4 * c, o);
        }
        if constexpr (PARAMS) ad[i] += o;
      }
    }
  }
  if constexpr (!PARAMS) return;
  // the waves add their column sums into the block's LDS row one after the other (plain read-modify-write:
  // LDS float atomics cost ~10 us per workgroup here)
  for (int w = 0; w < wpb; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
          *(f32x4*)&acc[4 * c] += ag[i];
          *(f32x4*)&acc[H + 4 * c] += ab[i];
          if (with_dbias) *(f32x4*)&acc[2 * H + 4 * c] += ad[i];
        }
      }
    }
    __syncthreads();
  }
  const int nblk = gridDim.x;
  for (int i = threadIdx.x; i < H; i += blockDim.x) {
    part[((int64_t)0 * nblk + blockIdx.x) * H + i] = acc[i];
    part[((int64_t)1 * nblk + blockIdx.x) * H + i] = acc[H + i];
    if (with_dbias) part[((int64_t)2 * nblk + blockIdx.x) * H + i] = acc[2 * H + i];
  }
}

// ---- bf16 fast path of the LayerNorm backward: H == VPL*256, no bounds checks, no divergent branches ----------
// The generic kernel above spends ~500 VALU instructions per row (exec-mask branches around every vector, register
// shuffles, six LDS-crossbar shuffles per reduction) and was VALU-issue bound at two waves per SIMD (59 us for 200 MB).
// Here: packed-pair fp32 math, bf16 pairs unpacked with one shift / one mask, DPP reductions, the dropout hash input
// formed by addition from a per-row scalar base, compile-time DROP / DBIAS, conflict-free LDS accumulation.
__device__ __forceinline__ f32x2 unpack_bf16x2(uint32_t w) { return unpack2(w); }
__device__ __forceinline__ uint32_t pack_bf16x2(f32x2 v) { return pack2(v); }

template <int VPL, bool DROP, bool DBIAS, int WAVES, bool PARAMS = true>   // PARAMS = false: dx / dx_drop only (see ln_bwd_kernel)
__global__ __launch_bounds__(WAVES * 64) void ln_bwd_fast_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                          const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          bf16* __restrict__ dx, bf16* __restrict__ dx_drop,
                                                          float* __restrict__ part, int64_t M, int rows_per_block, DropCfg drop,
                                                          Fp8Grad f8) {   // f8: e4m3 copy / amax of the dense-branch gradient
  constexpr int H = VPL * 256;
  extern __shared__ __attribute__((aligned(16))) float acc[];   // [wave][k][e][i][lane]: every wave parks its column sums here
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float s8 = fp8_grad_scale(f8.amax_prev);
  float amax8 = 0.f;
  f32x2 gm[VPL][2], ag[VPL][2], ab[VPL][2], ad[VPL][2];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const f32x4 g4 = *(const f32x4*)(gamma + 4 * (lane + 64 * i));
    gm[i][0] = f32x2{g4[0], g4[1]}; gm[i][1] = f32x2{g4[2], g4[3]};
    ag[i][0] = ag[i][1] = ab[i][0] = ab[i][1] = ad[i][0] = ad[i][1] = f32x2{0.f, 0.f};
  }
  // rows are dealt round-robin over ALL waves of the grid (rows_per_block < 0: stride = -rows_per_block), so at any
  // moment the grid streams one contiguous window of the tensors instead of gridDim.x*4 separate ones
  const int64_t stride = rows_per_block < 0 ? -(int64_t)rows_per_block : WAVES;
  const int64_t r0 = rows_per_block < 0 ? (int64_t)blockIdx.x * WAVES : (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = rows_per_block < 0 ? M : ((r0 + rows_per_block < M) ? r0 + rows_per_block : M);
  constexpr float invH = 1.0f / (float)H;
  int64_t row = r0 + wave;
  if (row < r1) {
    uint2 nx[VPL], nd[VPL];
    float nmean = stats[2 * row], nrstd = stats[2 * row + 1];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      nx[i] = *(const uint2*)(x + row * H + 4 * (lane + 64 * i));
      nd[i] = *(const uint2*)(dy + row * H + 4 * (lane + 64 * i));
    }
    for (; row < r1; row += stride) {
      const float mean = nmean, rstd = nrstd;
      uint2 cx[VPL], cd[VPL];
#pragma unroll
      for (int i = 0; i < VPL; ++i) { cx[i] = nx[i]; cd[i] = nd[i]; }
      {  // next row (clamped: the last iteration re-reads its own row instead of branching)
        const int64_t nrow = (row + stride < r1) ? row + stride : row;
        nmean = stats[2 * nrow]; nrstd = stats[2 * nrow + 1];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          nx[i] = *(const uint2*)(x + nrow * H + 4 * (lane + 64 * i));
          nd[i] = *(const uint2*)(dy + nrow * H + 4 * (lane + 64 * i));
        }
      }
      const float mr = -mean * rstd;
      f32x2 xh[VPL][2], d[VPL][2], g[VPL][2];
      f32x2 p1 = {0.f, 0.f}, p2 = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        xh[i][0] = unpack_bf16x2(cx[i].x) * rstd + mr; xh[i][1] = unpack_bf16x2(cx[i].y) * rstd + mr;
        d[i][0] = unpack_bf16x2(cd[i].x); d[i][1] = unpack_bf16x2(cd[i].y);
        g[i][0] = d[i][0] * gm[i][0]; g[i][1] = d[i][1] * gm[i][1];
        p1 += g[i][0]; p1 += g[i][1];
        p2 += g[i][0] * xh[i][0]; p2 += g[i][1] * xh[i][1];
      }
      float s1 = p1[0] + p1[1], s2 = p2[0] + p2[1];
      wave_sum2(s1, s2);
      const float a1 = -s1 * invH * rstd, a2 = -s2 * invH * rstd;
      const uint32_t hbase = (uint32_t)((row * H) >> 1) * 0x9E3779B9U + drop.key;   // hash input of the row's first pair
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        f32x2 o[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) o[h] = xh[i][h] * a2 + (g[i][h] * rstd + a1);
        const int64_t off = row * H + 4 * (lane + 64 * i);
        *(uint2*)(dx + off) = uint2{pack_bf16x2(o[0]), pack_bf16x2(o[1])};
        if constexpr (PARAMS) {
#pragma unroll
          for (int h = 0; h < 2; ++h) { ag[i][h] += d[i][h] * xh[i][h]; ab[i][h] += d[i][h]; }
        }
        if (DROP) {
          const uint32_t q = (uint32_t)(2 * (lane + 64 * i));   // pair index inside the row
          const uint32_t h0 = nb_hash32(hbase + q * 0x9E3779B9U), h1 = nb_hash32(hbase + (q + 1) * 0x9E3779B9U);
          o[0][0] = ((h0 & 0xFFFFu) >= drop.thr16) ? o[0][0] * drop.scale : 0.f;
          o[0][1] = ((h0 >> 16) >= drop.thr16) ? o[0][1] * drop.scale : 0.f;
          o[1][0] = ((h1 & 0xFFFFu) >= drop.thr16) ? o[1][0] * drop.scale : 0.f;
          o[1][1] = ((h1 >> 16) >= drop.thr16) ? o[1][1] * drop.scale : 0.f;
          if (dx_drop) *(uint2*)(dx_drop + off) = uint2{pack_bf16x2(o[0]), pack_bf16x2(o[1])};   // (null: only its e4m3 copy is wanted)
        }
        if (PARAMS && DBIAS) { ad[i][0] += o[0]; ad[i][1] += o[1]; }
        if (f8.amax_new) {   // o = the gradient the dense-layer dgrad / wgrad GEMMs read (after the dropout mask)
          amax8 = fmaxf(fmaxf(amax8, fmaxf(fabsf(o[0][0]), fabsf(o[0][1]))), fmaxf(fabsf(o[1][0]), fabsf(o[1][1])));
          if (f8.out8) {
            const float q[4] = {o[0][0] * s8, o[0][1] * s8, o[1][0] * s8, o[1][1] * s8};
            *(uint32_t*)(f8.out8 + off) = fp8_pack4(q);
          }
        }
      }
    }
  }
  if (f8.amax_new) {
    amax8 = wave_max(amax8);
    if (lane == 0) amax_update(f8.amax_new, amax8);
  }
  if constexpr (!PARAMS) return;
  float* mine = acc + wave * 3 * H;
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int a = (e * VPL + i) * 64 + lane;
      mine[a] = ag[i][e >> 1][e & 1];
      mine[H + a] = ab[i][e >> 1][e & 1];
      if (DBIAS) mine[2 * H + a] = ad[i][e >> 1][e & 1];
    }
  __syncthreads();
  const int nblk = gridDim.x;
  for (int col = threadIdx.x; col < H; col += WAVES * 64) {
    const int chunk = col >> 2, e = col & 3, a = (e * VPL + (chunk >> 6)) * 64 + (chunk & 63);
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      t0 += acc[w * 3 * H + a]; t1 += acc[w * 3 * H + H + a];
      if (DBIAS) t2 += acc[w * 3 * H + 2 * H + a];
    }
    part[((int64_t)0 * nblk + blockIdx.x) * H + col] = t0;
    part[((int64_t)1 * nblk + blockIdx.x) * H + col] = t1;
    if (DBIAS) part[((int64_t)2 * nblk + blockIdx.x) * H + col] = t2;
  }
}

// out_k[col] (+)= sum_blk part[k][blk][col];  grid (ceil(N/64), nout), block (64,16)
struct RowredOut {
  float* out[3];
  int accumulate[3];
};
__global__ __launch_bounds__(1024) void rowred_finalize_kernel(const float* __restrict__ part, int nblk, int N, RowredOut o) {
  // block = 32 columns x 32 row lanes (twice the workgroups of a 64 x 16 block for the same N, half the rows per
  // thread, four independent partial sums per thread): this launch is pure latency, 2 - 5 MB read by a few dozen blocks
  __shared__ float sm[32][33];
  const int k = blockIdx.y;
  const int col = blockIdx.x * 32 + threadIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < N && o.out[k] != nullptr) {
    const float* p = part + (int64_t)k * nblk * N + col;
    int b = threadIdx.y;
    for (; b + 96 < nblk; b += 128) {
      s0 += p[(int64_t)b * N]; s1 += p[(int64_t)(b + 32) * N]; s2 += p[(int64_t)(b + 64) * N]; s3 += p[(int64_t)(b + 96) * N];
    }
    for (; b < nblk; b += 32) s0 += p[(int64_t)b * N];
  }
  sm[threadIdx.y][threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (threadIdx.y == 0 && col < N && o.out[k] != nullptr) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) s += sm[r][threadIdx.x];
    o.out[k][col] = o.accumulate[k] ? o.out[k][col] + s : s;
  }
}

// column sums of X[M][N] (ld): block = 64 column-float4 lanes x 4 row lanes; grid (ceil(N/256), nblk)
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ X, float* __restrict__ part, int64_t M,
                                                     int64_t N, int64_t ld, int rows_per_block) {
  __shared__ f32x4 sm[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 256 + 4 * tx;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < M) ? r0 + rows_per_block : M;
  f32x4 a = {0, 0, 0, 0};
  if (col < N)
    for (int64_t r = r0 + ty; r < r1; r += 4) a += Vec4<T>::load(X + r * ld + col);
  sm[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && col < N) {
    a = (sm[0][tx] + sm[1][tx]) + (sm[2][tx] + sm[3][tx]);
    *(f32x4*)(part + (int64_t)blockIdx.y * N + col) = a;
  }
}

// ------------------------------------------------------------------------------------------------
// Embedding row arithmetic of the interpolated forward (integrated gradients) and nbest_embed_attrib.  emb_row_stats restates
// embed_fwd_kernel's statistics code (that kernel keeps its inline copy, so its plain instantiations compute the bits they computed
// before); the compiler may contract the two copies differently, so the attribution kernel's statistics agree with the forward's to
// rounding.
// Word part of a row at path point a: ((1 - a) wb + a w) in fp32 from the stored table rows, one fma per element
// (a = 1: exactly w; a = 0: exactly wb).
__device__ __forceinline__ f32x4 emb_lerp4(f32x4 w, f32x4 wb, float a) {
  const float b = 1.0f - a;
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(a, w[e], b * wb[e]);
  return r;
}
// mean and rstd of the row v (chunk c = lane + 64 i, c < nvec), s = this lane's sum of its chunks in ascending i
template <int VPL>
__device__ __forceinline__ void emb_row_stats(const f32x4* v, float s, int lane, int nvec, float invH, float eps, float& mean,
                                              float& rstd) {
  mean = wave_sum(s) * invH;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nvec) { f32x4 d = v[i] - mean; q += sum4(d * d); }
  }
  rstd = 1.0f / sqrtf(wave_sum(q) * invH + eps);
}

// INTERP (nbest_embed_ln_fwd_interp): the word part of row m is emb_lerp4(word[ids[m]], word[base_ids[m]], alpha[m / S]); one kernel
// for both, so that an alpha = 1 row runs the plain forward's instructions
// ADV (nbest_embed_ln_fwd_adv): the word part of row m is word[ids[m]] + delta[m] (fp32 [M][H]), added before the token-type row - the
// order emb_tok_grad<ADV> recomputes; a zero delta row leaves the word row's bits
template <typename T, int VPL, bool INTERP = false, bool ADV = false>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ seg,
                                                        const int64_t* __restrict__ pos, const T* __restrict__ word,
                                                        const T* __restrict__ type, const T* __restrict__ ptab,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        T* __restrict__ out, float* __restrict__ stats, int64_t M, int H,
                                                        float eps, DropCfg drop, const int64_t* __restrict__ base_ids = nullptr,
                                                        const float* __restrict__ alpha = nullptr, int S = 1,
                                                        const float* __restrict__ delta = nullptr) {
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6, nvec = H >> 2;
  const float invH = 1.0f / (float)H;
  for (int64_t row = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * wpb) {
    const T* wr = word + ids[row] * H;
    const T* tr = type + (seg ? seg[row] : 0) * H;
    const T* pr = ptab + pos[row] * H;
    const T* br = INTERP ? word + base_ids[row] * H : nullptr;
    const float a = INTERP ? alpha[row / S] : 1.f;
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        if constexpr (INTERP)
          v[i] = (emb_lerp4(Vec4<T>::load(wr + 4 * c), Vec4<T>::load(br + 4 * c), a) + Vec4<T>::load(tr + 4 * c)) + Vec4<T>::load(pr + 4 * c);
        else if constexpr (ADV)
          v[i] = ((Vec4<T>::load(wr + 4 * c) + *(const f32x4*)(delta + row * H + 4 * c)) + Vec4<T>::load(tr + 4 * c)) + Vec4<T>::load(pr + 4 * c);
        else
          v[i] = (Vec4<T>::load(wr + 4 * c) + Vec4<T>::load(tr + 4 * c)) + Vec4<T>::load(pr + 4 * c);
        s += sum4(v[i]);
      } else v[i] = f32x4{0, 0, 0, 0};
    }
    const float mean = wave_sum(s) * invH;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) { f32x4 d = v[i] - mean; q += sum4(d * d); }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * invH + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        f32x4 g = *(const f32x4*)(gamma + 4 * c), b = *(const f32x4*)(beta + 4 * c);
        f32x4 o = (v[i] - mean) * rstd * g + b;
        if (drop.thr16) {
          const uint32_t k = nb_keep4(drop, (uint32_t)(row * H + 4 * c));
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (k >> e & 1) ? o[e] * drop.scale : 0.f;
        }
        Vec4<T>::store(out + row * H + 4 * c, o);
      }
    }
    if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
  }
}

// Integrated-gradients reduction (nbest_embed_attrib).  One wave per (pair p, token t); the pair's m path points are the rows
// r_k = (p m + k) S + t, k = 0 .. m-1, of an encoder call whose embeddings were interpolated (embed_fwd_kernel<INTERP>, no dropout).
// word[x], word[x'], the type row, the position row and gamma stay in registers; for each k in ascending order the wave recomputes
// the row E(alpha[p m + k]) with the forward's lerp and additions and its statistics with emb_row_stats, applies the LayerNorm
// backward to dh[r_k] (the formula of emb_tok_grad) and adds the dot product with delta = word[x] - word[x'] to an fp32 sum:
//   attr[p S + t] = (sum_k <LN'(dh[r_k]), delta>) / m      (x == x', padding included: exactly 0, dh not read).
// No LDS, no barrier, no atomics: the same additions in the same order on every run.  The next path point's dh row is in flight
// while this one is reduced.
template <typename T, int VPL>
__global__ __launch_bounds__(256) void embed_attrib_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ base_ids,
                                                           const float* __restrict__ alpha, const int64_t* __restrict__ seg,
                                                           const int64_t* __restrict__ pos, const T* __restrict__ word,
                                                           const T* __restrict__ type, const T* __restrict__ ptab,
                                                           const float* __restrict__ gamma, const T* __restrict__ dh,
                                                           float* __restrict__ attr, int64_t n_items, int m, int S, int H, float eps) {
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6, nvec = H >> 2;
  const float invH = 1.0f / (float)H;
  for (int64_t it = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); it < n_items; it += (int64_t)gridDim.x * wpb) {
    const int64_t p = it / S;
    const int64_t row0 = p * m * S + (it - p * S);   // path point k: row0 + k S
    const int64_t id = ids[row0], bid = base_ids[row0];
    if (id == bid) {   // wave-uniform: no displacement, no attribution
      if (lane == 0) attr[it] = 0.f;
      continue;
    }
    const T* wr = word + id * H;
    const T* br = word + bid * H;
    const T* tr = type + (seg ? seg[row0] : 0) * H;
    const T* pr = ptab + pos[row0] * H;
    f32x4 w[VPL], wb[VPL], tp[VPL], pp[VPL], gm[VPL], dl[VPL];
    typename Vec4<T>::raw_t nd[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        w[i] = Vec4<T>::load(wr + 4 * c); wb[i] = Vec4<T>::load(br + 4 * c);
        tp[i] = Vec4<T>::load(tr + 4 * c); pp[i] = Vec4<T>::load(pr + 4 * c);
        gm[i] = *(const f32x4*)(gamma + 4 * c);
        dl[i] = w[i] - wb[i];
        nd[i] = Vec4<T>::raw_load(dh + row0 * H + 4 * c);
      } else {
        w[i] = wb[i] = tp[i] = pp[i] = gm[i] = dl[i] = f32x4{0, 0, 0, 0};
      }
    }
    float acc = 0.f;
    for (int k = 0; k < m; ++k) {
      typename Vec4<T>::raw_t cd[VPL];
#pragma unroll
      for (int i = 0; i < VPL; ++i) cd[i] = nd[i];
      if (k + 1 < m) {
        const T* nr = dh + (row0 + (int64_t)(k + 1) * S) * H;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int c = lane + 64 * i;
          if (c < nvec) nd[i] = Vec4<T>::raw_load(nr + 4 * c);
        }
      }
      const float a = alpha[p * m + k];
      f32x4 v[VPL];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
          v[i] = (emb_lerp4(w[i], wb[i], a) + tp[i]) + pp[i];
          s += sum4(v[i]);
        } else v[i] = f32x4{0, 0, 0, 0};
      }
      float mean, rstd;
      emb_row_stats<VPL>(v, s, lane, nvec, invH, eps, mean, rstd);
      f32x4 xh[VPL], g[VPL];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
          xh[i] = (v[i] - mean) * rstd;
          g[i] = Vec4<T>::cvt(cd[i]) * gm[i];
          s1 += sum4(g[i]);
          s2 += sum4(g[i] * xh[i]);
        } else {
          xh[i] = g[i] = f32x4{0, 0, 0, 0};
        }
      }
      wave_sum2(s1, s2);
      s1 *= invH; s2 *= invH;
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) dot += sum4(((g[i] - s1 - xh[i] * s2) * rstd) * dl[i]);
      }
      acc += wave_sum(dot);
    }
    if (lane == 0) attr[it] = acc / (float)m;
  }
}

// FGM perturbation (nbest_embed_adv_delta), launch 1.  One wave per token row m: g_m = the embedding LayerNorm backward of the
// dropout-masked dout[m] (the formula of emb_tok_grad, mean and rstd recomputed from the clean row with emb_row_stats, as the
// attribution kernel does) goes to delta[m] in fp32, its sum of squares to rowsq[m].  Rows with key_mask[m] == 0: exact zeros, no table
// or statistics work.  The next row's dout is in flight while this one is reduced.  No LDS, no atomics.
template <typename T, int VPL>
__global__ __launch_bounds__(256) void embed_adv_grad_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ seg,
                                                             const int64_t* __restrict__ pos, const uint8_t* __restrict__ key_mask,
                                                             const T* __restrict__ word, const T* __restrict__ type,
                                                             const T* __restrict__ ptab, const float* __restrict__ gamma,
                                                             const T* __restrict__ dout, float* __restrict__ delta,
                                                             float* __restrict__ rowsq, int64_t M, int H, float eps, DropCfg drop) {
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6, nvec = H >> 2;
  const float invH = 1.0f / (float)H;
  const int64_t stride = (int64_t)gridDim.x * wpb;
  int64_t row = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
  if (row >= M) return;
  f32x4 gm[VPL];
  typename Vec4<T>::raw_t nd[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nvec) { gm[i] = *(const f32x4*)(gamma + 4 * c); nd[i] = Vec4<T>::raw_load(dout + row * H + 4 * c); }
    else gm[i] = f32x4{0, 0, 0, 0};
  }
  for (; row < M; row += stride) {
    typename Vec4<T>::raw_t cd[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) cd[i] = nd[i];
    if (row + stride < M) {
      const T* nr = dout + (row + stride) * H;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) nd[i] = Vec4<T>::raw_load(nr + 4 * c);
      }
    }
    float* gr = delta + row * H;
    if (key_mask[row] == 0) {   // wave-uniform: a masked token is not perturbed
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) *(f32x4*)(gr + 4 * c) = f32x4{0, 0, 0, 0};
      }
      if (lane == 0) rowsq[row] = 0.f;
      continue;
    }
    const T* wr = word + ids[row] * H;
    const T* tr = type + (seg ? seg[row] : 0) * H;
    const T* pr = ptab + pos[row] * H;
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        v[i] = (Vec4<T>::load(wr + 4 * c) + Vec4<T>::load(tr + 4 * c)) + Vec4<T>::load(pr + 4 * c);
        s += sum4(v[i]);
      } else v[i] = f32x4{0, 0, 0, 0};
    }
    float mean, rstd;
    emb_row_stats<VPL>(v, s, lane, nvec, invH, eps, mean, rstd);
    f32x4 xh[VPL], g[VPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        xh[i] = (v[i] - mean) * rstd;
        f32x4 d = Vec4<T>::cvt(cd[i]);
        if (drop.thr16) {
          const uint32_t k = nb_keep4(drop, (uint32_t)(row * H + 4 * c));
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = (k >> e & 1) ? d[e] * drop.scale : 0.f;
        }
        g[i] = d * gm[i];
        s1 += sum4(g[i]);
        s2 += sum4(g[i] * xh[i]);
      } else {
        xh[i] = g[i] = f32x4{0, 0, 0, 0};
      }
    }
    wave_sum2(s1, s2);
    s1 *= invH; s2 *= invH;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        const f32x4 o = (g[i] - s1 - xh[i] * s2) * rstd;
        *(f32x4*)(gr + 4 * c) = o;
        q += sum4(o * o);
      }
    }
    q = wave_sum(q);
    if (lane == 0) rowsq[row] = q;
  }
}

// launch 2, grid (Y, B): every block of utterance b forms n_b = sqrt(rowsq[b S] + rowsq[b S + 1] + ...) itself, in ascending t (the
// same S additions in every block and on every run), and scales its slice of the utterance's S H values in place by epsilon / n_b;
// n_b zero or not finite: exact zeros.  Block (0, b) writes norm[b].
__global__ __launch_bounds__(256) void embed_adv_scale_kernel(float* __restrict__ delta, const float* __restrict__ rowsq,
                                                              float* __restrict__ norm, int S, int H, float epsilon) {
  const int b = blockIdx.y;
  float q = 0.f;
  for (int t = 0; t < S; ++t) q += rowsq[(int64_t)b * S + t];
  const float n = sqrtf(q);
  const bool ok = n > 0.f && n <= 3.4028234e38f;   // false for 0, NaN and infinity
  const float sc = ok ? epsilon / n : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) norm[b] = n;
  const int64_t nv = (int64_t)S * (H >> 2);
  f32x4* p = (f32x4*)(delta + (int64_t)b * S * H);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = ok ? p[i] * sc : f32x4{0, 0, 0, 0};
}

// Embedding backward, deterministic (round 4; rounds 1-3 summed the word table with fp32 atomics: 150 us at the atomic rate and
// a step that was not bit-reproducible).  LayerNorm backward per token gives de = o (fp32, registers only); five kernels:
//   embed_bwd_colkey_kernel  one block per sequence position j: the column's key colkey[j] = the position key of its first
//                          non-padding row, and whether another non-padding row of the column has a different key (`mixed`).
//   embed_bwd_pos_kernel   block (j, y) owns sequence position j for the samples b = y, y + Y, ...: the rows whose key is colkey[j]
//                          (every non-padding row of the column for BERT's arange and for right-padded RoBERTa-family positions, in any
//                          row order) keep the position / token-type 0, 1 / LayerNorm-parameter sums in registers and leave them as ONE
//                          partial row per block and quantity (summed by embed_bwd_finalize_kernel in a fixed order).  Rows with another
//                          non-padding key (left padding, a padding id inside a row, arbitrary positions) and token types >= 2 fall back
//                          to float row atomics - correct, not reproducible.  Block (j, 0) also records whether position row colkey[j]
//                          can receive anything besides column j's sum (`shared`: a fallback anywhere, or another column with that key).
//   embed_bwd_word_kernel  the word table as a SEGMENTED REDUCE over the tokens sorted by word id (`perm`: a stable argsort of ids,
//                          built by the data loader next to ids): wave c owns `tpc` consecutive sorted tokens, recomputes o for each
//                          and adds runs of equal id in registers, in sorted order.  A run that begins and ends inside the chunk is
//                          stored straight into its table row (one plain 16-byte store per lane, no atomics, no memset of the touched
//                          rows needed); a run that crosses a chunk boundary leaves a partial row (slot 0: the run began before the
//                          chunk; slot 1: it began in the chunk and continues past it).
//   embed_bwd_wordfix_kernel  one block per chunk; the chunk in which a boundary-crossing run BEGINS sums that run's partial rows in
//                          chunk order (fixed tree: wave w takes every 4th row, the four wave sums are added in wave order) and stores
//                          the table row.  Frequent ids ([SEP]: (n_best + 1) x B tokens) span up to M / tpc chunks.
// Same additions in the same order on every run: for the layouts without fallback rows (every column's non-padding keys equal,
// column keys distinct, token types 0 / 1) the gradient is bit-reproducible.  Both token kernels recompute o (two reads of
// dout and of the gathered table rows, 2 x 100 MB at B = 256, S = 128 - mostly out of the Infinity Cache the second time) instead of
// writing it (100 MB fp32 out, 100 MB back in).
template <typename T, int VPL>
struct EmbTok {
  typename Vec4<T>::raw_t w[VPL], t[VPL], p[VPL], d[VPL];
  float mean, rstd;
};
// FULL: H == 256 VPL (every lane owns VPL whole chunks): no exec-mask guards, so a group of token loads is one straight run of
// global_load instructions the compiler never has to wait on early
template <typename T, int VPL, bool FULL>
__device__ __forceinline__ void emb_tok_load(EmbTok<T, VPL>& r, int64_t row, int64_t id, int64_t sv, int64_t key, const T* __restrict__ word,
                                             const T* __restrict__ type, const T* __restrict__ ptab, const float* __restrict__ stats,
                                             const T* __restrict__ dout, int H, int lane, int nvec) {
  const T* wr = word + id * H;
  const T* tr = type + sv * H;
  const T* pr = ptab + key * H;
  const T* dr = dout + row * H;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (FULL || c < nvec) {
      r.w[i] = Vec4<T>::raw_load(wr + 4 * c); r.t[i] = Vec4<T>::raw_load(tr + 4 * c);
      r.p[i] = Vec4<T>::raw_load(pr + 4 * c); r.d[i] = Vec4<T>::raw_load(dr + 4 * c);
    }
  }
  r.mean = stats[2 * row]; r.rstd = stats[2 * row + 1];
}
// ADV (nbest_embed_ln_bwd_adv): the forward added delta[row] (fp32) to the word row, so the recomputed x_hat does too.  The row travels
// beside EmbTok, in an array only the ADV instantiations declare with VPL entries: the plain ones keep their loads and registers.
template <int VPL, bool FULL>
__device__ __forceinline__ void emb_tok_delta(f32x4* dl, int64_t row, const float* __restrict__ delta, int H, int lane, int nvec) {
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (FULL || c < nvec) dl[i] = *(const f32x4*)(delta + row * H + 4 * c);
  }
}
// o = d(embedding sum) of the token; d / xh = dropout-masked upstream gradient and the normalised row (LayerNorm-parameter sums)
template <typename T, int VPL, bool FULL, bool ADV = false>
__device__ __forceinline__ void emb_tok_grad(const EmbTok<T, VPL>& r, int64_t row, const f32x4* gm, f32x4* o, f32x4* d, f32x4* xh, int H,
                                             int lane, int nvec, float invH, const DropCfg& drop, const f32x4* dl = nullptr) {
  f32x4 g[VPL];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (FULL || c < nvec) {
      f32x4 e;
      if constexpr (ADV) e = ((Vec4<T>::cvt(r.w[i]) + dl[i]) + Vec4<T>::cvt(r.t[i])) + Vec4<T>::cvt(r.p[i]);
      else e = (Vec4<T>::cvt(r.w[i]) + Vec4<T>::cvt(r.t[i])) + Vec4<T>::cvt(r.p[i]);
      xh[i] = (e - r.mean) * r.rstd;
      d[i] = Vec4<T>::cvt(r.d[i]);
      if (drop.thr16) {
        const uint32_t k = nb_keep4(drop, (uint32_t)(row * H + 4 * c));
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) d[i][e2] = (k >> e2 & 1) ? d[i][e2] * drop.scale : 0.f;
      }
      g[i] = d[i] * gm[i];
      s1 += sum4(g[i]);
      s2 += sum4(g[i] * xh[i]);
    } else {
      xh[i] = g[i] = d[i] = f32x4{0, 0, 0, 0};
    }
  }
  wave_sum2(s1, s2);
  s1 *= invH; s2 *= invH;
#pragma unroll
  for (int i = 0; i < VPL; ++i) o[i] = (g[i] - s1 - xh[i] * s2) * r.rstd;
}
constexpr int kEmbGroupWord = 4, kEmbGroupPos = 2;   // tokens whose rows a wave has in flight at once (the position kernel carries five accumulator rows)

// grid S, block 256: colkey[j] = key of the first non-padding row of column j (pos_pad_id if there is none), mixed[j] = some
// non-padding row of the column has another key.  tables_accumulate == 0: zero every row something will be ADDED to - row colkey[j]
// (finalize adds into it when the row is shared), the rows of the column's fallback tokens and dtype_tab rows >= 2 - so that a touched
// row is overwritten whichever path reaches it (zeros only: blocks that zero the same row do not conflict).
__global__ __launch_bounds__(256) void embed_bwd_colkey_kernel(const int64_t* __restrict__ seg, const int64_t* __restrict__ pos, int B, int S,
                                                               int H, int64_t pos_pad_id, int tables_accumulate, int64_t* __restrict__ colkey,
                                                               int* __restrict__ mixed, float* __restrict__ dptab, float* __restrict__ dtype_tab) {
  __shared__ int first[4];
  const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bmin = B;
  for (int b = threadIdx.x; b < B; b += blockDim.x)
    if (pos[(int64_t)b * S + j] != pos_pad_id) { bmin = b; break; }
  for (int o = 32; o > 0; o >>= 1) bmin = min(bmin, __shfl_xor(bmin, o, 64));
  if (lane == 0) first[wave] = bmin;
  __syncthreads();
  bmin = min(min(first[0], first[1]), min(first[2], first[3]));
  const int64_t key = bmin < B ? pos[(int64_t)bmin * S + j] : pos_pad_id;
  const f32x4 zero = {0, 0, 0, 0};
  bool mix = false;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int64_t m = (int64_t)b * S + j, k = pos[m], sv = seg ? seg[m] : 0;
    const bool off = k != key && k != pos_pad_id, tx = sv != 0 && sv != 1;
    mix |= off;
    if (!tables_accumulate && (off || tx))
      for (int c = 0; c < H; c += 4) {
        if (off) *(f32x4*)(dptab + k * H + c) = zero;
        if (tx) *(f32x4*)(dtype_tab + sv * H + c) = zero;
      }
  }
  mix = __syncthreads_or(mix);
  if (!tables_accumulate && key != pos_pad_id)
    for (int c = 4 * threadIdx.x; c < H; c += 4 * blockDim.x) *(f32x4*)(dptab + key * H + c) = zero;
  if (threadIdx.x == 0) { colkey[j] = key; mixed[j] = mix; }
}

template <typename T, int VPL, bool FULL, bool ADV = false>
__global__ __launch_bounds__(256) void embed_bwd_pos_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ seg,
                                                            const int64_t* __restrict__ pos, const T* __restrict__ word,
                                                            const T* __restrict__ type, const T* __restrict__ ptab,
                                                            const float* __restrict__ gamma, const float* __restrict__ stats,
                                                            const T* __restrict__ dout, float* __restrict__ dtype_tab,
                                                            float* __restrict__ dptab, float* __restrict__ part, int* __restrict__ fixlist,
                                                            const int64_t* __restrict__ colkey, const int* __restrict__ mixed,
                                                            int* __restrict__ shared, int B, int S, int H, int64_t pos_pad_id, DropCfg drop,
                                                            const float* __restrict__ delta = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float acc[];  // [5][H] column sums (dgamma, dbeta, position, type 0, type 1)
  // (readfirstlane: the wave index is uniform, but only this tells the compiler - otherwise every token index below is a
  // "divergent" value and each readlane becomes a waterfall loop)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wpb = blockDim.x >> 6, nvec = H >> 2;
  const float invH = 1.0f / (float)H;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) fixlist[0] = 0;   // work list of embed_bwd_word_kernel (launched next)
  for (int i = threadIdx.x; i < 5 * H; i += blockDim.x) acc[i] = 0.f;
  __syncthreads();
  f32x4 ag[VPL], ab[VPL], gm[VPL], ap[VPL], t0[VPL], t1[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    ag[i] = ab[i] = ap[i] = t0[i] = t1[i] = f32x4{0, 0, 0, 0};
    const int c = lane + 64 * i;
    gm[i] = (c < nvec) ? *(const f32x4*)(gamma + 4 * c) : f32x4{0, 0, 0, 0};
  }
  const int j = blockIdx.x;
  const int64_t key0 = colkey[j];
  if (blockIdx.y == 0) {   // can row key0 receive anything besides this column's sum? (block-uniform branch)
    bool hit = false;
    for (int jj = threadIdx.x; jj < S; jj += blockDim.x) hit |= mixed[jj] || (jj != j && colkey[jj] == key0);
    hit = __syncthreads_or(hit);
    if (threadIdx.x == 0) shared[j] = hit;
  }
  const int bstep = gridDim.y * wpb, b0 = blockIdx.y + gridDim.y * wave;
  // this wave's tokens b0, b0 + bstep, ...: indices of up to 64 of them at a time, one per lane (no dependent scalar load per token)
  for (int base = b0; base < B; base += 64 * bstep) {
    const int bl = base + lane * bstep;
    const int64_t lrow = (int64_t)(bl < B ? bl : b0) * S + j;
    const int64_t lid = ids[lrow], lkey = pos[lrow], lsv = seg ? seg[lrow] : 0;
    int n = (B - base + bstep - 1) / bstep;
    if (n > 64) n = 64;
    auto bc = [&](int64_t v, int l) -> int64_t {
      const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l), hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), l);
      return (int64_t)(((uint64_t)hi << 32) | lo);
    };
    // groups of kEmbGroupPos tokens: all their rows are requested before the first is reduced
    for (int g0 = 0; g0 < n; g0 += kEmbGroupPos) {
      EmbTok<T, VPL> r[kEmbGroupPos];
      f32x4 dl[ADV ? kEmbGroupPos : 1][ADV ? VPL : 1];
#pragma unroll
      for (int u = 0; u < kEmbGroupPos; ++u) {
        const int k = (g0 + u < n) ? g0 + u : n - 1;
        emb_tok_load<T, VPL, FULL>(r[u], bc(lrow, k), bc(lid, k), bc(lsv, k), bc(lkey, k), word, type, ptab, stats, dout, H, lane, nvec);
        if constexpr (ADV) emb_tok_delta<VPL, FULL>(dl[u], bc(lrow, k), delta, H, lane, nvec);
      }
#pragma unroll
      for (int u = 0; u < kEmbGroupPos; ++u) {
        const int k = g0 + u;
        if (k >= n) break;
        const int64_t row = bc(lrow, k), key = bc(lkey, k), sv = bc(lsv, k);
        f32x4 o[VPL], d[VPL], xh[VPL];
        if constexpr (ADV) emb_tok_grad<T, VPL, FULL, true>(r[u], row, gm, o, d, xh, H, lane, nvec, invH, drop, dl[u]);
        else emb_tok_grad<T, VPL, FULL>(r[u], row, gm, o, d, xh, H, lane, nvec, invH, drop);
        const bool own_key = (key == key0), t_is0 = (sv == 0), t_is1 = (sv == 1);   // wave-uniform
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          ag[i] += d[i] * xh[i];
          ab[i] += d[i];
          if (own_key) ap[i] += o[i];
          if (t_is0) t0[i] += o[i];
          if (t_is1) t1[i] += o[i];
        }
        if ((!own_key && key != pos_pad_id) || (!t_is0 && !t_is1)) {   // the fallback: not reached by BERT / right-padded RoBERTa positions
#pragma unroll
          for (int i = 0; i < VPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nvec)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (!own_key && key != pos_pad_id) atomicAdd(dptab + key * H + 4 * c + e, o[i][e]);
                if (!t_is0 && !t_is1) atomicAdd(dtype_tab + sv * H + 4 * c + e, o[i][e]);
              }
          }
        }
      }
    }
  }
  for (int w = 0; w < wpb; ++w) {   // waves take turns, in wave order (no LDS float atomics, see ln_bwd_kernel)
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
          *(f32x4*)&acc[4 * c] += ag[i];
          *(f32x4*)&acc[H + 4 * c] += ab[i];
          *(f32x4*)&acc[2 * H + 4 * c] += ap[i];
          *(f32x4*)&acc[3 * H + 4 * c] += t0[i];
          *(f32x4*)&acc[4 * H + 4 * c] += t1[i];
        }
      }
    }
    __syncthreads();
  }
  const int nblk = gridDim.x * gridDim.y, bid = blockIdx.y * gridDim.x + blockIdx.x;
  for (int i = threadIdx.x; i < H; i += blockDim.x)
#pragma unroll
    for (int k = 0; k < 5; ++k) part[((int64_t)k * nblk + bid) * H + i] = acc[k * H + i];
}

// sums of the partial rows of embed_bwd_pos_kernel, fixed order.  grid (ceil(H / 32), 4 + ceil(S / 32)), block (32, 32):
//   y = 0, 1, 2, 3: dgamma, dbeta, token-type rows 0 / 1 = sum over all S * Y blocks (32 row lanes + an LDS tree);
//   y = 4 + g: thread row r owns position j = 32 g + r: position row colkey[j] = sum over the Y blocks (j, 0), (j, 1), ..., stored
//   (or added, `accum_tab`) when column j is the row's only contributor; a float atomic add otherwise (embed_bwd_colkey_kernel zeroed
//   the row when !accum_tab).  `accum_ln` / `accum_tab`: add to what the outputs hold.
__global__ __launch_bounds__(1024) void embed_bwd_finalize_kernel(const float* __restrict__ part, const int64_t* __restrict__ colkey,
                                                                  const int* __restrict__ shared, int S, int Y,
                                                                  int H, int n_types, int64_t pos_pad_id, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, float* __restrict__ dtype_tab,
                                                                  float* __restrict__ dptab, int accum_ln, int accum_tab) {
  __shared__ float sm[32][33];
  const int nblk = S * Y, col = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y;
  if (y >= 4) {
    const int j = (y - 4) * 32 + threadIdx.y;
    if (j >= S || col >= H) return;
    const int64_t key = colkey[j];
    if (key == pos_pad_id) return;
    const float* p = part + ((int64_t)2 * nblk + j) * H + col;      // blocks (j, 0), (j, 1), ...: bid = yy * S + j
    float s = 0.f;
    for (int yy = 0; yy < Y; ++yy) s += p[(int64_t)yy * S * H];
    float* o = dptab + key * H + col;
    if (shared[j]) atomicAdd(o, s);
    else *o = accum_tab ? *o + s : s;
    return;
  }
  float* outp = y == 0 ? dgamma : (y == 1 ? dbeta : (y == 2 ? dtype_tab : (n_types > 1 ? dtype_tab + H : nullptr)));
  const float* p = part + (int64_t)(y < 2 ? y : y + 1) * nblk * H + col;
  const int acc = y < 2 ? accum_ln : accum_tab;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < H && outp != nullptr) {
    int b = threadIdx.y;
    for (; b + 96 < nblk; b += 128) {
      s0 += p[(int64_t)b * H]; s1 += p[(int64_t)(b + 32) * H]; s2 += p[(int64_t)(b + 64) * H]; s3 += p[(int64_t)(b + 96) * H];
    }
    for (; b < nblk; b += 32) s0 += p[(int64_t)b * H];
  }
  sm[threadIdx.y][threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (threadIdx.y == 0 && col < H && outp != nullptr) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) s += sm[r][threadIdx.x];
    outp[col] = acc ? outp[col] + s : s;
  }
}

// sorted id of sorted position i (out of range: sentinels that equal no id and not each other)
__device__ __forceinline__ int64_t emb_sid(const int32_t* __restrict__ perm, const int64_t* __restrict__ ids, int64_t i, int64_t M) {
  return i < 0 ? -2 : (i >= M ? -3 : ids[perm[i]]);
}

template <typename T, int VPL, bool FULL, bool ADV = false>
__global__ __launch_bounds__(256) void embed_bwd_word_kernel(const int32_t* __restrict__ perm, const int64_t* __restrict__ ids,
                                                             const int64_t* __restrict__ seg, const int64_t* __restrict__ pos,
                                                             const T* __restrict__ word, const T* __restrict__ type,
                                                             const T* __restrict__ ptab, const float* __restrict__ gamma,
                                                             const float* __restrict__ stats, const T* __restrict__ dout,
                                                             float* __restrict__ dword, float* __restrict__ wpart, int* __restrict__ fixlist,
                                                             int64_t M, int H, int tpc, int64_t word_pad_id, int accumulate, DropCfg drop,
                                                             const float* __restrict__ delta = nullptr) {
  const int lane = threadIdx.x & 63, nvec = H >> 2;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: see the pos kernel
  const int64_t i0 = c * tpc;
  if (i0 >= M) return;
  const int64_t i1 = (i0 + tpc < M) ? i0 + tpc : M;
  const float invH = 1.0f / (float)H;
  // lane l holds sorted position i0 - 1 + l: the chunk's token rows and ids (tpc <= 62) plus the id before and after the chunk
  const int n = (int)(i1 - i0);
  const int64_t li = i0 - 1 + lane;
  const bool lin = lane <= n + 1 && li >= 0 && li < M;
  const int64_t lrow = lin ? perm[li] : 0;
  const int64_t lid = lin ? ids[lrow] : (li < 0 ? -2 : -3);          // sentinels equal no id
  const int64_t lsv = (seg && lin) ? seg[lrow] : 0;
  const int64_t lkey = lin ? pos[lrow] : 0;
  auto bc = [&](int64_t v, int l) -> int64_t {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l), hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
  };
  if (bc(lid, 1) == word_pad_id && bc(lid, n) == word_pad_id) return;   // sorted: the whole chunk is padding (no gradient)
  f32x4 gm[VPL], acc[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int cc = lane + 64 * i;
    gm[i] = (cc < nvec) ? *(const f32x4*)(gamma + 4 * cc) : f32x4{0, 0, 0, 0};
    acc[i] = f32x4{0, 0, 0, 0};
  }
  bool run_began_here = true;                                // does the running sum hold the FIRST token of its id?
  int64_t run_id = -5;
  for (int g0 = 1; g0 <= n; g0 += kEmbGroupWord) {               // groups of kEmbGroupWord tokens: every row requested before the first is reduced
    EmbTok<T, VPL> r[kEmbGroupWord];
    f32x4 dl[ADV ? kEmbGroupWord : 1][ADV ? VPL : 1];
#pragma unroll
    for (int u = 0; u < kEmbGroupWord; ++u) {
      const int k = (g0 + u <= n) ? g0 + u : n;
      emb_tok_load<T, VPL, FULL>(r[u], bc(lrow, k), bc(lid, k), bc(lsv, k), bc(lkey, k), word, type, ptab, stats, dout, H, lane, nvec);
      if constexpr (ADV) emb_tok_delta<VPL, FULL>(dl[u], bc(lrow, k), delta, H, lane, nvec);
    }
#pragma unroll
    for (int u = 0; u < kEmbGroupWord; ++u) {
      const int k = g0 + u;
      if (k > n) break;
      const int64_t id = bc(lid, k), row = bc(lrow, k);
      if (id == word_pad_id) continue;                       // padding rows carry no gradient
      if (id != run_id) {                                    // a new run starts with this token
        run_id = id;
        run_began_here = (bc(lid, k - 1) != id);             // k = 1: compares with the id before the chunk
#pragma unroll
        for (int i = 0; i < VPL; ++i) acc[i] = f32x4{0, 0, 0, 0};
      }
      f32x4 o[VPL], d[VPL], xh[VPL];
      if constexpr (ADV) emb_tok_grad<T, VPL, FULL, true>(r[u], row, gm, o, d, xh, H, lane, nvec, invH, drop, dl[u]);
      else emb_tok_grad<T, VPL, FULL>(r[u], row, gm, o, d, xh, H, lane, nvec, invH, drop);
#pragma unroll
      for (int i = 0; i < VPL; ++i) acc[i] += o[i];
      const int64_t id_next = bc(lid, k + 1);                // k = n: the id after the chunk
      if (id_next != id) {                                   // the run ends with this token
        float* dst = run_began_here ? dword + id * H : wpart + (c * 2 + 0) * H;
        const bool add = run_began_here && accumulate;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int cc = lane + 64 * i;
          if (FULL || cc < nvec) *(f32x4*)(dst + 4 * cc) = add ? *(const f32x4*)(dst + 4 * cc) + acc[i] : acc[i];
        }
      } else if (k == n) {                                   // the chunk ends inside the run
        float* dst = wpart + (c * 2 + (run_began_here ? 1 : 0)) * H;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int cc = lane + 64 * i;
          if (FULL || cc < nvec) *(f32x4*)(dst + 4 * cc) = acc[i];
        }
        // the chunk in which a boundary-crossing run BEGINS owns its fix-up (order of the list: irrelevant - every entry is a
        // different table row, and the additions inside a row are ordered by chunk)
        if (run_began_here && lane == 0) fixlist[1 + atomicAdd(fixlist, 1)] = (int)c;
      }
    }
  }
}

// Fix-up of the runs that cross chunk boundaries: a fixed grid of blocks walks embed_bwd_word_kernel's work list (chunks in
// which such a run begins); the block adds the run's partial rows in chunk order and stores the table row.
__global__ __launch_bounds__(256) void embed_bwd_wordfix_kernel(const int32_t* __restrict__ perm, const int64_t* __restrict__ ids,
                                                                const float* __restrict__ wpart, const int* __restrict__ fixlist,
                                                                float* __restrict__ dword, int64_t M, int H, int tpc, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float sm[];       // [4][H]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nvec = H >> 2;
  int* first = (int*)sm;                                           // [4], before the row sums use the buffer
  const int count = fixlist[0];
  for (int item = blockIdx.x; item < count; item += gridDim.x) {
    const int64_t c = fixlist[1 + item];
    const int64_t i1 = (c + 1) * tpc;                              // < M: the run continues past the chunk
    const int64_t id = emb_sid(perm, ids, i1 - 1, M);
    // chunks c + 1 .. ce continue the run (slot 0 each); the run ends in chunk ce = the first chunk q > c whose end is the end of
    // the data or is followed by another id.  256 candidates are probed at once (a serial walk costs two dependent loads per
    // chunk: 73 us for the (n_best + 1) x B [SEP] tokens of a batch).
    int64_t ce = c + 1;
    for (int64_t base = c + 1;; base += 256) {
      const int64_t q = base + threadIdx.x;
      const int64_t e1 = ((q + 1) * tpc < M) ? (q + 1) * tpc : M;
      const bool ends = e1 >= M || emb_sid(perm, ids, e1, M) != id;
      const unsigned long long m = __ballot(ends);
      if (lane == 0) first[wave] = m ? (__ffsll((long long)m) - 1) + 64 * wave : 1 << 30;
      __syncthreads();
      const int f = min(min(first[0], first[1]), min(first[2], first[3]));
      __syncthreads();
      if (f < (1 << 30)) { ce = base + f; break; }
    }
    for (int cc = lane; cc < nvec; cc += 64) {
      f32x4 s = {0, 0, 0, 0};
      int64_t q = c + 1 + wave;
      for (; q + 28 <= ce; q += 32) {                              // eight rows of this wave in flight, added in chunk order
        f32x4 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = *(const f32x4*)(wpart + ((q + 4 * u) * 2) * H + 4 * cc);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += a[u];
      }
      for (; q <= ce; q += 4) s += *(const f32x4*)(wpart + (q * 2) * H + 4 * cc);
      *(f32x4*)(sm + wave * H + 4 * cc) = s;
    }
    __syncthreads();
    for (int cc = threadIdx.x; cc < nvec; cc += blockDim.x) {
      f32x4 s = *(const f32x4*)(wpart + (c * 2 + 1) * H + 4 * cc);   // the part of the run inside its first chunk
      s += *(const f32x4*)(sm + 4 * cc); s += *(const f32x4*)(sm + H + 4 * cc);
      s += *(const f32x4*)(sm + 2 * H + 4 * cc); s += *(const f32x4*)(sm + 3 * H + 4 * cc);
      float* dst = dword + id * H + 4 * cc;
      *(f32x4*)dst = accumulate ? *(const f32x4*)dst + s : s;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ void cls_scatter_kernel(const float* __restrict__ dcls, T* __restrict__ dh, int64_t nvec_total, int S, int H) {
  const int nvec = H >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec_total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / nvec;
    const int c = (int)(i - row * nvec);
    f32x4 v = {0, 0, 0, 0};
    if (row % S == 0) v = *(const f32x4*)(dcls + (row / S) * H + 4 * c);
    Vec4<T>::store(dh + row * H + 4 * c, v);
  }
}

__global__ void cast_bf16_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int64_t n) {
  const int64_t n8 = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    Vec8<float>::load(src + 8 * i, v);
    Vec8<bf16>::store(dst + 8 * i, v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n8 << 3; i < n; ++i) dst[i] = (bf16)src[i];
}

// ---- sparse exchange of word-embedding gradient rows (data parallel, large vocabularies; trainer.GradReducer) ----------------
// gather: slot i < n takes row rows[i] of the table (and its id), slots n .. cap-1 are padding (id -1, zeros)
__global__ __launch_bounds__(256) void rows_gather_kernel(const float* __restrict__ table, const int64_t* __restrict__ rows, int64_t n,
                                                          int64_t* __restrict__ ids_out, float* __restrict__ vals_out, int H) {
  const int64_t i = blockIdx.x;
  const int64_t id = (i < n) ? rows[i] : -1;
  if (threadIdx.x == 0) ids_out[i] = id;
  const int nvec = H >> 2;
  for (int c = threadIdx.x; c < nvec; c += blockDim.x) {
    const f32x4 v = (id >= 0) ? *(const f32x4*)(table + id * H + 4 * c) : f32x4{0, 0, 0, 0};
    *(f32x4*)(vals_out + i * H + 4 * c) = v;
  }
}
// table[ids[i]] = 0 (vals == nullptr) or table[ids[i]] += vals[i]; ids unique within one call (negative ids are padding)
__global__ __launch_bounds__(256) void rows_update_kernel(float* __restrict__ table, const int64_t* __restrict__ ids,
                                                          const float* __restrict__ vals, int H) {
  const int64_t i = blockIdx.x;
  const int64_t id = ids[i];
  if (id < 0) return;
  const int nvec = H >> 2;
  for (int c = threadIdx.x; c < nvec; c += blockDim.x) {
    float* p = table + id * H + 4 * c;
    *(f32x4*)p = vals ? *(const f32x4*)p + *(const f32x4*)(vals + i * H + 4 * c) : f32x4{0, 0, 0, 0};
  }
}

static inline int vpl_for(int H) { return ((H >> 2) + 63) / 64; }
static inline int grid_rows(int64_t M, int wpb) {
  int64_t g = (M + wpb - 1) / wpb;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

#define DISPATCH_VPL(H, CALL)                                     \
  do {                                                            \
    const int vpl__ = vpl_for(H);                                 \
    if (vpl__ <= 1) { constexpr int VPL = 1; CALL; }              \
    else if (vpl__ <= 2) { constexpr int VPL = 2; CALL; }         \
    else if (vpl__ <= 3) { constexpr int VPL = 3; CALL; }         \
    else if (vpl__ <= 4) { constexpr int VPL = 4; CALL; }         \
    else { constexpr int VPL = 8; CALL; }                         \
  } while (0)

static int check_h(int H) {
  NB_CHECK(H > 0 && H % 4 == 0 && H <= 2048, NBEST_ERR_SHAPE, "hidden size %d must be a multiple of 4 and <= 2048", H);
  return NBEST_OK;
}

// ---- deferred finalizes ----------------------------------------------------------------------------------------------
// A backward layer has four producers of partial rows (LayerNorm-backward x 2, the fused column sums of the dU GEMM, the
// attention backward's bias gradient); finalised one by one that is four 5-us launches of pure latency per layer (49 per
// step).  nbest_encoder_backward opens a batch per layer: while it is open finalize() only RECORDS its job (the producers
// write their partial rows into regions of their own) and one launch at the end of the layer sums them all.
constexpr int kMaxBatch = 8;
struct RowredJob {
  const float* part;
  int nblk, N, nout;
  RowredOut o;
};
struct RowredJobs {
  RowredJob j[kMaxBatch];
};
thread_local RowredJobs* t_batch = nullptr;
thread_local int t_batch_n = 0;

__global__ __launch_bounds__(1024) void rowred_finalize_multi_kernel(RowredJobs jobs) {
  __shared__ float sm[32][33];
  const RowredJob& jb = jobs.j[blockIdx.z];
  const int k = blockIdx.y, N = jb.N, nblk = jb.nblk;
  if (k >= jb.nout || (int)blockIdx.x * 32 >= N) return;        // block-uniform
  float* outp = jb.o.out[k];
  const int col = blockIdx.x * 32 + threadIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < N && outp != nullptr) {
    const float* p = jb.part + (int64_t)k * nblk * N + col;
    int b = threadIdx.y;
    for (; b + 96 < nblk; b += 128) {
      s0 += p[(int64_t)b * N]; s1 += p[(int64_t)(b + 32) * N]; s2 += p[(int64_t)(b + 64) * N]; s3 += p[(int64_t)(b + 96) * N];
    }
    for (; b < nblk; b += 32) s0 += p[(int64_t)b * N];
  }
  sm[threadIdx.y][threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (threadIdx.y == 0 && col < N && outp != nullptr) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) s += sm[r][threadIdx.x];
    outp[col] = jb.o.accumulate[k] ? outp[col] + s : s;
  }
}

static int finalize(const float* part, int nblk, int N, float* o0, int a0, float* o1, int a1, float* o2, int a2,
                    hipStream_t st) {
  RowredOut o;
  o.out[0] = o0; o.out[1] = o1; o.out[2] = o2;
  o.accumulate[0] = a0; o.accumulate[1] = a1; o.accumulate[2] = a2;
  const int nout = o2 ? 3 : (o1 ? 2 : 1);
  if (t_batch != nullptr && t_batch_n < kMaxBatch) {              // deferred: summed by nbest_internal_rowred_batch_flush
    RowredJob& jb = t_batch->j[t_batch_n++];
    jb.part = part; jb.nblk = nblk; jb.N = N; jb.nout = nout; jb.o = o;
    return NBEST_OK;
  }
  rowred_finalize_kernel<<<dim3((N + 31) / 32, nout), dim3(32, 32), 0, st>>>(part, nblk, N, o);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

}  // namespace

// Deferred finalizes (see RowredJobs): between begin and flush every finalize of THIS thread is recorded instead of launched; the
// caller guarantees that the recorded producers wrote their partial rows to distinct memory.  flush launches one kernel for all.
static thread_local RowredJobs t_jobs_storage;
void nbest_internal_rowred_batch_begin() { t_batch = &t_jobs_storage; t_batch_n = 0; }
void nbest_internal_rowred_batch_abort() { t_batch = nullptr; t_batch_n = 0; }     // error paths: never leave a batch open
int nbest_internal_rowred_batch_flush(hipStream_t st) {
  RowredJobs* b = t_batch;
  const int n = t_batch_n;
  t_batch = nullptr; t_batch_n = 0;
  if (b == nullptr || n == 0) return NBEST_OK;
  int maxN = 0, maxout = 1;
  for (int i = 0; i < n; ++i) { if (b->j[i].N > maxN) maxN = b->j[i].N; if (b->j[i].nout > maxout) maxout = b->j[i].nout; }
  rowred_finalize_multi_kernel<<<dim3((maxN + 31) / 32, maxout, n), dim3(32, 32), 0, st>>>(*b);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

// out[n] (+)= sum over `nrows` partial rows (used by the fused bias-gradient epilogues of the GEMM / attention)
int nbest_internal_partial_rows_sum(const float* part, int nrows, int N, float* out, int accumulate, hipStream_t st) {
  return finalize(part, nrows, N, out, accumulate, nullptr, 0, nullptr, 0, st);
}

extern "C" size_t nbest_rowred_ws_bytes(int64_t M, int64_t N) {
  int64_t b = (M + 31) / 32;
  if (b < 1) b = 1;
  if (b > kMaxLnBwdBlocks) b = kMaxLnBwdBlocks;
  return (size_t)3 * b * N * sizeof(float);
}
constexpr int kEmbTpc = 16;   // sorted tokens per wave of embed_bwd_word_kernel
extern "C" size_t nbest_embed_bwd_ws_bytes(int64_t M, int64_t H) {
  // partial rows of embed_bwd_pos_kernel (<= kMaxLnBwdBlocks blocks x 5 quantities) | column keys (int64) and the mixed / shared flags
  // (int, int) of the <= kMaxLnBwdBlocks positions | two partial rows per chunk of embed_bwd_word_kernel | the fix-up work list (a
  // counter + one chunk id per entry)
  const int64_t chunks = (M + kEmbTpc - 1) / kEmbTpc;
  return (size_t)5 * kMaxLnBwdBlocks * H * sizeof(float) + (size_t)kMaxLnBwdBlocks * (sizeof(int64_t) + 2 * sizeof(int)) +
         (size_t)chunks * 2 * H * sizeof(float) + (size_t)(chunks + 4) * sizeof(int);
}

// y8 != NULL (bf16, H % 256 == 0, H <= 1024 only): also write the e4m3 copy of y that the next fp8 forward GEMM reads; a_new is
// recorded into only together with y8 (a calibration pass measures y with nbest_internal_amax_bf16)
int nbest_internal_layernorm_fwd8(const void* x, const float* gamma, const float* beta, void* y, void* y8, float* stats,
                                  int64_t M, int H, float eps, int dtype, nbest_stream_t stream, const uint32_t* a_prev, uint32_t* a_new) {
  if (int e = check_h(H)) return e;
  NB_CHECK(x && gamma && beta && y && stats && M > 0, NBEST_ERR_ARG, "layernorm_fwd: null pointer or M <= 0");
  NB_CHECK(!y8 || (dtype == NBEST_BF16 && H % 256 == 0 && H <= 1024), NBEST_ERR_SHAPE, "layernorm_fwd: fp8 copy needs bf16 and H in {256..1024}");
  hipStream_t st = (hipStream_t)stream;
  const int grid0 = grid_rows(M, 4);
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (ln_fwd_kernel<float, VPL><<<grid0, 256, 0, st>>>((const float*)x, gamma, beta, (float*)y, stats, M, H, eps)));
  } else if (dtype == NBEST_BF16 && H % 256 == 0 && H <= 1024) {
    const int grid = grid0 < 1024 ? grid0 : 1024;   // 512 ... 4096 blocks tie at 17 us for 100 MB (5.9 TB/s); 8192: 19.5
    switch (H / 256) {
      case 1: ln_fwd_fast_kernel<1><<<grid, 256, 0, st>>>((const bf16*)x, gamma, beta, (bf16*)y, stats, M, eps, (uint8_t*)y8, a_prev, a_new); break;
      case 2: ln_fwd_fast_kernel<2><<<grid, 256, 0, st>>>((const bf16*)x, gamma, beta, (bf16*)y, stats, M, eps, (uint8_t*)y8, a_prev, a_new); break;
      case 3: ln_fwd_fast_kernel<3><<<grid, 256, 0, st>>>((const bf16*)x, gamma, beta, (bf16*)y, stats, M, eps, (uint8_t*)y8, a_prev, a_new); break;
      default: ln_fwd_fast_kernel<4><<<grid, 256, 0, st>>>((const bf16*)x, gamma, beta, (bf16*)y, stats, M, eps, (uint8_t*)y8, a_prev, a_new); break;
    }
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (ln_fwd_kernel<bf16, VPL><<<grid0, 256, 0, st>>>((const bf16*)x, gamma, beta, (bf16*)y, stats, M, H, eps)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "layernorm_fwd: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats,
                                   int64_t M, int H, float eps, int dtype, nbest_stream_t stream) {
  return nbest_internal_layernorm_fwd8(x, gamma, beta, y, nullptr, stats, M, H, eps, dtype, stream, nullptr, nullptr);
}

// f8 (bf16 fast path only): e4m3 copy + amax of the gradient the dense-layer GEMMs read (dx_drop under dropout, else dx).  Both are
// taken from the fp32 value BEFORE its bf16 rounding (the attention and LayerNorm-forward producers round the stored bf16 value): the
// byte is e4m3(fp32 . s), a dropped element is byte 0, and bf16(recorded amax) = max |bf16 tensor|.  The kernel writes the copy
// only where it records, so out8 or amax_prev without amax_new is refused.  Pinned by tests/test_fp8_producers_gpu.py.
int nbest_internal_layernorm_bwd8(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                                  void* dx_drop, float* dgamma, float* dbeta, float* dbias, int64_t M, int H, int dtype,
                                  int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws,
                                  size_t ws_bytes, nbest_stream_t stream, Fp8Grad f8) {
  if (int e = check_h(H)) return e;
  // any fp8 argument needs the fast kernels (the generic ones know none of them, and store dx_drop unconditionally); a copy is written
  // only by the code that records, so out8 without amax_new would be a silent no-op: refused
  NB_CHECK(!(f8.out8 || f8.amax_prev || f8.amax_new) || (dtype == NBEST_BF16 && H % 256 == 0 && H <= 1024), NBEST_ERR_SHAPE,
           "layernorm_bwd: fp8 copy needs bf16 and H in {256..1024}");
  NB_CHECK(!(f8.out8 || f8.amax_prev) || f8.amax_new, NBEST_ERR_ARG, "layernorm_bwd: the fp8 copy is written only together with the amax record (amax_new)");
  // dgamma == dbeta == dbias == NULL (the no_param_grad backward of nbest_encoder_backward): dx / dx_drop only, no workspace, no finalize
  const bool params = dgamma || dbeta || dbias;
  NB_CHECK(dy && x && stats && gamma && dx && M > 0 && (!params || (dgamma && dbeta && ws)), NBEST_ERR_ARG, "layernorm_bwd: null pointer");
  NB_CHECK(!params || ws_bytes >= nbest_rowred_ws_bytes(M, H), NBEST_ERR_WORKSPACE, "layernorm_bwd: workspace too small");
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  NB_CHECK(d.thr16 == 0 || (dx_drop && dx_drop != dx) || (!dx_drop && f8.out8), NBEST_ERR_ARG, "layernorm_bwd: dropout needs a separate dx_drop buffer");
  NB_CHECK(M * (int64_t)H < (int64_t)1 << 32 || d.thr16 == 0, NBEST_ERR_SHAPE, "layernorm_bwd: dropout counter overflow");
  hipStream_t st = (hipStream_t)stream;
  int nblk = (int)((M + 31) / 32 < 1 ? 1 : ((M + 31) / 32 > kMaxLnBwdBlocks ? kMaxLnBwdBlocks : (M + 31) / 32));
  if (nblk > 512) nblk = 512;   // isolated, 256 and 512 blocks tie (32 us for 200 MB); inside the step 512 is faster (35 vs 44 us)
  int rpb = (int)((M + nblk - 1) / nblk);
  nblk = (int)((M + rpb - 1) / rpb);
  constexpr int waves = 4;   // 8: measured in the step, see profiles/README.md
  float* part = (float*)ws;
  const size_t smem = (size_t)3 * H * sizeof(float);
  const int wb = dbias ? 1 : 0;
  if (!params) {   // the PARAMS = false instantiations: same grid, same dx arithmetic, no column sums
    if (dtype == NBEST_F32) {
      DISPATCH_VPL(H, (ln_bwd_kernel<float, VPL, false><<<nblk, 256, 0, st>>>((const float*)dy, (const float*)x, stats, gamma,
                                                                               (float*)dx, (float*)dx_drop, nullptr, M, H, rpb, 0, d)));
    } else if (dtype == NBEST_BF16 && H % 256 == 0 && H <= 1024) {
#define NB_LNB0(V, D) ln_bwd_fast_kernel<V, D, false, waves, false><<<nblk, waves * 64, 0, st>>>((const bf16*)dy, (const bf16*)x, stats, gamma, \
                                                                                               (bf16*)dx, (bf16*)dx_drop, nullptr, M, rpb, d, f8)
#define NB_LNB0_V(V)                      \
  do {                                     \
    if (d.thr16) NB_LNB0(V, true);         \
    else NB_LNB0(V, false);                \
  } while (0)
      switch (H / 256) {
        case 1: NB_LNB0_V(1); break;
        case 2: NB_LNB0_V(2); break;
        case 3: NB_LNB0_V(3); break;
        default: NB_LNB0_V(4); break;
      }
#undef NB_LNB0_V
#undef NB_LNB0
    } else if (dtype == NBEST_BF16) {
      DISPATCH_VPL(H, (ln_bwd_kernel<bf16, VPL, false><<<nblk, 256, 0, st>>>((const bf16*)dy, (const bf16*)x, stats, gamma,
                                                                              (bf16*)dx, (bf16*)dx_drop, nullptr, M, H, rpb, 0, d)));
    } else NB_CHECK(false, NBEST_ERR_DTYPE, "layernorm_bwd: bad dtype %d", dtype);
    NB_LAUNCH_CHECK();
    return NBEST_OK;
  }
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (ln_bwd_kernel<float, VPL><<<nblk, 256, smem, st>>>((const float*)dy, (const float*)x, stats, gamma,
                                                                         (float*)dx, (float*)dx_drop, part, M, H, rpb, wb, d)));
  } else if (dtype == NBEST_BF16 && H % 256 == 0 && H <= 1024) {
#define NB_LNB(V, D, B)                                                                                                        \
  do {                                                                                                                         \
    if (waves == 8) {                                                                                                          \
      (void)hipFuncSetAttribute((const void*)ln_bwd_fast_kernel<V, D, B, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 3 * H * 4); \
      ln_bwd_fast_kernel<V, D, B, 8><<<nblk, 512, 8 * 3 * H * 4, st>>>((const bf16*)dy, (const bf16*)x, stats, gamma, (bf16*)dx,       \
                                                                       (bf16*)dx_drop, part, M, rpb, d, f8);                   \
    } else {                                                                                                                   \
      ln_bwd_fast_kernel<V, D, B, 4><<<nblk, 256, 4 * 3 * H * 4, st>>>((const bf16*)dy, (const bf16*)x, stats, gamma, (bf16*)dx,       \
                                                                       (bf16*)dx_drop, part, M, rpb, d, f8);                   \
    }                                                                                                                          \
  } while (0)
#define NB_LNB_V(V)                                                     \
  do {                                                                  \
    if (d.thr16) { if (wb) NB_LNB(V, true, true); else NB_LNB(V, true, false); } \
    else { if (wb) NB_LNB(V, false, true); else NB_LNB(V, false, false); }       \
  } while (0)
    switch (H / 256) {
      case 1: NB_LNB_V(1); break;
      case 2: NB_LNB_V(2); break;
      case 3: NB_LNB_V(3); break;
      default: NB_LNB_V(4); break;
    }
#undef NB_LNB_V
#undef NB_LNB
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (ln_bwd_kernel<bf16, VPL><<<nblk, 256, smem, st>>>((const bf16*)dy, (const bf16*)x, stats, gamma,
                                                                        (bf16*)dx, (bf16*)dx_drop, part, M, H, rpb, wb, d)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "layernorm_bwd: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return finalize(part, nblk, H, dgamma, accumulate, dbeta, accumulate, dbias, accumulate, st);
}

extern "C" int nbest_layernorm_bwd(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                                   void* dx_drop, float* dgamma, float* dbeta, float* dbias, int64_t M, int H, int dtype,
                                   int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws,
                                   size_t ws_bytes, nbest_stream_t stream) {
  return nbest_internal_layernorm_bwd8(dy, x, stats, gamma, dx, dx_drop, dgamma, dbeta, dbias, M, H, dtype, accumulate, drop_p, seed,
                                       drop_stream, ws, ws_bytes, stream, Fp8Grad{nullptr, nullptr, nullptr});
}

// The fp8 producers on their own (include/nbest_hip.h): the arguments nbest_encoder_forward / _backward pass, forwarded unchanged
extern "C" int nbest_layernorm_fwd_fp8(const void* x, const float* gamma, const float* beta, void* y, void* y8, float* stats, int64_t M,
                                       int H, float eps, int dtype, const uint32_t* amax_prev, uint32_t* amax_new, nbest_stream_t stream) {
  // (the kernels without a copy would ignore a history or a slot block: refused like a copy)
  NB_CHECK(!(y8 || amax_prev || amax_new) || (dtype == NBEST_BF16 && H % 256 == 0 && H <= 1024), NBEST_ERR_SHAPE,
           "layernorm_fwd_fp8: fp8 copy needs bf16 and H in {256..1024}");
  return nbest_internal_layernorm_fwd8(x, gamma, beta, y, y8, stats, M, H, eps, dtype, stream, amax_prev, amax_new);
}
extern "C" int nbest_layernorm_bwd_fp8(const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_drop,
                                       float* dgamma, float* dbeta, float* dbias, int64_t M, int H, int dtype, int accumulate,
                                       float drop_p, uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, void* out8,
                                       const uint32_t* amax_prev, uint32_t* amax_new, nbest_stream_t stream) {
  return nbest_internal_layernorm_bwd8(dy, x, stats, gamma, dx, dx_drop, dgamma, dbeta, dbias, M, H, dtype, accumulate, drop_p, seed,
                                       drop_stream, ws, ws_bytes, stream, Fp8Grad{(uint8_t*)out8, amax_prev, amax_new});
}

extern "C" int nbest_colsum(const void* X, float* out, int64_t M, int64_t N, int64_t ld, int dtype, int accumulate,
                            void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(X && out && ws && M > 0 && N > 0 && N % 4 == 0 && ld % 4 == 0, NBEST_ERR_ARG, "colsum: bad arguments");
  NB_CHECK(ws_bytes >= nbest_rowred_ws_bytes(M, N), NBEST_ERR_WORKSPACE, "colsum: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = rowred_blocks(M);
  const int rpb = (int)((M + nblk - 1) / nblk);
  float* part = (float*)ws;
  dim3 grid((unsigned)((N + 255) / 256), nblk);
  if (dtype == NBEST_F32) colsum_kernel<float><<<grid, 256, 0, st>>>((const float*)X, part, M, N, ld, rpb);
  else if (dtype == NBEST_BF16) colsum_kernel<bf16><<<grid, 256, 0, st>>>((const bf16*)X, part, M, N, ld, rpb);
  else NB_CHECK(false, NBEST_ERR_DTYPE, "colsum: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return finalize(part, nblk, (int)N, out, accumulate, nullptr, 0, nullptr, 0, st);
}

extern "C" int nbest_embed_ln_fwd(const int64_t* ids, const int64_t* seg, const int64_t* pos, const void* word,
                                  const void* type, const void* ptab, const float* gamma, const float* beta, void* out,
                                  float* stats, int64_t M, int H, float eps, int dtype, float drop_p, uint64_t seed,
                                  uint32_t drop_stream, nbest_stream_t stream) {
  if (int e = check_h(H)) return e;
  NB_CHECK(ids && pos && word && type && ptab && gamma && beta && out && stats && M > 0, NBEST_ERR_ARG, "embed_ln_fwd: null pointer");
  NB_CHECK(M * (int64_t)H < (int64_t)1 << 32, NBEST_ERR_SHAPE, "embed_ln_fwd: M*H must fit 32 bits (dropout counter)");
  hipStream_t st = (hipStream_t)stream;
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  const int grid = grid_rows(M, 4);
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (embed_fwd_kernel<float, VPL><<<grid, 256, 0, st>>>(ids, seg, pos, (const float*)word, (const float*)type,
                                                                        (const float*)ptab, gamma, beta, (float*)out, stats, M, H, eps, d)));
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (embed_fwd_kernel<bf16, VPL><<<grid, 256, 0, st>>>(ids, seg, pos, (const bf16*)word, (const bf16*)type,
                                                                       (const bf16*)ptab, gamma, beta, (bf16*)out, stats, M, H, eps, d)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "embed_ln_fwd: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_embed_ln_fwd_interp(const int64_t* ids, const int64_t* base_ids, const float* alpha, const int64_t* seg,
                                         const int64_t* pos, const void* word, const void* type, const void* ptab, const float* gamma,
                                         const float* beta, void* out, float* stats, int B, int S, int H, float eps, int dtype,
                                         float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t stream) {
  if (int e = check_h(H)) return e;
  NB_CHECK(ids && base_ids && alpha && pos && word && type && ptab && gamma && beta && out && stats && B > 0 && S > 0, NBEST_ERR_ARG,
           "embed_ln_fwd_interp: null pointer or empty batch");
  const int64_t M = (int64_t)B * S;
  NB_CHECK(M * (int64_t)H < (int64_t)1 << 32, NBEST_ERR_SHAPE, "embed_ln_fwd_interp: M*H must fit 32 bits (dropout counter)");
  hipStream_t st = (hipStream_t)stream;
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  const int grid = grid_rows(M, 4);
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (embed_fwd_kernel<float, VPL, true><<<grid, 256, 0, st>>>(ids, seg, pos, (const float*)word, (const float*)type, (const float*)ptab,
                                                                              gamma, beta, (float*)out, stats, M, H, eps, d, base_ids, alpha, S)));
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (embed_fwd_kernel<bf16, VPL, true><<<grid, 256, 0, st>>>(ids, seg, pos, (const bf16*)word, (const bf16*)type, (const bf16*)ptab,
                                                                             gamma, beta, (bf16*)out, stats, M, H, eps, d, base_ids, alpha, S)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "embed_ln_fwd_interp: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_embed_ln_fwd_adv(const int64_t* ids, const int64_t* seg, const int64_t* pos, const void* word, const void* type,
                                      const void* ptab, const float* gamma, const float* beta, const float* delta, void* out, float* stats,
                                      int64_t M, int H, float eps, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                                      nbest_stream_t stream) {
  if (int e = check_h(H)) return e;
  NB_CHECK(ids && pos && word && type && ptab && gamma && beta && delta && out && stats && M > 0, NBEST_ERR_ARG, "embed_ln_fwd_adv: null pointer");
  NB_CHECK(M * (int64_t)H < (int64_t)1 << 32, NBEST_ERR_SHAPE, "embed_ln_fwd_adv: M*H must fit 32 bits (dropout counter)");
  hipStream_t st = (hipStream_t)stream;
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  const int grid = grid_rows(M, 4);
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (embed_fwd_kernel<float, VPL, false, true><<<grid, 256, 0, st>>>(ids, seg, pos, (const float*)word, (const float*)type, (const float*)ptab,
                                                                                     gamma, beta, (float*)out, stats, M, H, eps, d, nullptr, nullptr, 1, delta)));
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (embed_fwd_kernel<bf16, VPL, false, true><<<grid, 256, 0, st>>>(ids, seg, pos, (const bf16*)word, (const bf16*)type, (const bf16*)ptab,
                                                                                    gamma, beta, (bf16*)out, stats, M, H, eps, d, nullptr, nullptr, 1, delta)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "embed_ln_fwd_adv: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" size_t nbest_embed_adv_ws_bytes(int B, int S) { return (size_t)(B > 0 ? B : 0) * (size_t)(S > 0 ? S : 0) * sizeof(float); }

extern "C" int nbest_embed_adv_delta(const int64_t* ids, const int64_t* seg, const int64_t* pos, const uint8_t* key_mask, const void* word,
                                     const void* type, const void* ptab, const float* gamma, const void* dout, float* delta, float* norm,
                                     int B, int S, int H, float eps, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                                     float epsilon, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  if (int e = check_h(H)) return e;
  NB_CHECK(ids && pos && key_mask && word && type && ptab && gamma && dout && delta && norm && ws, NBEST_ERR_ARG, "embed_adv_delta: null pointer");
  NB_CHECK(B > 0 && S > 0, NBEST_ERR_SHAPE, "embed_adv_delta: B=%d, S=%d must be positive", B, S);
  NB_CHECK(epsilon >= 0.f && epsilon <= 3.4028234e38f, NBEST_ERR_ARG, "embed_adv_delta: epsilon %g must be finite and >= 0", (double)epsilon);
  NB_CHECK(ws_bytes >= nbest_embed_adv_ws_bytes(B, S), NBEST_ERR_WORKSPACE, "embed_adv_delta: workspace too small");
  const int64_t M = (int64_t)B * S;
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  NB_CHECK(M * (int64_t)H < (int64_t)1 << 32 || d.thr16 == 0, NBEST_ERR_SHAPE, "embed_adv_delta: dropout counter overflow");
  hipStream_t st = (hipStream_t)stream;
  float* rowsq = (float*)ws;
  const int grid = grid_rows(M, 4);
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (embed_adv_grad_kernel<float, VPL><<<grid, 256, 0, st>>>(ids, seg, pos, key_mask, (const float*)word, (const float*)type,
                                                                             (const float*)ptab, gamma, (const float*)dout, delta, rowsq, M, H, eps, d)));
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (embed_adv_grad_kernel<bf16, VPL><<<grid, 256, 0, st>>>(ids, seg, pos, key_mask, (const bf16*)word, (const bf16*)type,
                                                                            (const bf16*)ptab, gamma, (const bf16*)dout, delta, rowsq, M, H, eps, d)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "embed_adv_delta: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  // blocks per utterance: enough that B x Y covers the chip a few times over, each with at least one float4 per thread
  const int64_t nv = (int64_t)S * (H >> 2);
  int Y = (int)((nv + 255) / 256);
  const int want = (2048 + B - 1) / B;
  if (Y > want) Y = want;
  if (Y < 1) Y = 1;
  NB_CHECK(B <= 65535, NBEST_ERR_SHAPE, "embed_adv_delta: B = %d exceeds the grid's y extent", B);
  embed_adv_scale_kernel<<<dim3(Y, B), 256, 0, st>>>(delta, rowsq, norm, S, H, epsilon);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_embed_attrib(const int64_t* ids, const int64_t* base_ids, const float* alpha, const int64_t* seg, const int64_t* pos,
                                  const void* word, const void* type, const void* ptab, const float* gamma, const void* dhidden,
                                  float* attr, int pairs, int m, int S, int H, float eps, int dtype, nbest_stream_t stream) {
  if (int e = check_h(H)) return e;
  NB_CHECK(ids && base_ids && alpha && pos && word && type && ptab && gamma && dhidden && attr, NBEST_ERR_ARG, "embed_attrib: null pointer");
  NB_CHECK(pairs > 0 && m > 0 && S > 0, NBEST_ERR_SHAPE, "embed_attrib: pairs=%d, m=%d, S=%d must be positive", pairs, m, S);
  NB_CHECK((int64_t)pairs * m <= INT32_MAX, NBEST_ERR_SHAPE, "embed_attrib: pairs x m = %lld sequences does not fit int32",
           (long long)pairs * m);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)pairs * S;
  const int grid = grid_rows(n, 4);
  if (dtype == NBEST_F32) {
    DISPATCH_VPL(H, (embed_attrib_kernel<float, VPL><<<grid, 256, 0, st>>>(ids, base_ids, alpha, seg, pos, (const float*)word, (const float*)type,
                                                                           (const float*)ptab, gamma, (const float*)dhidden, attr, n, m, S, H, eps)));
  } else if (dtype == NBEST_BF16) {
    DISPATCH_VPL(H, (embed_attrib_kernel<bf16, VPL><<<grid, 256, 0, st>>>(ids, base_ids, alpha, seg, pos, (const bf16*)word, (const bf16*)type,
                                                                          (const bf16*)ptab, gamma, (const bf16*)dhidden, attr, n, m, S, H, eps)));
  } else NB_CHECK(false, NBEST_ERR_DTYPE, "embed_attrib: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

// delta != NULL (nbest_embed_ln_bwd_adv): the ADV instantiations of the two token kernels, which recompute x_hat from the perturbed row
static int embed_ln_bwd_impl(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                             const void* type, const void* ptab, const float* gamma, const float* stats,
                             const void* dout, float* dword, float* dtype_tab, float* dptab, float* dgamma,
                             float* dbeta, int B, int S, int H, int n_types, int dtype, int64_t word_pad_id,
                             int64_t pos_pad_id, int accumulate, int tables_accumulate, float drop_p, uint64_t seed,
                             uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream, const float* delta) {
  if (int e = check_h(H)) return e;
  const int64_t M = (int64_t)B * S;
  NB_CHECK(ids && pos && word && type && ptab && gamma && stats && dout && dword && dtype_tab && dptab && dgamma && dbeta && ws && M > 0,
           NBEST_ERR_ARG, "embed_ln_bwd: null pointer");
  NB_CHECK(perm, NBEST_ERR_ARG, "embed_ln_bwd: perm (stable argsort of ids, int32 [B*S]) is required: the word-table gradient is a "
                                "segmented reduce over the sorted tokens, not a scatter of atomics");
  NB_CHECK(M < ((int64_t)1 << 31), NBEST_ERR_SHAPE, "embed_ln_bwd: B*S must fit int32 (perm)");
  NB_CHECK(ws_bytes >= nbest_embed_bwd_ws_bytes(M, H), NBEST_ERR_WORKSPACE, "embed_ln_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  // S x Y blocks (position, batch slice): as many as the partial-row workspace holds (kMaxLnBwdBlocks), at most one per sample
  int Y = kMaxLnBwdBlocks / S;
  if (Y > B) Y = B;
  if (Y < 1) Y = 1;
  NB_CHECK((int64_t)S * Y <= kMaxLnBwdBlocks, NBEST_ERR_SHAPE, "embed_ln_bwd: S = %d exceeds %d", S, kMaxLnBwdBlocks);
  float* part = (float*)ws;
  int64_t* colkey = (int64_t*)(part + (size_t)5 * kMaxLnBwdBlocks * H);
  int* mixed = (int*)(colkey + kMaxLnBwdBlocks);
  int* shared = mixed + kMaxLnBwdBlocks;
  float* wpart = (float*)(shared + kMaxLnBwdBlocks);              // 16-byte aligned: every region before it is a multiple of 16 bytes
  const size_t smem = (size_t)5 * H * sizeof(float);
  const dim3 grid(S, Y);
  const int64_t chunks = (M + kEmbTpc - 1) / kEmbTpc;
  const unsigned wgrid = (unsigned)((chunks + 3) / 4);
  int* fixlist = (int*)(wpart + (size_t)chunks * 2 * H);
#define NB_EMB_BWD2(TT, FULL, ADV)                                                                                              \
  DISPATCH_VPL(H, ((void)hipFuncSetAttribute((const void*)embed_bwd_pos_kernel<TT, VPL, FULL, ADV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), \
                   embed_bwd_pos_kernel<TT, VPL, FULL, ADV><<<grid, 256, smem, st>>>(ids, seg, pos, (const TT*)word, (const TT*)type, (const TT*)ptab, gamma, \
                                                                                 stats, (const TT*)dout, dtype_tab, dptab, part, fixlist, colkey, mixed, \
                                                                                 shared, B, S, H, pos_pad_id, d, delta), \
                   embed_bwd_word_kernel<TT, VPL, FULL, ADV><<<wgrid, 256, 0, st>>>(perm, ids, seg, pos, (const TT*)word, (const TT*)type, (const TT*)ptab, \
                                                                                gamma, stats, (const TT*)dout, dword, wpart, fixlist, M, H,  \
                                                                                kEmbTpc, word_pad_id, tables_accumulate, d, delta)))
#define NB_EMB_BWD(TT)                                                                  \
  do {                                                                                  \
    if (H % 256 == 0 && H <= 1024) { if (delta) NB_EMB_BWD2(TT, true, true); else NB_EMB_BWD2(TT, true, false); } \
    else { if (delta) NB_EMB_BWD2(TT, false, true); else NB_EMB_BWD2(TT, false, false); } \
  } while (0)
  embed_bwd_colkey_kernel<<<S, 256, 0, st>>>(seg, pos, B, S, H, pos_pad_id, tables_accumulate, colkey, mixed, dptab, dtype_tab);
  if (dtype == NBEST_F32) NB_EMB_BWD(float);
  else if (dtype == NBEST_BF16) NB_EMB_BWD(bf16);
  else NB_CHECK(false, NBEST_ERR_DTYPE, "embed_ln_bwd: bad dtype %d", dtype);
#undef NB_EMB_BWD2
#undef NB_EMB_BWD
  NB_LAUNCH_CHECK();
  embed_bwd_wordfix_kernel<<<(unsigned)(chunks < 2048 ? chunks : 2048), 256, (size_t)4 * H * sizeof(float), st>>>(perm, ids, wpart, fixlist, dword, M, H,
                                                                                                                    kEmbTpc, tables_accumulate);
  embed_bwd_finalize_kernel<<<dim3((H + 31) / 32, 4 + (S + 31) / 32), dim3(32, 32), 0, st>>>(part, colkey, shared, S, Y, H, n_types, pos_pad_id, dgamma, dbeta,
                                                                                             dtype_tab, dptab, accumulate, tables_accumulate);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_embed_ln_bwd(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                                  const void* type, const void* ptab, const float* gamma, const float* stats,
                                  const void* dout, float* dword, float* dtype_tab, float* dptab, float* dgamma,
                                  float* dbeta, int B, int S, int H, int n_types, int dtype, int64_t word_pad_id,
                                  int64_t pos_pad_id, int accumulate, int tables_accumulate, float drop_p, uint64_t seed,
                                  uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  return embed_ln_bwd_impl(ids, seg, pos, perm, word, type, ptab, gamma, stats, dout, dword, dtype_tab, dptab, dgamma, dbeta, B, S, H, n_types,
                           dtype, word_pad_id, pos_pad_id, accumulate, tables_accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream,
                           nullptr);
}

extern "C" int nbest_embed_ln_bwd_adv(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                                      const void* type, const void* ptab, const float* gamma, const float* stats, const float* delta,
                                      const void* dout, float* dword, float* dtype_tab, float* dptab, float* dgamma,
                                      float* dbeta, int B, int S, int H, int n_types, int dtype, int64_t word_pad_id,
                                      int64_t pos_pad_id, int accumulate, int tables_accumulate, float drop_p, uint64_t seed,
                                      uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(delta, NBEST_ERR_ARG, "embed_ln_bwd_adv: null delta (call nbest_embed_ln_bwd)");
  return embed_ln_bwd_impl(ids, seg, pos, perm, word, type, ptab, gamma, stats, dout, dword, dtype_tab, dptab, dgamma, dbeta, B, S, H, n_types,
                           dtype, word_pad_id, pos_pad_id, accumulate, tables_accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream,
                           delta);
}

extern "C" int nbest_rows_gather(const float* table, const int64_t* rows, int64_t n_rows, int64_t cap, int64_t* ids_out,
                                 float* vals_out, int H, nbest_stream_t stream) {
  NB_CHECK(table && ids_out && vals_out && (rows || n_rows == 0) && n_rows >= 0 && cap >= n_rows && H > 0 && H % 4 == 0, NBEST_ERR_ARG,
           "rows_gather: bad arguments");
  if (cap == 0) return NBEST_OK;
  rows_gather_kernel<<<(unsigned)cap, 256, 0, (hipStream_t)stream>>>(table, rows, n_rows, ids_out, vals_out, H);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_rows_zero(float* table, const int64_t* ids, int64_t n, int H, nbest_stream_t stream) {
  NB_CHECK(table && (ids || n == 0) && n >= 0 && H > 0 && H % 4 == 0, NBEST_ERR_ARG, "rows_zero: bad arguments");
  if (n == 0) return NBEST_OK;
  rows_update_kernel<<<(unsigned)n, 256, 0, (hipStream_t)stream>>>(table, ids, nullptr, H);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_rows_add(float* table, const int64_t* ids, const float* vals, int64_t n, int H, nbest_stream_t stream) {
  NB_CHECK(table && ((ids && vals) || n == 0) && n >= 0 && H > 0 && H % 4 == 0, NBEST_ERR_ARG, "rows_add: bad arguments");
  if (n == 0) return NBEST_OK;
  rows_update_kernel<<<(unsigned)n, 256, 0, (hipStream_t)stream>>>(table, ids, vals, H);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_cls_grad_scatter(const float* dcls, void* dhidden, int B, int S, int H, int dtype,
                                      nbest_stream_t stream) {
  if (int e = check_h(H)) return e;
  NB_CHECK(dcls && dhidden && B > 0 && S > 0, NBEST_ERR_ARG, "cls_grad_scatter: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nv = (int64_t)B * S * (H >> 2);
  int grid = (int)((nv + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (dtype == NBEST_F32) cls_scatter_kernel<float><<<grid, 256, 0, st>>>(dcls, (float*)dhidden, nv, S, H);
  else if (dtype == NBEST_BF16) cls_scatter_kernel<bf16><<<grid, 256, 0, st>>>(dcls, (bf16*)dhidden, nv, S, H);
  else NB_CHECK(false, NBEST_ERR_DTYPE, "cls_grad_scatter: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

// ---- the CLS rows of the top layer (nbest_encoder_desc::cls_top) ----------------------------------------------------------------
// y[r][c] = drop(x[r][c]) + R[r][c] over `rows` rows of N columns with row strides ldx, ldy, ldr (R == NULL: no residual).  The
// dropout decision of element (r, c) is the one the full-width kernels take for row r * row_mul of an [.][N] tensor - counter
// (r row_mul) N + c - so a compact [B][N] buffer of the CLS rows (row_mul = S) drops what the GEMM epilogue and the LayerNorm backward
// drop at rows b S.  drop_p == 0: a strided row copy (gather / scatter of the CLS rows).  One thread per element pair.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void rows_drop_res_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ R, int64_t ldr,
                                                            T* __restrict__ y, int64_t ldy, int64_t rows, int N, int64_t row_mul,
                                                            DropCfg drop) {
  const int half = N >> 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * half) return;
  const int64_t r = i / half;
  const int c = (int)(i - r * half) * 2;
  float v0 = (float)x[r * ldx + c], v1 = (float)x[r * ldx + c + 1];
  if (drop.thr16) {
    const uint32_t k = nb_keep2(drop, (uint32_t)(r * row_mul * N + c));
    v0 = (k & 1u) ? v0 * drop.scale : 0.f;
    v1 = (k & 2u) ? v1 * drop.scale : 0.f;
  }
  if (R) { v0 += (float)R[r * ldr + c]; v1 += (float)R[r * ldr + c + 1]; }
  y[r * ldy + c] = (T)v0;
  y[r * ldy + c + 1] = (T)v1;
}
}  // namespace

int nbest_internal_rows_drop_res(const void* x, int64_t ldx, const void* R, int64_t ldr, void* y, int64_t ldy, int64_t rows, int N,
                                 int64_t row_mul, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, hipStream_t st) {
  NB_CHECK(x && y && rows > 0 && N > 0 && N % 2 == 0 && ldx >= N && ldy >= N && (!R || ldr >= N), NBEST_ERR_ARG, "rows_drop_res: bad arguments");
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  NB_CHECK(d.thr16 == 0 || rows * row_mul * N < ((int64_t)1 << 32), NBEST_ERR_SHAPE, "rows_drop_res: dropout counter overflow");
  const int64_t n = rows * (N >> 1);
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (dtype == NBEST_F32)
    rows_drop_res_kernel<float><<<grid, 256, 0, st>>>((const float*)x, ldx, (const float*)R, ldr, (float*)y, ldy, rows, N, row_mul, d);
  else if (dtype == NBEST_BF16)
    rows_drop_res_kernel<bf16><<<grid, 256, 0, st>>>((const bf16*)x, ldx, (const bf16*)R, ldr, (bf16*)y, ldy, rows, N, row_mul, d);
  else NB_CHECK(false, NBEST_ERR_DTYPE, "rows_drop_res: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_cast_f32_to_bf16(const float* src, void* dst, int64_t n, nbest_stream_t stream) {
  NB_CHECK(src && dst && n >= 0, NBEST_ERR_ARG, "cast: bad arguments");
  if (n == 0) return NBEST_OK;
  int64_t g = ((n >> 3) + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  cast_bf16_kernel<<<(int)g, 256, 0, (hipStream_t)stream>>>(src, (bf16*)dst, n);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
