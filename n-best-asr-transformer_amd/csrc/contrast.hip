// K8c  in-batch contrastive loss between the ASR and the transcript CLS rows (--contrastive_weight): include/nbest_hip.h.
//
// Four launches on the caller's stream, each reading only what an earlier launch wrote (no atomics, no workgroup waits for another):
//   1 contrast_unit_kernel   2 B blocks   a row of either pass -> its fp32 unit vector (zero-padded to a multiple of 4) and its norm
//   2 contrast_sim_kernel      B blocks   Z[i][:] = <u_i, v_j> / T, formed ONCE: the row and the column softmax read the same bits
//   3 contrast_lse_kernel    2 B blocks   lr_i (rows) / lc_j (columns) by max-subtracted log-sum-exp; the rows also record their hit
//   4 contrast_grad_kernel   2 B + 1      du_i / dv_j, projected onto the tangent of the unit sphere; the last block sums the loss
// Everything is fp32 on the vector units.  The unit vectors are NOT rounded to bf16 and the bf16 MFMA is not used: a cosine near 1 has
// a bf16 ulp of 2^-8, and at T = 0.05 that is 0.08 in a logit - the size of the differences the softmax is there to resolve.
// All sums run in a fixed order (strided per thread, xor butterfly per wave, waves 0..3 in turn), so two calls give the same bits.
#include "common.h"

namespace {
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxB = 4096, kMaxH = 8192;

// the fp32 regions of the workspace, in floats; every region starts on 16 bytes and is fully written before it is read
struct ContrastWs {
  int64_t Hp, U, V, na, nt, lr, lc, hit, Z, floats;
  ContrastWs(int B, int H) {
    Hp = round_up(H, 4);
    const int64_t Bp = round_up(B, 4);
    U = 0; V = U + B * Hp; na = V + B * Hp; nt = na + Bp; lr = nt + Bp; lc = lr + Bp; hit = lc + Bp; Z = hit + Bp;
    floats = Z + (int64_t)B * B;
  }
};

// block-wide (max, first index of the max); smem needs >= 2 * kWaves words.  All threads get the result.
__device__ __forceinline__ void block_argmax(float& m, int& am, float* smem) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const int a2 = __shfl_xor(am, o, 64);
    if (m2 > m || (m2 == m && a2 < am)) { m = m2; am = a2; }
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { smem[w] = m; ((int*)smem)[kWaves + w] = am; }
  __syncthreads();
  m = smem[0]; am = ((int*)smem)[kWaves];
  for (int i = 1; i < kWaves; ++i) {
    const float m2 = smem[i];
    const int a2 = ((int*)smem)[kWaves + i];
    if (m2 > m || (m2 == m && a2 < am)) { m = m2; am = a2; }
  }
}

// block r < B: ASR row r; block r >= B: transcript row r - B.  unit = x / max(||x||, 1e-12) (torch's F.normalize), norm = the clamped one.
template <typename T>
__global__ __launch_bounds__(kThreads) void contrast_unit_kernel(const T* __restrict__ ha, int64_t sa, const T* __restrict__ ht, int64_t st_,
                                                                 int B, int H, int Hp, float* __restrict__ U, float* __restrict__ V,
                                                                 float* __restrict__ na, float* __restrict__ nt) {
  __shared__ float sm[16];
  const bool tr = (int)blockIdx.x >= B;
  const int i = tr ? blockIdx.x - B : blockIdx.x;
  const T* x = tr ? ht + (int64_t)i * st_ : ha + (int64_t)i * sa;
  float* o = (tr ? V : U) + (int64_t)i * Hp;
  float s = 0.f;
  for (int h = threadIdx.x; h < H; h += kThreads) {
    const float v = to_f<T>(x[h]);
    s = fmaf(v, v, s);
  }
  const float n = fmaxf(sqrtf(block_sum(s, sm)), 1e-12f);
  for (int h = threadIdx.x; h < Hp; h += kThreads) o[h] = h < H ? to_f<T>(x[h]) / n : 0.f;
  if (threadIdx.x == 0) (tr ? nt : na)[i] = n;
}

// block i: u_i in LDS; a wave takes four columns at a time (four independent 16-byte loads per lane and step), lanes over h
__global__ __launch_bounds__(kThreads) void contrast_sim_kernel(const float* __restrict__ U, const float* __restrict__ V, int B, int Hp,
                                                                float temperature, float* __restrict__ Z) {
  extern __shared__ __attribute__((aligned(16))) float us[];  // [Hp]
  const int i = blockIdx.x, nv = Hp >> 2;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const f32x4* u4 = (const f32x4*)(U + (int64_t)i * Hp);
  const f32x4* V4 = (const f32x4*)V;
  f32x4* us4 = (f32x4*)us;
  for (int c = threadIdx.x; c < nv; c += kThreads) us4[c] = u4[c];
  __syncthreads();
  for (int j0 = wave * 4; j0 < B; j0 += kWaves * 4) {
    int64_t row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = (int64_t)min(j0 + q, B - 1) * nv;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < nv; c += 64) {
      const f32x4 u = us4[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = V4[row[q] + c];
        s[q] = fmaf(u[3], v[3], fmaf(u[2], v[2], fmaf(u[1], v[1], fmaf(u[0], v[0], s[q]))));
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float t = wave_sum(s[q]);
      if (lane == 0 && j0 + q < B) Z[(int64_t)i * B + j0 + q] = t / temperature;
    }
  }
}

// keep(i, j) = (i == j) or (k_i != k_j); without keys every pair is kept
__device__ __forceinline__ bool contrast_keep(const int64_t* key, int64_t ki, int i, int j) { return i == j || !key || key[j] != ki; }

// block r < B: lr_r over the kept columns of row r, and whether the row's first maximum is its own column;
// block r >= B: lc_(r - B) over the kept rows of that column.  The diagonal is always kept, so the maximum is finite.
__global__ __launch_bounds__(kThreads) void contrast_lse_kernel(const float* __restrict__ Z, const int64_t* __restrict__ key, int B,
                                                                float* __restrict__ lr, float* __restrict__ lc, float* __restrict__ hit) {
  __shared__ float zs[kMaxB];
  __shared__ float sm[16];
  const bool col = (int)blockIdx.x >= B;
  const int i = col ? blockIdx.x - B : blockIdx.x;
  const float* base = col ? Z + i : Z + (int64_t)i * B;
  const int64_t stride = col ? B : 1, ki = key ? key[i] : 0;
  float m = -INFINITY;
  int am = 0x7fffffff;
  for (int j = threadIdx.x; j < B; j += kThreads) {
    const float z = contrast_keep(key, ki, i, j) ? base[j * stride] : -INFINITY;
    zs[j] = z;
    if (z > m) { m = z; am = j; }   // j ascends: the first maximum of this thread's columns
  }
  block_argmax(m, am, sm);
  float s = 0.f;
  for (int j = threadIdx.x; j < B; j += kThreads) s += expf(zs[j] - m);   // a dropped pair: exp(-inf) = 0
  s = block_sum(s, sm);
  if (threadIdx.x == 0) {
    (col ? lc : lr)[i] = m + logf(s);   // one kept pair: m + log(1) = Z_ii exactly
    if (!col) hit[i] = am == i ? 1.f : 0.f;
  }
}

// block r < B: da_r += proj(du_r), du_r = sum_j G_rj v_j;  block B <= r < 2 B: dt_j (+)= proj(dv_j), dv_j = sum_i G_ij u_i, j = r - B;
// block n_grad (the last one): out[0..3].  proj(d) = (d - <d, own> own) / ||row||: the backward of x / ||x||.
// G_ij = scale [ keep (exp(Z_ij - lr_i) + exp(Z_ij - lc_j)) - 2 [i == j] ], scale = W / 2T.
__global__ __launch_bounds__(kThreads) void contrast_grad_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                                 const float* __restrict__ na, const float* __restrict__ nt,
                                                                 const float* __restrict__ Z, const float* __restrict__ lr,
                                                                 const float* __restrict__ lc, const float* __restrict__ hit,
                                                                 const int64_t* __restrict__ key, int B, int H, int Hp, float scale,
                                                                 float* __restrict__ da, float* __restrict__ dt, int accumulate_dt,
                                                                 int n_grad, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // red [kThreads][4] | sm [16] | d [Hp] | g [B]
  float* sm = lds + kThreads * 4;
  if ((int)blockIdx.x == n_grad) {
    float s = 0.f, h = 0.f;
    for (int i = threadIdx.x; i < B; i += kThreads) {
      const float zii = Z[(int64_t)i * B + i];
      s += (lr[i] - zii) + (lc[i] - zii);
      h += hit[i];
    }
    s = block_sum(s, sm);
    h = block_sum(h, sm);
    if (threadIdx.x == 0) { out[0] = 0.5f * s; out[1] = h; out[2] = (float)B; out[3] = 0.f; }
    return;
  }
  const bool col = (int)blockIdx.x >= B;
  const int i = col ? blockIdx.x - B : blockIdx.x;
  float* dst = col ? dt : da;
  if (!dst) return;   // block-uniform
  f32x4* red = (f32x4*)lds;
  float* d = sm + 16;
  float* g = d + Hp;
  const int nv = Hp >> 2, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* own = (col ? V : U) + (int64_t)i * Hp;
  const f32x4* X4 = (const f32x4*)(col ? U : V);   // the rows the sum runs over
  const float lse_own = col ? lc[i] : lr[i];
  const float* lse_other = col ? lr : lc;
  const int64_t ki = key ? key[i] : 0;
  for (int j = threadIdx.x; j < B; j += kThreads) {
    const float z = col ? Z[(int64_t)j * B + i] : Z[(int64_t)i * B + j];
    const float e = contrast_keep(key, ki, i, j) ? expf(z - lse_own) + expf(z - lse_other[j]) : 0.f;
    g[j] = scale * (e - (j == i ? 2.f : 0.f));
  }
  __syncthreads();
  for (int c0 = 0; c0 < nv; c0 += 64) {   // 256 columns at a time: a wave takes every fourth row, a lane four columns
    const int c = c0 + lane;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c < nv) {
#pragma unroll 8
      for (int j = wave; j < B; j += kWaves) acc += g[j] * X4[(int64_t)j * nv + c];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (wave == 0 && c < nv) ((f32x4*)d)[c] = (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
    __syncthreads();
  }
  float dot = 0.f;
  for (int h = threadIdx.x; h < H; h += kThreads) dot = fmaf(d[h], own[h], dot);
  dot = block_sum(dot, sm);
  const float n = (col ? nt : na)[i];
  float* o = dst + (int64_t)i * H;
  const bool add = !col || accumulate_dt;
  for (int h = threadIdx.x; h < H; h += kThreads) {
    const float v = (d[h] - dot * own[h]) / n;
    o[h] = add ? o[h] + v : v;
  }
}
}  // namespace

extern "C" size_t nbest_cls_contrast_ws_bytes(int B, int H) {
  if (B <= 0 || H <= 0) return 0;
  return (size_t)ContrastWs(B, H).floats * sizeof(float);
}

extern "C" int nbest_cls_contrast(const void* hidden_a, int64_t stride_a, const void* hidden_t, int64_t stride_t, const int64_t* key,
                                  float weight, float temperature, float* out, float* da, float* dt, int accumulate_dt, int B, int H,
                                  int dtype, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(hidden_a && hidden_t && out && ws, NBEST_ERR_ARG, "cls_contrast: null pointer");
  NB_CHECK(B > 0 && H > 0 && B <= kMaxB, NBEST_ERR_ARG, "cls_contrast: B = %d, H = %d (0 < B <= %d, H > 0)", B, H, kMaxB);
  NB_CHECK(temperature > 0.f && temperature < INFINITY, NBEST_ERR_ARG, "cls_contrast: temperature %g must be finite and > 0",
           (double)temperature);
  NB_CHECK(weight >= 0.f && weight < INFINITY, NBEST_ERR_ARG, "cls_contrast: weight %g must be finite and >= 0", (double)weight);
  NB_CHECK(((uintptr_t)ws & 15) == 0, NBEST_ERR_ARG, "cls_contrast: workspace not aligned to 16 bytes");
  NB_CHECK(H <= kMaxH, NBEST_ERR_SHAPE, "cls_contrast: H = %d exceeds %d", H, kMaxH);
  const ContrastWs w(B, H);
  NB_CHECK(ws_bytes >= (size_t)w.floats * sizeof(float), NBEST_ERR_WORKSPACE, "cls_contrast: workspace too small");
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "cls_contrast: bad dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  float* f = (float*)ws;
  float *U = f + w.U, *V = f + w.V, *na = f + w.na, *nt = f + w.nt, *lr = f + w.lr, *lc = f + w.lc, *hit = f + w.hit, *Z = f + w.Z;
  const int Hp = (int)w.Hp;
  if (dtype == NBEST_F32)
    contrast_unit_kernel<float><<<2 * B, kThreads, 0, st>>>((const float*)hidden_a, stride_a, (const float*)hidden_t, stride_t, B, H, Hp, U, V, na, nt);
  else
    contrast_unit_kernel<bf16><<<2 * B, kThreads, 0, st>>>((const bf16*)hidden_a, stride_a, (const bf16*)hidden_t, stride_t, B, H, Hp, U, V, na, nt);
  NB_LAUNCH_CHECK();
  contrast_sim_kernel<<<B, kThreads, (size_t)Hp * sizeof(float), st>>>(U, V, B, Hp, temperature, Z);
  NB_LAUNCH_CHECK();
  contrast_lse_kernel<<<2 * B, kThreads, 0, st>>>(Z, key, B, lr, lc, hit);
  NB_LAUNCH_CHECK();
  // loss only: the one block that sums it
  const int n_grad = (da || dt) ? 2 * B : 0;
  const size_t smem = ((size_t)kThreads * 4 + 16 + Hp + B) * sizeof(float);
  contrast_grad_kernel<<<n_grad + 1, kThreads, smem, st>>>(U, V, na, nt, Z, lr, lc, hit, key, B, H, Hp, weight / (2.f * temperature), da,
                                                          dt, accumulate_dt, n_grad, out);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
