// K3r - one step of the CLS attention rollout (Abnar & Zuidema, 2020) from the forward's stash (nbest_attention_rollout_step):
//   r_out[b][j] = rho r_in[b][j] + (1 - rho) / heads * sum_h sum_i r_in[b][i] P[b][h][i][j]
//   P[b][h][i][j] = exp(scale q_i . k_j - lse[b][h][i]) on unmasked keys, exactly 0 on masked ones
// i.e. the row vector r_in pushed through rho I + (1 - rho) mean_h P_h.  No map is ever in memory: the probabilities are formed
// tile by tile the way nbest_attention_probs forms them (same operands, same expression, hence the same bits), weighted by
// r_in[query] and summed in registers.  Traffic: the Q and K thirds of qkv, lse, the key mask and two [B][S] vectors.
//   grid (B, ceil(S / 64)): one workgroup of NW = 4, 8 or 16 waves per (utterance, block of 64 keys).  The (head, query block)
//   items of the utterance are dealt to the waves as NW contiguous ranges; a wave keeps its running sums over all of its items in
//   registers, the NW partial rows [64] meet in LDS and are added in wave order by the threads that store the block's keys: every
//   r_out element is written once, by one thread, and nothing depends on the order anything ran in (no atomics: bit-reproducible).
//   A wave's items are one dependent chain each (loads -> 8 MFMAs -> 16 expf), so the waves are what hides the latency: NW is the
//   largest of 16 / 8 / 4 that leaves every wave 4 query blocks (fp32: 16 queries).  Measured, bf16 (profiles/rollout_bench.txt).
//   bf16: item = 16 queries.  Scores SWAPPED, S^T = K . Q^T on v_mfma_f32_16x16x32_bf16 (two k-steps over d = 64, fragments
//         fetched as 16-byte rows straight from qkv; the K fragments of the key block stay in registers while the head lasts), so
//         a lane holds 4 consecutive keys x 4 key tiles of ONE query (col = lane & 15): the weighted column sum is a multiply by
//         r_in[query], and the sum over the 16 query lanes - one DPP row - is taken once, after the last item.
//   fp32: item = 1 query (wave-uniform: its row is read through the scalar cache), lane = key, the key row in registers; each
//         score is one sequential fma chain over d, as attn_probs_f32_kernel.
// Exactness: a masked key's sum is exactly 0, so r_out = rho r_in there; at rho = 1 the weight (1 - rho) / heads is 0 and
// r_out = r_in bit for bit.  VEC: S % 4 == 0 and 16-byte aligned r_in / r_out (else one 4-byte load / store per element).
#include "common.h"

namespace {

// sum over the 16 lanes of a DPP row; every lane of the row gets it
__device__ __forceinline__ float row16_sum(float a) {
  a = dpp_add<0xB1>(a); a = dpp_add<0x4E>(a); a = dpp_add<0x141>(a); a = dpp_add<0x140>(a);
  return a;
}

// the waves' partial rows -> r_out for keys 64 kb .. 64 kb + 63 of utterance row `rin` / `rout`
template <int NW, bool VEC>
__device__ __forceinline__ void rollout_finish(const float (*part)[64], const float* __restrict__ rin, float* __restrict__ rout, int S,
                                               int kb, float rho, float w) {
  __syncthreads();
  const int tid = threadIdx.x, key = 64 * kb + 4 * tid;
  if (tid >= 16 || key >= S) return;
  f32x4 s = *(const f32x4*)&part[0][4 * tid];
#pragma unroll
  for (int wv = 1; wv < NW; ++wv) s += *(const f32x4*)&part[wv][4 * tid];
  if (VEC) {
    const f32x4 x = *(const f32x4*)(rin + key);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaf(w, s[e], rho * x[e]);
    *(f32x4*)(rout + key) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (key + e < S) rout[key + e] = fmaf(w, s[e], rho * rin[key + e]);
  }
}

template <int NW, bool VEC>
__global__ __launch_bounds__(64 * NW) void attn_rollout_bf16_kernel(const bf16* __restrict__ qkv, const uint8_t* __restrict__ mask,
                                                                const float* __restrict__ lse, const float* __restrict__ r_in,
                                                                float* __restrict__ r_out, int S, int heads, int H, float scale,
                                                                float rho, float w) {
  __shared__ __attribute__((aligned(16))) float part[NW][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, kb = blockIdx.y;
  const int64_t ld = 3 * (int64_t)H;
  const bf16* base = qkv + (int64_t)b * S * ld;
  const uint8_t* mk = mask + (int64_t)b * S;
  const float* rin = r_in + (int64_t)b * S;
  // bit 4 t + r: key 64 kb + 16 t + 4 g + r exists and is unmasked
  uint32_t keep = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = 64 * kb + 16 * t + 4 * g + r;
      if (key < S && mk[key]) keep |= 1u << (4 * t + r);
    }
  f32x4 sum[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) sum[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nq = (S + 15) / 16, total = heads * nq, per = (total + NW - 1) / NW;
  int i = wave * per;
  const int i1 = min(total, i + per);
  while (i < i1) {                              // (wave-uniform) the items of one head
    const int h = i / nq, qb0 = i - h * nq, qb1 = min(nq, qb0 + (i1 - i));
    bf16x8 kf[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = 64 * kb + 16 * t + c;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const i32x4 raw = (key < S) ? *(const i32x4*)(base + (int64_t)key * ld + H + h * 64 + 32 * ks + 8 * g) : i32x4{0, 0, 0, 0};
        kf[t][ks] = __builtin_bit_cast(bf16x8, raw);
      }
    }
    const float* lh = lse + ((int64_t)b * heads + h) * S;
    for (int qb = qb0; qb < qb1; ++qb) {
      const int qrow = 16 * qb + c;
      bf16x8 qf[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const i32x4 raw = (qrow < S) ? *(const i32x4*)(base + (int64_t)qrow * ld + h * 64 + 32 * ks + 8 * g) : i32x4{0, 0, 0, 0};
        qf[ks] = __builtin_bit_cast(bf16x8, raw);
      }
      const float lq = (qrow < S) ? lh[qrow] : 0.f;
      const float rq = (qrow < S) ? rin[qrow] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[ks], acc, 0, 0, 0);
        // acc[r] = q_(16 qb + c) . k_(64 kb + 16 t + 4 g + r)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = ((keep >> (4 * t + r)) & 1u) ? expf(acc[r] * scale - lq) : 0.f;
          sum[t][r] = fmaf(rq, p, sum[t][r]);
        }
      }
    }
    i += qb1 - qb0;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[t][r] = row16_sum(sum[t][r]);
    if (c == 0) *(f32x4*)&part[wave][16 * t + 4 * g] = sum[t];
  }
  rollout_finish<NW, VEC>(part, rin, r_out + (int64_t)b * S, S, kb, rho, w);
}

template <int NW, bool VEC>
__global__ __launch_bounds__(64 * NW) void attn_rollout_f32_kernel(const float* __restrict__ qkv, const uint8_t* __restrict__ mask,
                                                               const float* __restrict__ lse, const float* __restrict__ r_in,
                                                               float* __restrict__ r_out, int S, int heads, int H, float scale,
                                                               float rho, float w) {
  __shared__ __attribute__((aligned(16))) float part[NW][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, kb = blockIdx.y;
  const int64_t ld = 3 * (int64_t)H;
  const float* base = qkv + (int64_t)b * S * ld;
  const float* rin = r_in + (int64_t)b * S;
  const int key = 64 * kb + lane;
  const bool valid = key < S && mask[(int64_t)b * S + key];
  float sum = 0.f;
  const int total = heads * S, per = (total + NW - 1) / NW;
  int i = wave * per;
  const int i1 = min(total, i + per);
  while (i < i1) {                              // (wave-uniform) the queries of one head
    const int h = i / S, q0 = i - h * S, q1 = min(S, q0 + (i1 - i));
    float k[64];
    const float* kp = base + (int64_t)(valid ? key : 0) * ld + H + h * 64;
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
      const f32x4 x = *(const f32x4*)(kp + d);
      k[d] = x[0]; k[d + 1] = x[1]; k[d + 2] = x[2]; k[d + 3] = x[3];
    }
    const float* lh = lse + ((int64_t)b * heads + h) * S;
    for (int qi = q0; qi < q1; ++qi) {
      const float* qp = base + (int64_t)qi * ld + h * 64;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 64; ++d) s = fmaf(qp[d], k[d], s);
      const float p = valid ? expf(s * scale - lh[qi]) : 0.f;
      sum = fmaf(rin[qi], p, sum);
    }
    i += q1 - q0;
  }
  part[wave][lane] = sum;
  rollout_finish<NW, VEC>(part, rin, r_out + (int64_t)b * S, S, kb, rho, w);
}

}  // namespace

extern "C" int nbest_attention_rollout_step(const void* qkv, const uint8_t* key_mask, const float* lse, const float* r_in, float* r_out,
                                            float residual, int B, int S, int heads, int d, int dtype, nbest_stream_t stream) {
  NB_CHECK(qkv && key_mask && lse && r_in && r_out, NBEST_ERR_ARG, "attention_rollout_step: null pointer");
  NB_CHECK(r_in != r_out, NBEST_ERR_ARG, "attention_rollout_step: r_in and r_out must be different buffers");
  NB_CHECK(residual >= 0.f && residual <= 1.f, NBEST_ERR_ARG, "attention_rollout_step: residual %g outside [0, 1]", (double)residual);
  NB_CHECK(B > 0 && heads > 0, NBEST_ERR_SHAPE, "attention_rollout_step: bad shape");
  NB_CHECK(d == 64, NBEST_ERR_SHAPE, "attention_rollout_step: head dimension %d not supported (64 only)", d);
  NB_CHECK(S >= 1 && S <= 512, NBEST_ERR_SHAPE, "attention_rollout_step: S=%d outside 1..512", S);
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "attention_rollout_step: bad dtype %d", dtype);
  NB_CHECK(((uintptr_t)qkv & 15) == 0, NBEST_ERR_ALIGN, "attention_rollout_step: qkv must be 16-byte aligned");
  NB_CHECK(((uintptr_t)lse & 3) == 0 && ((uintptr_t)r_in & 3) == 0 && ((uintptr_t)r_out & 3) == 0, NBEST_ERR_ALIGN,
           "attention_rollout_step: lse, r_in and r_out must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int H = heads * d;
  const float scale = 1.0f / sqrtf((float)d);
  const float w = (1.0f - residual) / (float)heads;
  const bool vec = (S % 4) == 0 && (((uintptr_t)r_in | (uintptr_t)r_out) & 15) == 0;
  const dim3 grid(B, (S + 63) / 64);
  // waves per workgroup: 16, 8 or 4 - the most that leaves every wave min_items items (a function of the shape alone, so the
  // order of the sums is too)
  const bool f32 = dtype == NBEST_F32;
  const int items = f32 ? heads * S : heads * ((S + 15) / 16), min_items = f32 ? 16 : 4;
  const int nw = items >= 16 * min_items ? 16 : (items >= 8 * min_items ? 8 : 4);
#define ROLL(KERNEL, T, NW)                                                                                                             \
  do {                                                                                                                                  \
    if (vec) KERNEL<NW, true><<<grid, 64 * NW, 0, st>>>((const T*)qkv, key_mask, lse, r_in, r_out, S, heads, H, scale, residual, w);  \
    else KERNEL<NW, false><<<grid, 64 * NW, 0, st>>>((const T*)qkv, key_mask, lse, r_in, r_out, S, heads, H, scale, residual, w);     \
  } while (0)
  if (f32) {
    if (nw == 16) ROLL(attn_rollout_f32_kernel, float, 16);
    else if (nw == 8) ROLL(attn_rollout_f32_kernel, float, 8);
    else ROLL(attn_rollout_f32_kernel, float, 4);
  } else {
    if (nw == 16) ROLL(attn_rollout_bf16_kernel, bf16, 16);
    else if (nw == 8) ROLL(attn_rollout_bf16_kernel, bf16, 8);
    else ROLL(attn_rollout_bf16_kernel, bf16, 4);
  }
#undef ROLL
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
