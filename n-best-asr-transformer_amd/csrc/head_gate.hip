// Head gates (HF's head_mask; Michel et al., 2019): a per-head factor xi[h] on the attention context between the attention kernel
// and the attention-output GEMM, and its gradient.  Two memory-bound kernels of their own: the tuned attention kernels are not
// touched (several sit at their register / LDS limits).  d = 64, fp32 and bf16, 16-byte accesses, no atomics, bit-reproducible.
//   forward:  out[m][h d + k] = T(gate[h] * float(in[m][h d + k]))                     1 read + 1 write of [M][H]
//   backward: dgate[b][h] = sum_{s,k} ctx[b,s,h,k] * dctx[b,s,h,k]  (fp32, fixed order), then dctx <- T(gate[h] * dctx) in place
//             2 reads + 1 write of [M][H]; the write is skipped for gate[h] == 1
#include "common.h"

namespace {

constexpr int kGateThreads = 256;

// one thread per 16-byte vector (N elements) of the [M][heads * 64] rows; a vector never straddles a head (64 % N == 0)
template <typename T, int N>
__global__ __launch_bounds__(kGateThreads) void head_gate_fwd_kernel(const T* in, int64_t ld_in, T* out, int64_t ld_out,
                                                                     const float* __restrict__ gate, int64_t M, int heads) {
  constexpr int VPH = 64 / N;                                 // vectors per head
  const int vpr = heads * VPH;                                // vectors per row
  const int64_t total = M * vpr;
  for (int64_t v = (int64_t)blockIdx.x * kGateThreads + threadIdx.x; v < total; v += (int64_t)gridDim.x * kGateThreads) {
    const int64_t m = v / vpr;
    const int c = (int)(v - m * vpr);
    const float g = gate[c / VPH];
    const T* src = in + m * ld_in + (int64_t)c * N;
    T* dst = out + m * ld_out + (int64_t)c * N;               // (in place: every thread reads its vector before it writes it)
    if constexpr (N == 8) {
      float x[8];
      Vec8<T>::load(src, x);
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] *= g;
      Vec8<T>::store(dst, x);
    } else {
      const f32x4 x = Vec4<T>::load(src);
      Vec4<T>::store(dst, f32x4{x[0] * g, x[1] * g, x[2] * g, x[3] * g});
    }
  }
}

// One workgroup per (utterance b, head h): its S rows of 64 elements.  Thread t owns vector t % VPH of the rows t / VPH,
// t / VPH + RPP, ..: a fixed set of elements, summed in ascending row order with one fma per element, then the wave's
// xor-shuffle tree and the four wave totals in wave order - the same additions in the same order in every run.
template <typename T, int N>
__global__ __launch_bounds__(kGateThreads) void head_gate_bwd_kernel(const T* __restrict__ ctx, T* dctx, const float* __restrict__ gate,
                                                                     float* __restrict__ dgate, int S, int heads) {
  constexpr int VPH = 64 / N, RPP = kGateThreads / VPH;      // vectors per head row, rows per pass
  __shared__ float red[16];
  const int h = blockIdx.x, b = blockIdx.y;
  const int H = heads * 64;
  const float g = gate[h];
  const bool scale = g != 1.0f;                               // an all-ones gate leaves dctx bit-identical: no store at all
  if (!dgate && !scale) return;                               // nothing to sum, nothing to store (uniform over the block, before any barrier)
  const int r0 = threadIdx.x / VPH, vc = (threadIdx.x % VPH) * N;
  const int64_t base = (int64_t)b * S * H + (int64_t)h * 64 + vc;
  float acc = 0.f;
  for (int s = r0; s < S; s += RPP) {
    const int64_t off = base + (int64_t)s * H;
    float dv[N];
    if constexpr (N == 8) Vec8<T>::load(dctx + off, dv);
    else { const f32x4 t = Vec4<T>::load(dctx + off); dv[0] = t[0]; dv[1] = t[1]; dv[2] = t[2]; dv[3] = t[3]; }
    if (dgate) {
      float cv[N];
      if constexpr (N == 8) Vec8<T>::load(ctx + off, cv);
      else { const f32x4 t = Vec4<T>::load(ctx + off); cv[0] = t[0]; cv[1] = t[1]; cv[2] = t[2]; cv[3] = t[3]; }
#pragma unroll
      for (int i = 0; i < N; ++i) acc = fmaf(cv[i], dv[i], acc);
    }
    if (scale) {
#pragma unroll
      for (int i = 0; i < N; ++i) dv[i] *= g;
      if constexpr (N == 8) Vec8<T>::store(dctx + off, dv);
      else Vec4<T>::store(dctx + off, f32x4{dv[0], dv[1], dv[2], dv[3]});
    }
  }
  if (dgate) {                                                // (uniform over the grid: every thread reaches the barriers)
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) dgate[(int64_t)b * heads + h] = tot;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int nbest_head_gate_fwd(const void* ctx_in, int64_t ld_in, void* ctx_out, int64_t ld_out, const float* gate, int64_t M,
                                   int heads, int d, int dtype, nbest_stream_t stream) {
  NB_CHECK(ctx_in && ctx_out && gate, NBEST_ERR_ARG, "head_gate_fwd: null pointer");
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "head_gate_fwd: bad dtype %d", dtype);
  NB_CHECK(d == 64 && heads > 0 && M > 0, NBEST_ERR_SHAPE, "head_gate_fwd: needs d == 64 (got %d), heads > 0, M > 0", d);
  const int64_t H = (int64_t)heads * 64;
  const int n = dtype == NBEST_BF16 ? 8 : 4;
  NB_CHECK(ld_in >= H && ld_out >= H && ld_in % n == 0 && ld_out % n == 0, NBEST_ERR_SHAPE,
           "head_gate_fwd: ld_in %lld / ld_out %lld must be >= H = %lld and multiples of %d elements", (long long)ld_in, (long long)ld_out,
           (long long)H, n);
  NB_CHECK(aligned16(ctx_in) && aligned16(ctx_out), NBEST_ERR_ALIGN, "head_gate_fwd: ctx_in / ctx_out must be 16-byte aligned");
  const int64_t vecs = M * (H / n);
  const int64_t blocks = (vecs + kGateThreads - 1) / kGateThreads;
  const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == NBEST_BF16)
    hipLaunchKernelGGL((head_gate_fwd_kernel<bf16, 8>), grid, dim3(kGateThreads), 0, st, (const bf16*)ctx_in, ld_in, (bf16*)ctx_out, ld_out, gate, M, heads);
  else
    hipLaunchKernelGGL((head_gate_fwd_kernel<float, 4>), grid, dim3(kGateThreads), 0, st, (const float*)ctx_in, ld_in, (float*)ctx_out, ld_out, gate, M, heads);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_head_gate_bwd(const void* ctx, void* dctx, const float* gate, float* dgate, int B, int S, int heads, int d, int dtype,
                                   nbest_stream_t stream) {
  NB_CHECK(dctx && gate && (ctx || !dgate), NBEST_ERR_ARG, "head_gate_bwd: null pointer (ctx may be NULL only without dgate)");
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "head_gate_bwd: bad dtype %d", dtype);
  NB_CHECK(d == 64 && heads > 0 && B > 0 && S > 0 && B <= 65535, NBEST_ERR_SHAPE,
           "head_gate_bwd: needs d == 64 (got %d), heads > 0, S > 0, 0 < B <= 65535 (got %d)", d, B);
  NB_CHECK(aligned16(dctx) && aligned16(ctx), NBEST_ERR_ALIGN, "head_gate_bwd: ctx / dctx must be 16-byte aligned");
  const dim3 grid((unsigned)heads, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == NBEST_BF16)
    hipLaunchKernelGGL((head_gate_bwd_kernel<bf16, 8>), grid, dim3(kGateThreads), 0, st, (const bf16*)ctx, (bf16*)dctx, gate, dgate, S, heads);
  else
    hipLaunchKernelGGL((head_gate_bwd_kernel<float, 4>), grid, dim3(kGateThreads), 0, st, (const float*)ctx, (float*)dctx, gate, dgate, S, heads);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
