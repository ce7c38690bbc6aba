// K9s sharpness-aware minimization (--sam_rho; Foret et al. 2021, adaptive: Kwon et al. 2021) over the flat fp32 arenas and the
// descriptor tables of K9: the weight-space half of the step.  w -> w + e before the second forward / backward, w back afterwards.
//
// HBM-bound streaming kernels in the pattern of K9e (optim.hip): the block -> (tensor, chunk) map is a binary search over
// desc.block_start, one workgroup of 256 threads per chunk of nbest_bertadam_chunk() elements, float4 path when the tensor's offset
// is a multiple of 4 and a scalar tail, no LDS beyond the norm stage's block sum, no atomics: bit-reproducible.  Inactive tensors
// and the elements between tensors are never read or written.
#include "common.h"

namespace {

constexpr int kChunk = 16384;  // == nbest_bertadam_chunk() (checked by every entry point): the descriptors' block_start counts these

__device__ __forceinline__ int find_tensor(const nbest_tensor_desc* __restrict__ d, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].block_start <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// (t g)^2, t = |p| + eta: the element of the adaptive norm ||T_w g||, T_w = diag(|w| + eta)
__device__ __forceinline__ float asam_sq(float p, float g, float eta) {
  const float x = (fabsf(p) + eta) * g;
  return x * x;
}

// the summation shape of optim.hip's sumsq_kernel: a tree of depth 2 per float4, a running sum per thread, block_sum
__global__ __launch_bounds__(256) void sam_norms_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                        const nbest_tensor_desc* __restrict__ descs, int n_tensors, float eta,
                                                        float* __restrict__ partial) {
  __shared__ float sm[16];
  const int blk = blockIdx.x;
  const int t = find_tensor(descs, n_tensors, blk);
  const nbest_tensor_desc d = descs[t];
  float s = 0.f;
  if (d.active) {
    const int64_t c0 = (int64_t)(blk - d.block_start) * kChunk;
    const int64_t c1 = (c0 + kChunk < d.numel) ? c0 + kChunk : d.numel;
    const float* pp = p + d.offset;
    const float* gp = g + d.offset;
    if ((d.offset & 3) == 0) {
      const int64_t v1 = c0 + ((c1 - c0) & ~(int64_t)3);
      for (int64_t i = c0 + 4 * threadIdx.x; i < v1; i += 1024) {
        const f32x4 w = *(const f32x4*)(pp + i), x = *(const f32x4*)(gp + i);
        s += (asam_sq(w[0], x[0], eta) + asam_sq(w[1], x[1], eta)) + (asam_sq(w[2], x[2], eta) + asam_sq(w[3], x[3], eta));
      }
      for (int64_t i = v1 + threadIdx.x; i < c1; i += 256) s += asam_sq(pp[i], gp[i], eta);
    } else {
      for (int64_t i = c0 + threadIdx.x; i < c1; i += 256) s += asam_sq(pp[i], gp[i], eta);
    }
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) partial[blk] = s;
}

// p + e as ONE explicit fma (no contraction choice left to the compiler), as optim.hip's ema1.  plain: e = s g; adaptive:
// e = s t^2 g, t = |p| + eta (three roundings before the fma)
template <bool ADAPTIVE>
__device__ __forceinline__ float perturb1(float p, float g, float s, float eta) {
  if (ADAPTIVE) {
    const float t = fabsf(p) + eta;
    return fmaf(s, (t * t) * g, p);
  }
  return fmaf(s, g, p);
}

// MODE 0: s == 0 (rho == 0, or the norm is 0 or not finite) - backup and the bf16 copy are written, g is not touched (it may hold
// inf / NaN) and p keeps its bits; 1: plain; 2: adaptive.  The mode is uniform over the launch: every thread reads the same norm.
template <int MODE>
__device__ __forceinline__ void perturb_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                              bf16* __restrict__ plow, int64_t base, int64_t c0, int64_t c1, float s, float eta) {
  int64_t v1 = c0;
  if ((base & 3) == 0) {
    v1 = c0 + ((c1 - c0) & ~(int64_t)3);
    for (int64_t i = c0 + 4 * threadIdx.x; i < v1; i += 1024) {
      f32x4 pp = *(const f32x4*)(p + base + i);
      *(f32x4*)(backup + base + i) = pp;
      if (MODE != 0) {
        const f32x4 gg = *(const f32x4*)(g + base + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = perturb1<MODE == 2>(pp[e], gg[e], s, eta);
        *(f32x4*)(p + base + i) = pp;
      }
      if (plow) Vec4<bf16>::store(plow + base + i, pp);
    }
  }
  for (int64_t i = v1 + threadIdx.x; i < c1; i += 256) {
    float pp = p[base + i];
    backup[base + i] = pp;
    if (MODE != 0) {
      pp = perturb1<MODE == 2>(pp, g[base + i], s, eta);
      p[base + i] = pp;
    }
    if (plow) plow[base + i] = (bf16)pp;
  }
}

__global__ __launch_bounds__(256) void sam_perturb_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                                          bf16* __restrict__ plow, const nbest_tensor_desc* __restrict__ descs,
                                                          int n_tensors, const float* __restrict__ norm, float rho, float eta) {
  const int blk = blockIdx.x;
  const int t = find_tensor(descs, n_tensors, blk);
  const nbest_tensor_desc d = descs[t];
  if (!d.active) return;
  const float nrm = norm[0];
  const bool moves = rho > 0.f && nrm > 0.f && isfinite(nrm);
  const float s = moves ? rho / (nrm + 1e-12f) : 0.f;
  const int64_t c0 = (int64_t)(blk - d.block_start) * kChunk;
  const int64_t c1 = (c0 + kChunk < d.numel) ? c0 + kChunk : d.numel;
  if (!moves) perturb_chunk<0>(p, g, backup, plow, d.offset, c0, c1, 0.f, eta);
  else if (eta < 0.f) perturb_chunk<1>(p, g, backup, plow, d.offset, c0, c1, s, eta);
  else perturb_chunk<2>(p, g, backup, plow, d.offset, c0, c1, s, eta);
}

// p = backup, plow = its bf16 (the conversion of the optimizer kernels' compute copy): a pure move
__global__ __launch_bounds__(256) void sam_restore_kernel(float* __restrict__ p, const float* __restrict__ backup, bf16* __restrict__ plow,
                                                          const nbest_tensor_desc* __restrict__ descs, int n_tensors) {
  const int blk = blockIdx.x;
  const int t = find_tensor(descs, n_tensors, blk);
  const nbest_tensor_desc d = descs[t];
  if (!d.active) return;
  const int64_t c0 = (int64_t)(blk - d.block_start) * kChunk;
  const int64_t c1 = (c0 + kChunk < d.numel) ? c0 + kChunk : d.numel;
  const int64_t base = d.offset;
  int64_t v1 = c0;
  if ((base & 3) == 0) {
    v1 = c0 + ((c1 - c0) & ~(int64_t)3);
    for (int64_t i = c0 + 4 * threadIdx.x; i < v1; i += 1024) {
      const f32x4 bb = *(const f32x4*)(backup + base + i);
      *(f32x4*)(p + base + i) = bb;
      if (plow) Vec4<bf16>::store(plow + base + i, bb);
    }
  }
  for (int64_t i = v1 + threadIdx.x; i < c1; i += 256) {
    const float bb = backup[base + i];
    p[base + i] = bb;
    if (plow) plow[base + i] = (bf16)bb;
  }
}

inline bool finite_f(float x) { return x == x && x - x == 0.f; }

}  // namespace

extern "C" int nbest_sam_norms(const float* p, const float* g, const nbest_tensor_desc* descs, int n_tensors, int n_blocks, float eta,
                               float* partial, nbest_stream_t stream) {
  NB_CHECK(p && g && descs && partial && n_tensors > 0 && n_blocks > 0, NBEST_ERR_ARG, "sam_norms: bad arguments");
  NB_CHECK(finite_f(eta) && eta > 0.f, NBEST_ERR_ARG, "sam_norms: eta must be finite and > 0");
  NB_CHECK(nbest_bertadam_chunk() == kChunk, NBEST_ERR_ARG, "sam_norms: chunk size differs from the optimizer's");
  sam_norms_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>(p, g, descs, n_tensors, eta, partial);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_sam_perturb(float* p, const float* g, float* backup, void* p_lowp, const nbest_tensor_desc* descs, int n_tensors,
                                 int n_blocks, const float* norm, float rho, float eta, nbest_stream_t stream) {
  NB_CHECK(p && g && backup && descs && norm && n_tensors > 0 && n_blocks > 0, NBEST_ERR_ARG, "sam_perturb: bad arguments");
  NB_CHECK(finite_f(rho) && rho >= 0.f, NBEST_ERR_ARG, "sam_perturb: rho must be finite and >= 0");
  NB_CHECK(finite_f(eta) && eta != 0.f, NBEST_ERR_ARG, "sam_perturb: eta must be finite and not 0 (< 0: plain SAM)");
  NB_CHECK(nbest_bertadam_chunk() == kChunk, NBEST_ERR_ARG, "sam_perturb: chunk size differs from the optimizer's");
  sam_perturb_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>(p, g, backup, (bf16*)p_lowp, descs, n_tensors, norm, rho, eta);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_sam_restore(float* p, const float* backup, void* p_lowp, const nbest_tensor_desc* descs, int n_tensors, int n_blocks,
                                 nbest_stream_t stream) {
  NB_CHECK(p && backup && descs && n_tensors > 0 && n_blocks > 0, NBEST_ERR_ARG, "sam_restore: bad arguments");
  NB_CHECK(nbest_bertadam_chunk() == kChunk, NBEST_ERR_ARG, "sam_restore: chunk size differs from the optimizer's");
  sam_restore_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>(p, backup, (bf16*)p_lowp, descs, n_tensors);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
