// Token elimination between encoder layers (PoWER-BERT, Goyal et al., ICML 2020, at a fixed count per layer): the per-utterance
// top-k selection, the row compaction that follows it, and the two small launches the inference composite needs around them.
//   nbest_token_select: one workgroup per utterance, one thread per position (blockDim = S rounded up to whole waves).
//     Every position gets ONE 64-bit key whose unsigned order is the selection order (include/nbest_hip.h):
//       bit 43      position 0 (always kept)
//       bit 42      unmasked
//       bit 41      the score is a number (not a NaN)
//       bits 9..40  the score's bits mapped so that unsigned order = float order (-0 folded into +0 first; 0 for a NaN)
//       bits 0..8   511 - position (lower index first)
//     Keys of different positions differ, so "the number of keys above mine" is a permutation of 0 .. S-1: the rank.  The keys sit
//     in LDS; a thread reads all of them two at a time (every lane the same address: an LDS broadcast, no bank conflict) and counts
//     with a compare and an add - at most 512 x 512 comparisons per utterance, no branch, no sort network.  rank < k = kept; the
//     output slot of a kept position is the number of kept positions below it: popcount of the wave's ballot under the lane, plus the
//     counts of the waves before it (8 words of LDS).  Ascending positions, every output element written once, no atomics.
//   nbest_rows_compact: dst[b][r][:] = src[b][idx[b][r]][:], one 16-byte vector per thread.  An index outside [0, S) cannot leave
//     the source tensor: it is clamped (the selection never produces one).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned long long u64x2;

__global__ __launch_bounds__(512) void token_select_kernel(const float* __restrict__ score, const uint8_t* __restrict__ mask,
                                                           const int32_t* __restrict__ origin_in, int32_t* __restrict__ idx_out,
                                                           uint8_t* __restrict__ mask_out, float* __restrict__ maskf_out,
                                                           int32_t* __restrict__ origin_out, int S, int k) {
  __shared__ __attribute__((aligned(16))) unsigned long long keys[512];
  __shared__ int wave_kept[8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t row = (int64_t)blockIdx.x * S;
  const int Sp = (S + 1) & ~1;   // the keys are read in pairs: an odd S is padded with key 0, which is above no key
  unsigned long long key = 0;
  bool m = false;
  if (t < S) {
    m = mask[row + t] != 0;
    const float s = score[row + t] + 0.f;   // -0 -> +0: the two compare equal, so they must tie
    const bool num = s == s;
    const uint32_t u = __float_as_uint(s);
    const uint32_t mono = num ? (u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u)) : 0u;
    const uint32_t cls = (t == 0 ? 4u : 0u) | (m ? 2u : 0u) | (num ? 1u : 0u);
    key = ((unsigned long long)cls << 41) | ((unsigned long long)mono << 9) | (unsigned long long)(511 - t);
  }
  if (t < Sp) keys[t] = key;
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < Sp; j += 2) {
    const u64x2 kk = *(const u64x2*)&keys[j];
    rank += (kk[0] > key ? 1 : 0) + (kk[1] > key ? 1 : 0);
  }
  const bool kept = t < S && rank < k;
  const unsigned long long ballot = __ballot(kept);
  if (lane == 0) wave_kept[wave] = __popcll(ballot);
  __syncthreads();
  int slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0));
  for (int w = 0; w < wave; ++w) slot += wave_kept[w];
  if (kept) {   // exactly k threads of the workgroup, slots 0 .. k-1
    const int64_t o = (int64_t)blockIdx.x * k + slot;
    idx_out[o] = t;
    mask_out[o] = m ? 1 : 0;
    maskf_out[o] = m ? 1.f : 0.f;
    if (origin_out) origin_out[o] = origin_in ? origin_in[row + t] : t;
  }
}

__global__ __launch_bounds__(256) void rows_compact_kernel(const i32x4* __restrict__ src, const int32_t* __restrict__ idx,
                                                           i32x4* __restrict__ dst, int S, int k, int V, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = i / V, b = r / k;
  const int v = (int)(i - r * V);
  const int s = min(max(idx[r], 0), S - 1);
  dst[i] = src[(b * S + s) * V + v];
}

__global__ __launch_bounds__(256) void mask_to_f32_kernel(const uint8_t* __restrict__ mask, float* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = mask[i] ? 1.f : 0.f;
}

// out[b][j] = j < k ? (origin ? origin[b][j] : j) : -1, out rows S wide
__global__ __launch_bounds__(256) void token_kept_row_kernel(const int32_t* __restrict__ origin, int32_t* __restrict__ out, int S, int k,
                                                             int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / S;
  const int j = (int)(i - b * S);
  out[i] = j < k ? (origin ? origin[b * k + j] : j) : -1;
}

}  // namespace

extern "C" int nbest_token_select(const float* score, const uint8_t* key_mask, const int32_t* origin_in, int k, int32_t* idx_out,
                                  uint8_t* mask_out, float* maskf_out, int32_t* origin_out, int B, int S, nbest_stream_t stream) {
  NB_CHECK(score && key_mask && idx_out && mask_out && maskf_out, NBEST_ERR_ARG, "token_select: null pointer");
  NB_CHECK((const void*)idx_out != (const void*)score && (const void*)idx_out != (const void*)key_mask &&
               (const void*)idx_out != (const void*)origin_in, NBEST_ERR_ARG, "token_select: idx_out aliases an input");
  NB_CHECK((const void*)mask_out != (const void*)key_mask && (const void*)maskf_out != (const void*)score &&
               (!origin_out || (const void*)origin_out != (const void*)origin_in), NBEST_ERR_ARG,
           "token_select: an output aliases its input (every workgroup reads its whole input row)");
  NB_CHECK(B > 0, NBEST_ERR_SHAPE, "token_select: bad shape (B=%d)", B);
  NB_CHECK(S >= 1 && S <= 512, NBEST_ERR_SHAPE, "token_select: S=%d outside 1..512", S);
  NB_CHECK(k >= 1 && k <= S, NBEST_ERR_SHAPE, "token_select: k=%d outside 1..S=%d", k, S);
  NB_CHECK((((uintptr_t)score | (uintptr_t)origin_in | (uintptr_t)idx_out | (uintptr_t)maskf_out | (uintptr_t)origin_out) & 3) == 0,
           NBEST_ERR_ALIGN, "token_select: score, origins, idx_out and maskf_out must be 4-byte aligned");
  token_select_kernel<<<B, (S + 63) / 64 * 64, 0, (hipStream_t)stream>>>(score, key_mask, origin_in, idx_out, mask_out, maskf_out,
                                                                         origin_out, S, k);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_rows_compact(const void* src, const int32_t* idx, void* dst, int B, int S, int k, int H, int dtype,
                                  nbest_stream_t stream) {
  NB_CHECK(src && idx && dst, NBEST_ERR_ARG, "rows_compact: null pointer");
  NB_CHECK(src != dst, NBEST_ERR_ARG, "rows_compact: src and dst must be different buffers");
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "rows_compact: bad dtype %d", dtype);
  NB_CHECK(B > 0 && S >= 1 && k >= 1 && k <= S && H > 0, NBEST_ERR_SHAPE, "rows_compact: bad shape (B=%d S=%d k=%d H=%d)", B, S, k, H);
  const int per = dtype == NBEST_BF16 ? 8 : 4;   // elements per 16 bytes
  NB_CHECK(H % per == 0, NBEST_ERR_SHAPE, "rows_compact: H=%d must be a multiple of %d (16-byte rows)", H, per);
  NB_CHECK((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && ((uintptr_t)idx & 3) == 0, NBEST_ERR_ALIGN,
           "rows_compact: src and dst must be 16-byte aligned, idx 4-byte aligned");
  const int V = H / per;
  const int64_t n = (int64_t)B * k * V;
  rows_compact_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>((const i32x4*)src, idx, (i32x4*)dst, S, k, V, n);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

int nbest_internal_mask_to_f32(const uint8_t* mask, float* out, int64_t n, hipStream_t stream) {
  mask_to_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(mask, out, n);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

int nbest_internal_token_kept_row(const int32_t* origin, int32_t* out, int B, int S, int k, hipStream_t stream) {
  const int64_t n = (int64_t)B * S;
  token_kept_row_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(origin, out, S, k, n);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
