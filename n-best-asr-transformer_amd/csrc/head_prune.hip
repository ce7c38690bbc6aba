// Compact pruned heads: the weight images of an encoder whose layers keep k of their heads (include/nbest_hip.h), gathered from the
// arena and a head mask in ONE launch, and the host plan of their layout.  A pure gather: 16-byte accesses, plain vector stores,
// no atomics, every destination element written by exactly one thread - bit-reproducible.
//   Wqkv' [3 64k][H] T     row (t k + i) 64 + r  <-  row (t heads + idx[i]) 64 + r         bit copy
//   bqkv' [3 64k]    f32   the same mapping out of the fp32 arena                          bit copy
//   Wo'   [H][64k]   T     [n][i 64 + r] = T(gate[idx[i]] * float(Wo[n][idx[i] 64 + r]))   gate == 1: bit copy
#include <algorithm>

#include "common.h"

namespace {

constexpr int kPruneThreads = 256;

// blockIdx.y = layer; the layer's 16-byte vectors (N elements of T; 4 floats of the bias) in the order Wqkv' | bqkv' | Wo', one per
// thread and grid-stride step.  A vector never straddles a head: 64 % N == 0.
template <typename T, int N>
__global__ __launch_bounds__(kPruneThreads) void head_prune_pack_kernel(const T* __restrict__ wts, const float* __restrict__ prm,
                                                                        const float* __restrict__ gate,
                                                                        const nbest_head_prune_layer* __restrict__ table, int heads,
                                                                        T* __restrict__ w_out, float* __restrict__ b_out) {
  const int l = blockIdx.y;
  const nbest_head_prune_layer* L = table + l;
  const int k = L->k, H = heads * 64, Hk = k * 64;
  const int vpr = H / N;                                        // vectors per row of Wqkv'
  const int vpo = Hk / N;                                       // vectors per row of Wo'
  const int64_t nq = (int64_t)3 * Hk * vpr, nb = 3 * Hk / 4, no = (int64_t)H * vpo;
  for (int64_t v = (int64_t)blockIdx.x * kPruneThreads + threadIdx.x; v < nq + nb + no; v += (int64_t)gridDim.x * kPruneThreads) {
    if (v < nq) {
      const int row = (int)(v / vpr), c = (int)(v - (int64_t)row * vpr);
      const int t = row / Hk, rem = row - t * Hk, i = rem >> 6, r = rem & 63;
      const int srow = (t * heads + L->idx[i]) * 64 + r;
      *(i32x4*)(w_out + L->dst_wqkv + (int64_t)row * H + c * N) = *(const i32x4*)(wts + L->src_wqkv + (int64_t)srow * H + c * N);
    } else if (v < nq + nb) {
      const int e = (int)(v - nq) * 4;
      const int t = e / Hk, rem = e - t * Hk, i = rem >> 6, r = rem & 63;
      *(i32x4*)(b_out + L->dst_bqkv + e) = *(const i32x4*)(prm + L->src_bqkv + (t * heads + L->idx[i]) * 64 + r);
    } else {
      const int64_t u = v - nq - nb;
      const int n = (int)(u / vpo), c = (int)(u - (int64_t)n * vpo) * N;
      const int h = L->idx[c >> 6];
      const float g = gate[l * heads + h];
      const T* src = wts + L->src_wo + (int64_t)n * H + h * 64 + (c & 63);
      T* dst = w_out + L->dst_wo + (int64_t)n * Hk + c;
      if (g == 1.0f) {
        *(i32x4*)dst = *(const i32x4*)src;
      } else if constexpr (N == 8) {
        float x[8];
        Vec8<T>::load(src, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] *= g;
        Vec8<T>::store(dst, x);
      } else {
        const f32x4 x = Vec4<T>::load(src);
        Vec4<T>::store(dst, f32x4{x[0] * g, x[1] * g, x[2] * g, x[3] * g});
      }
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int nbest_head_prune_plan(const int32_t* k, int L, int heads, int dtype, nbest_head_prune_layer* layers, size_t* wqkv_bytes,
                                     size_t* wo_bytes, size_t* bqkv_bytes) {
  NB_CHECK(k && layers && L > 0, NBEST_ERR_ARG, "head_prune_plan: null pointer or L = %d", L);
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "head_prune_plan: bad dtype %d", dtype);
  NB_CHECK(heads > 0 && heads <= NBEST_HEAD_PRUNE_MAX_HEADS, NBEST_ERR_SHAPE, "head_prune_plan: heads %d outside 1 .. %d", heads,
           NBEST_HEAD_PRUNE_MAX_HEADS);
  for (int l = 0; l < L; ++l)
    NB_CHECK(k[l] >= 1 && k[l] <= heads, NBEST_ERR_ARG, "head_prune_plan: layer %d keeps %d heads (1 .. %d)", l, k[l], heads);
  const int64_t H = (int64_t)heads * 64, esz = dtype == NBEST_BF16 ? 2 : 4;
  int64_t q = 0, b = 0;
  for (int l = 0; l < L; ++l) {   // (3 64k H, 3 64k and H 64k are multiples of 64 elements: back to back keeps every tensor aligned)
    layers[l].k = k[l]; layers[l].pad = 0;
    layers[l].dst_wqkv = q; q += 3 * 64 * (int64_t)k[l] * H;
    layers[l].dst_bqkv = b; b += 3 * 64 * (int64_t)k[l];
  }
  int64_t o = q;
  for (int l = 0; l < L; ++l) { layers[l].dst_wo = o; o += H * 64 * (int64_t)k[l]; }
  if (wqkv_bytes) *wqkv_bytes = (size_t)(q * esz);
  if (wo_bytes) *wo_bytes = (size_t)((o - q) * esz);
  if (bqkv_bytes) *bqkv_bytes = (size_t)b * sizeof(float);
  return NBEST_OK;
}

extern "C" int nbest_head_prune_pack(const void* wts, const float* prm, const float* gate, const nbest_head_prune_layer* table_host,
                                     const nbest_head_prune_layer* table_dev, int L, int heads, int dtype, void* w_out, size_t w_bytes,
                                     float* b_out, size_t b_bytes, nbest_stream_t stream) {
  NB_CHECK(wts && prm && gate && table_host && table_dev && w_out && b_out, NBEST_ERR_ARG, "head_prune_pack: null pointer");
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "head_prune_pack: bad dtype %d", dtype);
  NB_CHECK(L > 0 && L <= 65535 && heads > 0 && heads <= NBEST_HEAD_PRUNE_MAX_HEADS, NBEST_ERR_SHAPE,
           "head_prune_pack: needs 0 < L <= 65535 (got %d) and 0 < heads <= %d (got %d)", L, NBEST_HEAD_PRUNE_MAX_HEADS, heads);
  NB_CHECK(aligned16(wts) && aligned16(prm) && aligned16(w_out) && aligned16(b_out), NBEST_ERR_ALIGN,
           "head_prune_pack: wts, prm, w_out and b_out must be 16-byte aligned");
  const int64_t H = (int64_t)heads * 64, esz = dtype == NBEST_BF16 ? 2 : 4, n = 16 / esz;
  int64_t most = 0;
  for (int l = 0; l < L; ++l) {
    const nbest_head_prune_layer& t = table_host[l];
    NB_CHECK(t.k >= 1 && t.k <= heads, NBEST_ERR_ARG, "head_prune_pack: layer %d keeps %d heads (1 .. %d)", l, t.k, heads);
    for (int i = 0; i < t.k; ++i)
      NB_CHECK(t.idx[i] >= 0 && t.idx[i] < heads && (i == 0 || t.idx[i] > t.idx[i - 1]), NBEST_ERR_ARG,
               "head_prune_pack: layer %d: kept head indices must ascend inside 0 .. %d", l, heads - 1);
    const int64_t Hk = 64 * (int64_t)t.k;
    NB_CHECK(t.src_wqkv >= 0 && t.src_bqkv >= 0 && t.src_wo >= 0 && t.src_wqkv % n == 0 && t.src_wo % n == 0 && t.src_bqkv % 4 == 0 &&
             t.dst_wqkv % n == 0 && t.dst_wo % n == 0 && t.dst_bqkv % 4 == 0, NBEST_ERR_ALIGN,
             "head_prune_pack: layer %d: offsets must be non-negative multiples of 16 bytes", l);
    NB_CHECK(t.dst_wqkv >= 0 && (uint64_t)(t.dst_wqkv + 3 * Hk * H) * esz <= w_bytes && t.dst_wo >= 0 &&
             (uint64_t)(t.dst_wo + H * Hk) * esz <= w_bytes && t.dst_bqkv >= 0 && (uint64_t)(t.dst_bqkv + 3 * Hk) * sizeof(float) <= b_bytes,
             NBEST_ERR_WORKSPACE, "head_prune_pack: layer %d: an image lies outside its buffer (%zu / %zu bytes)", l, w_bytes, b_bytes);
    most = std::max(most, (4 * Hk * H) / n + 3 * Hk / 4);
  }
  const int64_t blocks = (most + kPruneThreads - 1) / kPruneThreads;
  const dim3 grid((unsigned)(blocks < 2048 / L + 1 ? blocks : 2048 / L + 1), (unsigned)L);   // about 2048 workgroups in all, grid-stride
  hipStream_t st = (hipStream_t)stream;
  if (dtype == NBEST_BF16)
    hipLaunchKernelGGL((head_prune_pack_kernel<bf16, 8>), grid, dim3(kPruneThreads), 0, st, (const bf16*)wts, prm, gate, table_dev, heads,
                       (bf16*)w_out, b_out);
  else
    hipLaunchKernelGGL((head_prune_pack_kernel<float, 4>), grid, dim3(kPruneThreads), 0, st, (const float*)wts, prm, gate, table_dev, heads,
                       (float*)w_out, b_out);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
