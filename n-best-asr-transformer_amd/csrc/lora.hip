// K9l LoRA on merged weights (--lora_rank; new functionality, the reference has none): two HBM-streaming kernels that run once
// per optimizer step next to K9.  The encoder never sees the factors: it reads W = W0 + s B A from the arenas as always.
//   merge: p = base + s (B A) over every adapted block (+ the bf16 copy), one writer per element;
//   grad : dA = s B^T dW, dB = s dW A^T from the dense gradient the weight-gradient GEMMs left in g: g is read ONCE, tile partials
//          go to a workspace and a second launch adds them in a fixed order (no atomics, no workgroup waits for another).
// Both walk the same tiles: block b -> (descriptor, 64 rows x 256 columns) by a binary search over desc.tile_start.  A workgroup
// stages the tile's A rows [r][256] and B rows [64][r] in LDS (dynamic: 1280 r bytes, 80 KB at r = 64); lane l of every wave owns
// columns 4 l .. 4 l + 3 (one 16-byte access per row), wave w the rows 16 w .. 16 w + 15, so a B element is one LDS broadcast.
#include "common.h"

namespace {

constexpr int kTR = 64;    // tile rows
constexpr int kTC = 256;   // tile columns: 64 lanes x 4
constexpr int kRedY = 16;  // workgroups per descriptor of the reduce launch

__device__ __forceinline__ nbest_lora_desc find_desc(const nbest_lora_desc* __restrict__ d, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].tile_start <= blk) lo = mid; else hi = mid - 1;
  }
  return d[lo];
}

// the tile's factors into LDS, zero where the tile hangs over the block: As [r][kTC], Bs [kTR][r]
__device__ __forceinline__ void stage_factors(const float* __restrict__ ab, const nbest_lora_desc& d, int r0, int c0, float* As, float* Bs) {
  const int r = d.rank;
  const float* A = ab + d.a_off;
  for (int idx = threadIdx.x; idx < r * (kTC / 4); idx += 256) {
    const int k = idx >> 6, col = c0 + 4 * (idx & 63);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < d.cols) v = *(const f32x4*)(A + (int64_t)k * d.cols + col);
    *(f32x4*)(As + k * kTC + 4 * (idx & 63)) = v;
  }
  const int nrows = (d.rows - r0 < kTR) ? d.rows - r0 : kTR;
  const int count = nrows * r;                        // the tile's B rows are contiguous
  const float* Bsrc = ab + d.b_off + (int64_t)r0 * r;   // 16-byte aligned: b_off % 4 == 0 and r0 % 64 == 0
  for (int idx = 4 * threadIdx.x; idx < kTR * r; idx += 1024) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (idx + 3 < count) {
      v = *(const f32x4*)(Bsrc + idx);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (idx + e < count) v[e] = Bsrc[idx + e];
    }
    *(f32x4*)(Bs + idx) = v;
  }
}

// base + s acc; a result that compares equal to base keeps base's bits (B = 0 leaves a -0.0 of the base alone)
__device__ __forceinline__ float merge1(float base, float acc, float s) {
  const float o = base + s * acc;
  return o == base ? base : o;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(float* __restrict__ p, bf16* __restrict__ plow, const float* __restrict__ base,
                                                         const float* __restrict__ ab, const nbest_lora_desc* __restrict__ descs, int n) {
  extern __shared__ __attribute__((aligned(16))) float lora_smem[];
  const nbest_lora_desc d = find_desc(descs, n, blockIdx.x);
  const int r = d.rank;
  float* As = lora_smem;
  float* Bs = As + r * kTC;
  const int t = blockIdx.x - d.tile_start, nct = (d.cols + kTC - 1) / kTC;
  const int r0 = (t / nct) * kTR, c0 = (t % nct) * kTC;
  stage_factors(ab, d, r0, c0, As, Bs);
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = c0 + 4 * tx;
  if (col >= d.cols) return;
#pragma unroll 1
  for (int ib = 0; ib < 4; ++ib) {
    const int li = ty * 16 + ib * 4;                  // first of four tile rows
    f32x4 acc[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[rr] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < r; ++k) {                     // k ascending
      const f32x4 a = *(const f32x4*)(As + k * kTC + 4 * tx);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float b = Bs[(li + rr) * r + k];
        acc[rr] += b * a;
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = r0 + li + rr;
      if (row < d.rows) {
        const f32x4 w0 = *(const f32x4*)(base + d.base_off + (int64_t)row * d.cols + col);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = merge1(w0[e], acc[rr][e], d.scale);
        const int64_t at = d.p_off + (int64_t)row * d.stride + col;
        *(f32x4*)(p + at) = o;
        if (plow) Vec4<bf16>::store(plow + at, o);
      }
    }
  }
}

// tile partials: ws_dA [row tile][r][cols] (the tile's 64 rows summed: in-thread over a wave's 16 rows, then the four waves in
// order through LDS), ws_dB [column tile][rows][r] (the tile's 256 columns summed inside one wave).  Every element the reduce
// launch reads is written here, whatever the workspace held.
__global__ __launch_bounds__(256) void lora_grad_kernel(const float* __restrict__ g, const float* __restrict__ ab, float* __restrict__ ws,
                                                        const nbest_lora_desc* __restrict__ descs, int n) {
  extern __shared__ __attribute__((aligned(16))) float lora_smem[];
  const nbest_lora_desc d = find_desc(descs, n, blockIdx.x);
  const int r = d.rank;
  float* As = lora_smem;
  float* Bs = As + r * kTC;
  float* red = Bs + kTR * r;                          // [4 k][4 waves][kTC]
  const int t = blockIdx.x - d.tile_start, nct = (d.cols + kTC - 1) / kTC, nrt = (d.rows + kTR - 1) / kTR;
  const int rt = t / nct, ct = t % nct;
  const int r0 = rt * kTR, c0 = ct * kTC;
  stage_factors(ab, d, r0, c0, As, Bs);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = c0 + 4 * tx;
  const bool active = col < d.cols;
  f32x4 gv[16];
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) {
    const int row = r0 + ty * 16 + ii;
    gv[ii] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active && row < d.rows) gv[ii] = *(const f32x4*)(g + d.p_off + (int64_t)row * d.stride + col);
  }
  __syncthreads();
  float* wsA = ws + d.ws_off + (int64_t)rt * r * d.cols;
  float* wsB = ws + d.ws_off + (int64_t)nrt * r * d.cols + (int64_t)ct * d.rows * r;
  for (int k0 = 0; k0 < r; k0 += 4) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = k0 + kk;
      if (k < r) {                                    // uniform
        const f32x4 a = *(const f32x4*)(As + k * kTC + 4 * tx);
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        float keep = 0.f;
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
          const float b = Bs[(ty * 16 + ii) * r + k];
          s += b * gv[ii];
          float dot = (gv[ii][0] * a[0] + gv[ii][1] * a[1]) + (gv[ii][2] * a[2] + gv[ii][3] * a[3]);
          dot = wave_sum_dpp(dot);
          if (tx == ii) keep = dot;
        }
        const int row = r0 + ty * 16 + tx;
        if (tx < 16 && row < d.rows) wsB[(int64_t)row * r + k] = keep;
        *(f32x4*)(red + (kk * 4 + ty) * kTC + 4 * tx) = s;
      }
    }
    __syncthreads();
    const int k = k0 + ty;                            // wave w adds the four waves' sums of k0 + w, in wave order
    if (k < r && active) {
      const float* q = red + (ty * 4) * kTC + 4 * tx;
      f32x4 s = *(const f32x4*)q;
      s += *(const f32x4*)(q + kTC);
      s += *(const f32x4*)(q + 2 * kTC);
      s += *(const f32x4*)(q + 3 * kTC);
      *(f32x4*)(wsA + (int64_t)k * d.cols + col) = s;
    }
    __syncthreads();
  }
}

// dA = s sum over row tiles, dB = s sum over column tiles, tiles ascending
__global__ __launch_bounds__(256) void lora_grad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gab,
                                                               const nbest_lora_desc* __restrict__ descs) {
  const nbest_lora_desc d = descs[blockIdx.x];
  const int nct = (d.cols + kTC - 1) / kTC, nrt = (d.rows + kTR - 1) / kTR;
  const int64_t nA = (int64_t)d.rank * d.cols, nB = (int64_t)d.rows * d.rank;
  const float* wa = ws + d.ws_off;
  const float* wb = wa + nrt * nA;
  for (int64_t e = 4 * ((int64_t)blockIdx.y * 256 + threadIdx.x); e < nA; e += 4 * kRedY * 256) {   // nA % 4 == 0
    f32x4 s = *(const f32x4*)(wa + e);
    for (int i = 1; i < nrt; ++i) s += *(const f32x4*)(wa + i * nA + e);
    *(f32x4*)(gab + d.a_off + e) = d.scale * s;
  }
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < nB; e += kRedY * 256) {
    float s = wb[e];
    for (int i = 1; i < nct; ++i) s += wb[i * nB + e];
    gab[d.b_off + e] = d.scale * s;
  }
}

size_t lora_lds_bytes(int rank, bool grad) { return ((size_t)rank * (kTC + kTR) + (grad ? 16 * kTC : 0)) * sizeof(float); }

int64_t lora_ws_elems(const nbest_lora_desc& d) {
  const int64_t nct = (d.cols + kTC - 1) / kTC, nrt = (d.rows + kTR - 1) / kTR;
  return round_up(nrt * (int64_t)d.rank * d.cols + nct * (int64_t)d.rows * d.rank, 4);
}

// what both entries need of the host table; *n_tiles, *max_rank and *ws_elems as nbest_lora_plan lays them out
int lora_check(const char* who, const nbest_lora_desc* h, int n, int* n_tiles, int* max_rank, int64_t* ws_elems) {
  NB_CHECK(h && n > 0, NBEST_ERR_ARG, "%s: no descriptors", who);
  int64_t tiles = 0, ws = 0;
  int mr = 0;
  for (int i = 0; i < n; ++i) {
    const nbest_lora_desc& d = h[i];
    NB_CHECK(d.rank >= 1 && d.rank <= NBEST_LORA_MAX_RANK, NBEST_ERR_ARG, "%s: block %d has rank %d (1 .. %d)", who, i, d.rank,
             NBEST_LORA_MAX_RANK);
    NB_CHECK(d.rows > 0 && d.cols > 0 && d.cols % 4 == 0, NBEST_ERR_SHAPE, "%s: block %d is %d x %d (cols must be a positive multiple of 4)",
             who, i, d.rows, d.cols);
    NB_CHECK(d.stride == d.cols, NBEST_ERR_SHAPE, "%s: block %d has row stride %d, not cols = %d", who, i, d.stride, d.cols);
    NB_CHECK(d.p_off >= 0 && d.base_off >= 0 && d.a_off >= 0 && d.b_off >= 0, NBEST_ERR_ARG, "%s: block %d has a negative offset", who, i);
    NB_CHECK(((d.p_off | d.base_off | d.a_off | d.b_off) & 3) == 0, NBEST_ERR_ALIGN, "%s: block %d: offsets must be multiples of 4 elements",
             who, i);
    NB_CHECK(d.tile_start == tiles && d.ws_off == ws, NBEST_ERR_ARG, "%s: block %d: tile_start / ws_off are not nbest_lora_plan's", who, i);
    tiles += (int64_t)((d.rows + kTR - 1) / kTR) * ((d.cols + kTC - 1) / kTC);
    ws += lora_ws_elems(d);
    NB_CHECK(tiles < (1 << 30), NBEST_ERR_SHAPE, "%s: too many tiles", who);
    if (d.rank > mr) mr = d.rank;
  }
  *n_tiles = (int)tiles;
  *max_rank = mr;
  *ws_elems = ws;
  return NBEST_OK;
}

}  // namespace

extern "C" int nbest_lora_plan(nbest_lora_desc* descs_host, int n, int* n_tiles, size_t* ws_bytes) {
  NB_CHECK(descs_host && n > 0, NBEST_ERR_ARG, "lora_plan: no descriptors");
  int64_t tiles = 0, ws = 0;
  for (int i = 0; i < n; ++i) {
    nbest_lora_desc& d = descs_host[i];
    NB_CHECK(d.rows > 0 && d.cols > 0 && d.rank >= 1 && d.rank <= NBEST_LORA_MAX_RANK, NBEST_ERR_ARG, "lora_plan: block %d: bad rows / cols / rank", i);
    d.tile_start = (int32_t)tiles;
    d.ws_off = ws;
    tiles += (int64_t)((d.rows + kTR - 1) / kTR) * ((d.cols + kTC - 1) / kTC);
    ws += lora_ws_elems(d);
    NB_CHECK(tiles < (1 << 30), NBEST_ERR_SHAPE, "lora_plan: too many tiles");
  }
  if (n_tiles) *n_tiles = (int)tiles;
  if (ws_bytes) *ws_bytes = (size_t)ws * sizeof(float);
  return NBEST_OK;
}

extern "C" size_t nbest_lora_grad_ws_bytes(const nbest_lora_desc* descs_host, int n) {
  if (!descs_host || n <= 0) return 0;
  int64_t ws = 0;
  for (int i = 0; i < n; ++i) {
    const nbest_lora_desc& d = descs_host[i];
    if (d.rows <= 0 || d.cols <= 0 || d.rank < 1) return 0;
    ws += lora_ws_elems(d);
  }
  return (size_t)ws * sizeof(float);
}

extern "C" int nbest_lora_merge(float* p, void* p_lowp, const float* base, const float* ab, const nbest_lora_desc* descs_host,
                                const nbest_lora_desc* descs_dev, int n, nbest_stream_t stream) {
  NB_CHECK(p && base && ab && descs_host && descs_dev, NBEST_ERR_ARG, "lora_merge: null pointer");
  int tiles, mr;
  int64_t ws;
  if (int rc = lora_check("lora_merge", descs_host, n, &tiles, &mr, &ws)) return rc;
  NB_CHECK((((uintptr_t)p | (uintptr_t)base | (uintptr_t)ab) & 15) == 0 && ((uintptr_t)p_lowp & 7) == 0, NBEST_ERR_ALIGN,
           "lora_merge: p, base and ab must be 16-byte aligned (p_lowp 8-byte)");
  const size_t lds = lora_lds_bytes(mr, false);
  (void)hipFuncSetAttribute((const void*)lora_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  lora_merge_kernel<<<tiles, 256, lds, (hipStream_t)stream>>>(p, (bf16*)p_lowp, base, ab, descs_dev, n);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_lora_grad(const float* g, const float* ab, float* g_ab, const nbest_lora_desc* descs_host,
                               const nbest_lora_desc* descs_dev, int n, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(g && ab && g_ab && descs_host && descs_dev && ws, NBEST_ERR_ARG, "lora_grad: null pointer");
  int tiles, mr;
  int64_t need;
  if (int rc = lora_check("lora_grad", descs_host, n, &tiles, &mr, &need)) return rc;
  NB_CHECK(ws_bytes >= (size_t)need * sizeof(float), NBEST_ERR_WORKSPACE, "lora_grad: workspace too small (%zu < %zu bytes)", ws_bytes,
           (size_t)need * sizeof(float));
  NB_CHECK((((uintptr_t)g | (uintptr_t)ab | (uintptr_t)g_ab | (uintptr_t)ws) & 15) == 0, NBEST_ERR_ALIGN,
           "lora_grad: g, ab, g_ab and ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = lora_lds_bytes(mr, true);
  (void)hipFuncSetAttribute((const void*)lora_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  lora_grad_kernel<<<tiles, 256, lds, st>>>(g, ab, (float*)ws, descs_dev, n);
  NB_LAUNCH_CHECK();
  lora_grad_reduce_kernel<<<dim3(n, kRedY), 256, 0, st>>>((const float*)ws, g_ab, descs_dev);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
