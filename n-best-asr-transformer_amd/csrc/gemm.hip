// The GEMM code the kernel generations share, all of it host-side but the split-K reduce: the public entries (nbest_gemm and
// friends), their argument checks, the split-K plan and the split-K reduce.  The kernels live in gemm_f32.hip (fp32 parity
// path), gemm_bf16.hip (generation 1), gemm_bf16_v2.hip (generation 2) and gemm_fp8.hip.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, float* __restrict__ C, int64_t MN,
                                                            int64_t N, int64_t ldc, int splits, int accumulate,
                                                            float* __restrict__ C2, int64_t m_split, int64_t ldc2) {
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < MN; i += (int64_t)gridDim.x * blockDim.x * 4) {
    f32x4 s = *(const f32x4*)(slab + i);
    for (int z = 1; z < splits; ++z) s += *(const f32x4*)(slab + (int64_t)z * MN + i);
    const int64_t m = i / N, n = i - m * N;
    float* c = (m < m_split) ? C + m * ldc + n : C2 + (m - m_split) * ldc2 + n;
    if (accumulate) s += *(const f32x4*)c;
    *(f32x4*)c = s;
  }
}

// bias / R / U of the fused epilogues: present where the epilogue reads them (BIAS_GELU with a null U writes C only), R and U
// with leading dimensions that are multiples of `ld_mult` and `align`-byte aligned pointers
int check_epilogue_operands(const nbest_gemm_args* a, int64_t ld_mult, uintptr_t align) {
  const int epi = a->epilogue;
  if (epi == NBEST_EPI_BIAS || epi == NBEST_EPI_BIAS_GELU || epi == NBEST_EPI_BIAS_DROP_RES)
    NB_CHECK(a->bias, NBEST_ERR_ARG, "gemm: epilogue %d needs bias", epi);
  if (epi == NBEST_EPI_BIAS_DROP_RES || epi == NBEST_EPI_RES)
    NB_CHECK(a->R && a->ldr % ld_mult == 0 && ((uintptr_t)a->R & (align - 1)) == 0, NBEST_ERR_ARG, "gemm: epilogue %d needs R", epi);
  if ((epi == NBEST_EPI_BIAS_GELU && a->U) || epi == NBEST_EPI_DGELU)   // bf16: U = 8-bit GELU' rows (gd_pack4), ldu in bytes
    NB_CHECK(a->U && a->ldu % ld_mult == 0 && ((uintptr_t)a->U & (align - 1)) == 0, NBEST_ERR_ARG, "gemm: epilogue %d needs U", epi);
  return NBEST_OK;
}

// what every bf16 kernel generation needs of a problem; the tile constraints of each generation are checked in its file
int check_bf16(const nbest_gemm_args* a) {
  NB_CHECK(!(a->trans_a && !a->trans_b), NBEST_ERR_ARG, "gemm(bf16): trans_a without trans_b is not built");
  NB_CHECK(!a->trans_a || a->M % 128 == 0, NBEST_ERR_SHAPE, "gemm(bf16): trans_a needs M %% 128 == 0");
  NB_CHECK(a->lda % 8 == 0 && a->ldb % 8 == 0 && a->ldc % 8 == 0, NBEST_ERR_ALIGN, "gemm(bf16): leading dimensions must be multiples of 8");
  NB_CHECK(((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->B & 15) == 0 && ((uintptr_t)a->C & 15) == 0, NBEST_ERR_ALIGN,
           "gemm(bf16): pointers must be 16-byte aligned");
  // the kernels address A and B through buffer descriptors with 32-bit byte ranges
  const int64_t a_rows = a->trans_a ? a->K : a->M, a_cols = a->trans_a ? a->M : a->K;
  const int64_t b_rows = a->trans_b ? a->K : a->N, b_cols = a->trans_b ? a->N : a->K;
  const int64_t ab = ((a_rows - 1) * a->lda + a_cols) * 2, bb = ((b_rows - 1) * a->ldb + b_cols) * 2;
  NB_CHECK(ab < ((int64_t)1 << 32) && bb < ((int64_t)1 << 32), NBEST_ERR_SHAPE, "gemm(bf16): operand larger than 4 GiB");
  NB_CHECK(a->M * a->N < ((int64_t)1 << 32) || make_drop(a->drop_p, a->seed, a->drop_stream).thr16 == 0, NBEST_ERR_SHAPE,
           "gemm(bf16): dropout counter overflow");
  return check_epilogue_operands(a, 8, 16);
}

}  // namespace

void nb_splitk_plan(int64_t tiles, int64_t K, int64_t slots, int64_t min_blocks, int* splits, int64_t* k_per_split) {
  const int64_t maxs = (K / 512 < 1) ? 1 : ((K / 512 > 32) ? 32 : K / 512);
  int64_t best_s = 1;
  double best = -1.0;
  for (int64_t s = 1; s <= maxs; ++s) {
    const int64_t blocks = tiles * s;
    const double eff = (double)blocks / (double)(((blocks + slots - 1) / slots) * slots);
    if (eff > best + 1e-9) { best = eff; best_s = s; }
    if (blocks >= min_blocks && eff >= 0.93) { best_s = s; break; }
  }
  const int64_t k = round_up((K + best_s - 1) / best_s, 64);
  *splits = (int)((K + k - 1) / k);
  *k_per_split = k;
}

int nbest_internal_splitk_reduce(const float* slab, float* C, int64_t M, int64_t N, int64_t ldc, int splits, int accumulate,
                                 float* C2, int64_t m_split, int64_t ldc2, hipStream_t st) {
  const int64_t MN = M * N;
  int64_t g = (MN / 4 + 255) / 256;
  if (g > 2048) g = 2048;
  splitk_reduce_kernel<<<(int)g, 256, 0, st>>>(slab, C, MN, N, ldc, splits, accumulate, C2, m_split, ldc2);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

// ---- public dispatcher ----------------------------------------------------------------------------
extern "C" size_t nbest_gemm_ws_bytes(const nbest_gemm_args* a) {
  if (!a) return 0;
  if (a->dtype == NBEST_F32) return (a->colsum_out && a->epilogue != NBEST_EPI_F32_SPLITK) ? nbest_rowred_ws_bytes(a->M, a->N) : 0;
  if (a->dtype != NBEST_BF16) return 0;
  // callers size one workspace for whichever generation runs: take the larger requirement
  const size_t w1 = nbest_gemm_bf16_ws_bytes(a), w2 = nbest_gemm_bf16_v2_ws_bytes(a);
  return w1 > w2 ? w1 : w2;
}

// The argument checks of nbest_gemm and the kernel it resolves to, without the launch: host arithmetic on the argument block only - no
// HIP call, no pointer is dereferenced - so it answers on a machine without a GPU.  Every check is the one nbest_gemm runs, in its order.
extern "C" int nbest_gemm_plan(const nbest_gemm_args* a, nbest_gemm_plan_info* out) {
  NB_CHECK(out, NBEST_ERR_ARG, "gemm_plan: null output");
  *out = nbest_gemm_plan_info{};
  NB_CHECK(a && a->A && a->B && a->C, NBEST_ERR_ARG, "gemm: null pointer");
  NB_CHECK(a->M > 0 && a->N > 0 && a->K > 0, NBEST_ERR_SHAPE, "gemm: bad shape %lld x %lld x %lld", (long long)a->M,
           (long long)a->N, (long long)a->K);
  if (a->dtype == NBEST_F32) {
    if (int rc = check_epilogue_operands(a, 1, 1)) return rc;
    if (int rc = nbest_gemm_f32_resolve(a, out)) return rc;
    if (a->colsum_out && a->epilogue != NBEST_EPI_F32_SPLITK)
      NB_CHECK(a->ws && a->ws_bytes >= nbest_rowred_ws_bytes(a->M, a->N), NBEST_ERR_WORKSPACE, "gemm(f32): column-sum workspace too small");
    return NBEST_OK;
  }
  if (a->dtype == NBEST_BF16) {
    if (int rc = check_bf16(a)) return rc;
    return nbest_gemm_bf16_v2_wins(a) ? nbest_gemm_bf16_v2_resolve(a, out) : nbest_gemm_bf16_resolve(a, out);
  }
  nbest_set_error("gemm: bad dtype %d", a->dtype);
  return NBEST_ERR_DTYPE;
}

extern "C" int nbest_gemm(const nbest_gemm_args* a, nbest_stream_t stream) {
  NB_CHECK(a && a->A && a->B && a->C, NBEST_ERR_ARG, "gemm: null pointer");
  NB_CHECK(a->M > 0 && a->N > 0 && a->K > 0, NBEST_ERR_SHAPE, "gemm: bad shape %lld x %lld x %lld", (long long)a->M,
           (long long)a->N, (long long)a->K);
  if (a->dtype == NBEST_F32) {
    if (int rc = check_epilogue_operands(a, 1, 1)) return rc;
    if (int rc = nbest_gemm_f32(a, (hipStream_t)stream)) return rc;
    if (a->colsum_out && a->epilogue != NBEST_EPI_F32_SPLITK) {
      NB_CHECK(a->ws && a->ws_bytes >= nbest_rowred_ws_bytes(a->M, a->N), NBEST_ERR_WORKSPACE, "gemm(f32): column-sum workspace too small");
      return nbest_colsum(a->C, a->colsum_out, a->M, a->N, a->ldc, NBEST_F32, a->colsum_accumulate, a->ws, a->ws_bytes, stream);
    }
    return NBEST_OK;
  }
  if (a->dtype == NBEST_BF16) {
    if (int rc = check_bf16(a)) return rc;
    return nbest_gemm_bf16_v2_wins(a) ? nbest_gemm_bf16_v2(a, (hipStream_t)stream) : nbest_gemm_bf16(a, (hipStream_t)stream);
  }
  nbest_set_error("gemm: bad dtype %d", a->dtype);
  return NBEST_ERR_DTYPE;
}

// ---- pre-packed weight matrices (include/nbest_hip.h) ------------------------------------------------------------------
extern "C" int nbest_pack_bn(int64_t N) { return nbest_pack_bn_internal(N); }
extern "C" int nbest_pack_weights(const void* src, void* dst, const nbest_matrix_desc* descs, int n_matrices, int n_stages,
                                  nbest_stream_t stream) {
  NB_CHECK(src && dst && descs && n_matrices > 0 && n_stages > 0 && src != dst, NBEST_ERR_ARG, "pack_weights: bad arguments");
  return nbest_pack_weights_bf16(src, dst, descs, n_matrices, n_stages, (hipStream_t)stream);
}

// ---- two weight gradients, one launch (include/nbest_hip.h) ------------------------------------------------------------
extern "C" size_t nbest_wgrad_pair_ws_bytes(const nbest_gemm_args* a, const nbest_gemm_args* b) {
  if (!a || !b) return 0;
  return nbest_wgrad_pair_bf16_ws_bytes(a, b);
}

extern "C" int nbest_wgrad_pair(const nbest_gemm_args* a, const nbest_gemm_args* b, nbest_stream_t stream) {
  NB_CHECK(a && b && a->A && a->B && a->C && b->A && b->B && b->C, NBEST_ERR_ARG, "wgrad_pair: null pointer");
  NB_CHECK(a->M > 0 && b->M > 0 && a->N > 0 && a->K > 0, NBEST_ERR_SHAPE, "wgrad_pair: bad shape");
  NB_CHECK(nbest_wgrad_pair_bf16_ws_bytes(a, b) > 0, NBEST_ERR_SHAPE,
           "wgrad_pair: needs two bf16 F32_SPLITK problems (trans_a = trans_b = 1) with equal N, K and accumulate, M1, M2, N multiples of 256 "
           "and at least 18 output tiles in all");
  if (int rc = check_bf16(a)) return rc;
  if (int rc = check_bf16(b)) return rc;
  return nbest_wgrad_pair_bf16(a, b, (hipStream_t)stream);
}

// ---- up to 8 weight gradients, one launch without K-splits (include/nbest_hip.h) ----------------------------------------
static int check_wgrad_table(const char* who, const nbest_gemm_args* problems, int n) {
  for (int i = 0; i < n; ++i) {
    const nbest_gemm_args* a = problems + i;
    NB_CHECK(a->A && a->B && a->C, NBEST_ERR_ARG, "%s: null pointer in problem %d", who, i);
    NB_CHECK(a->M > 0 && a->N > 0 && a->K > 0, NBEST_ERR_SHAPE, "%s: bad shape in problem %d", who, i);
    NB_CHECK(a->dtype == NBEST_BF16, NBEST_ERR_DTYPE, "%s: bf16 operands only", who);
    NB_CHECK(a->M % 256 == 0 && a->N % 256 == 0, NBEST_ERR_SHAPE, "%s: problem %d: %lld x %lld is not a multiple of the 256 x 256 tile", who, i,
             (long long)a->M, (long long)a->N);
    if (int rc = check_bf16(a)) return rc;
  }
  return NBEST_OK;
}

extern "C" int nbest_wgrad_group(const nbest_gemm_args* problems, int n, nbest_stream_t stream) {
  NB_CHECK(problems && n >= 1 && n <= 8, NBEST_ERR_ARG, "wgrad_group: needs 1 .. 8 problems");
  if (int rc = check_wgrad_table("wgrad_group", problems, n)) return rc;
  return nbest_wgrad_group_bf16(problems, n, (hipStream_t)stream);
}

// ---- one window of at most 256 tiles out of up to 16 weight gradients (include/nbest_hip.h) ------------------------------
extern "C" int nbest_wgrad_window(const nbest_gemm_args* problems, const int32_t* tile_first, const int32_t* tile_count, int n,
                                  nbest_stream_t stream) {
  NB_CHECK(problems && tile_first && tile_count && n >= 1 && n <= 16, NBEST_ERR_ARG, "wgrad_window: needs 1 .. 16 entries");
  if (int rc = check_wgrad_table("wgrad_window", problems, n)) return rc;
  return nbest_wgrad_window_bf16(problems, tile_first, tile_count, n, (hipStream_t)stream);
}
