// Functions of libnbest_hip.so that one source defines and another calls, declared once.  Every source includes this file
// (the .hip files through common.h), so a definition that drifts from its callers no longer compiles; the library links with
// -z defs, so a reference that nothing defines fails the link instead of the first ctypes call.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/nbest_hip.h"

struct Fp8Grad;   // common.h

// ---- api.cpp ------------------------------------------------------------------------------------
void nbest_set_error(const char* fmt, ...);

// ---- norm_embed.hip -----------------------------------------------------------------------------
int nbest_internal_layernorm_fwd8(const void* x, const float* gamma, const float* beta, void* y, void* y8, float* stats,
                                  int64_t M, int H, float eps, int dtype, nbest_stream_t stream, const uint32_t* a_prev, uint32_t* a_new);
int nbest_internal_layernorm_bwd8(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                                  void* dx_drop, float* dgamma, float* dbeta, float* dbias, int64_t M, int H, int dtype,
                                  int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws,
                                  size_t ws_bytes, nbest_stream_t stream, Fp8Grad f8);
// out[N] (+)= the sum of the nrows partial rows part[nrows][N] (fused column sums of the GEMM and attention epilogues)
int nbest_internal_partial_rows_sum(const float* part, int nrows, int N, float* out, int accumulate, hipStream_t st);
int nbest_internal_rows_drop_res(const void* x, int64_t ldx, const void* R, int64_t ldr, void* y, int64_t ldy, int64_t rows, int N,
                                 int64_t row_mul, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, hipStream_t st);
void nbest_internal_rowred_batch_begin();
void nbest_internal_rowred_batch_abort();
int nbest_internal_rowred_batch_flush(hipStream_t st);

// ---- attention.hip ------------------------------------------------------------------------------
int nbest_internal_attention_fwd8(const void* qkv, const uint8_t* key_mask, void* ctx, void* ctx8, float* lse, int B, int S, int heads,
                                  int d, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t stream,
                                  uint32_t* keep, const uint32_t* a_prev, uint32_t* a_new);
int nbest_internal_attention_bwd8(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx, const float* lse,
                                  void* dqkv, float* dbias, int accumulate, void* ws, size_t ws_bytes, int B, int S, int heads,
                                  int d, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t stream, Fp8Grad f8,
                                  const uint32_t* keep);
size_t nbest_internal_attention_keep_bytes(int B, int S, int heads);
int nbest_attention_cls_fwd_internal(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const uint8_t* key_mask, void* ctx,
                                     int64_t ldctx, int B, int S, int heads, int d, int dtype, nbest_stream_t stream, float drop_p,
                                     uint64_t seed, uint32_t drop_stream);
int nbest_internal_attention_cls_bwd(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx, void* dqkv, float* dbias,
                                     int accumulate, void* ws, size_t ws_bytes, int B, int S, int heads, int d, int dtype, float drop_p,
                                     uint64_t seed, uint32_t drop_stream, nbest_stream_t stream);
int nbest_internal_attention_cls_probs(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const uint8_t* key_mask, float* probs,
                                       int64_t ldp, int B, int S, int heads, int d, int dtype, nbest_stream_t stream);

// ---- token_prune.hip ----------------------------------------------------------------------------
// out[i] = mask[i] ? 1 : 0 (the key mask as the first scored layer's r_in)
int nbest_internal_mask_to_f32(const uint8_t* mask, float* out, int64_t n, hipStream_t stream);
// out [B][S] = the k origins of each utterance (origin [B][k]; NULL: 0 .. k-1), then -1
int nbest_internal_token_kept_row(const int32_t* origin, int32_t* out, int B, int S, int k, hipStream_t stream);

// ---- gemm.hip: what the GEMM generations share ---------------------------------------------------
// Split-K plan of a grid of `tiles` output tiles: the smallest split count whose grid fills whole rounds of the `slots`
// workgroups resident at once (>= 93 %) with at least `min_blocks` workgroups, else the one with the fullest rounds; each
// split keeps K >= 512 (at most 32 splits).  k_per_split is a multiple of 64.
void nb_splitk_plan(int64_t tiles, int64_t K, int64_t slots, int64_t min_blocks, int* splits, int64_t* k_per_split);
// C (+)= the sum of the `splits` fp32 slabs [splits][M][N]; rows >= m_split go to C2 (ldc2), the second output of a
// weight-gradient pair (m_split = M: none)
int nbest_internal_splitk_reduce(const float* slab, float* C, int64_t M, int64_t N, int64_t ldc, int splits, int accumulate,
                                 float* C2, int64_t m_split, int64_t ldc2, hipStream_t st);

// ---- gemm_f32.hip, gemm_bf16.hip (generation 1), gemm_bf16_v2.hip (generation 2) ----------------
// Called by the public entries of gemm.hip only, after their argument checks (for bf16: what every generation needs, including
// the 4 GiB operand extent the kernels' byte offsets rely on); each generation checks its own tile constraints.
// nbest_gemm_*_resolve: the kernel instantiation a checked problem runs on and the refusals that need no device (tile constraints, workspace
// sizes, epilogues not built) - host arithmetic only; each generation's launch switches on it and nbest_gemm_plan reports it
int nbest_gemm_f32_resolve(const nbest_gemm_args* a, nbest_gemm_plan_info* out);
int nbest_gemm_bf16_resolve(const nbest_gemm_args* a, nbest_gemm_plan_info* out);
int nbest_gemm_bf16_v2_resolve(const nbest_gemm_args* a, nbest_gemm_plan_info* out);
int nbest_gemm_f32(const nbest_gemm_args* a, hipStream_t st);
size_t nbest_gemm_bf16_ws_bytes(const nbest_gemm_args* a);
int nbest_gemm_bf16(const nbest_gemm_args* a, hipStream_t st);
size_t nbest_gemm_bf16_v2_ws_bytes(const nbest_gemm_args* a);
int nbest_gemm_bf16_v2(const nbest_gemm_args* a, hipStream_t st);
bool nbest_gemm_bf16_v2_wins(const nbest_gemm_args* a);   // per-shape choice of the kernel generation
size_t nbest_wgrad_pair_bf16_ws_bytes(const nbest_gemm_args* a, const nbest_gemm_args* b);
int nbest_wgrad_pair_bf16(const nbest_gemm_args* a, const nbest_gemm_args* b, hipStream_t st);
int nbest_wgrad_group_bf16(const nbest_gemm_args* problems, int n, hipStream_t st);
int nbest_wgrad_window_bf16(const nbest_gemm_args* problems, const int32_t* tile_first, const int32_t* tile_count, int n, hipStream_t st);
int nbest_pack_bn_internal(int64_t N);
int nbest_pack_weights_bf16(const void* src, void* dst, const nbest_matrix_desc* descs, int n_matrices, int n_stages, hipStream_t st);

// ---- gemm_fp8.hip -------------------------------------------------------------------------------
int nbest_internal_amax_bf16(const void* x, int64_t n, uint32_t* out, hipStream_t st);
int nbest_internal_cast_bf16_to_fp8(const void* src, void* dst, int64_t n, const uint32_t* a_prev, uint32_t* a_new, hipStream_t st);
