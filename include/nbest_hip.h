/* nbest_hip.h - C ABI of libnbest_hip.so: the MI355X (gfx950) fine-tuning hot path of
 * N-Best-ASR-Transformer.
 *
 * The reference has NO native / FFI / plugin interface: its only seam is the Python
 * object injected at /root/reference/models/model.py:19 and called at :43-45,54-56.  This header is
 * therefore the boundary a maintainer binds from Python with ctypes (INTEGRATION.md shows the stub);
 * each entry point cites the reference (or third-party) code whose arithmetic it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller unless the
 *     name ends in _host; the library never allocates, never synchronises, never touches the default
 *     stream: work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - returns NBEST_OK (0) or a negative NBEST_ERR_*; nbest_last_error() gives the message
 *     (thread-local).  No global mutable state and no environment variables: entry points are re-entrant and the
 *     library has one code path per shape.
 *   - dtype: NBEST_F32 or NBEST_BF16 = type of activations, weight matrices and embedding tables.
 *     Biases, LayerNorm parameters, statistics, losses, gradients of parameters and optimizer state
 *     are always fp32.
 *   - matrices are row-major; "M" is the number of token rows B*S.
 *   - dropout: (p, seed, stream_id) select a counter-based mask that forward and backward
 *     regenerate identically; p = 0 disables it (parity runs).
 */
#ifndef NBEST_HIP_H
#define NBEST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBEST_ABI_VERSION 1

enum { NBEST_OK = 0, NBEST_ERR_ARG = -1, NBEST_ERR_SHAPE = -2, NBEST_ERR_DTYPE = -3, NBEST_ERR_ALIGN = -4,
       NBEST_ERR_LAUNCH = -5, NBEST_ERR_WORKSPACE = -6 };
enum { NBEST_F32 = 0, NBEST_BF16 = 1 };

typedef void* nbest_stream_t; /* hipStream_t */

int nbest_version(void);
/* copies the calling thread's last error message into buf (NUL-terminated); returns its length */
int nbest_last_error(char* buf, size_t n);

/* ---------------------------------------------------------------------------------------------
 * K1  embedding gather + LayerNorm (+dropout)
 * replaces transformers BertEmbeddings / XLMRobertaEmbeddings (installed modeling_bert.py:53-108),
 * reached from /root/reference/models/model.py:43-45.
 *   out[m,:] = drop(LN(word[ids[m]] + type[seg[m]] + ptab[pos[m]]))     stats[m] = {mean, rstd}
 * seg may be NULL (all zeros).  pos is explicit (BERT: arange; XLM-R: pad-offset cumsum).          */
int nbest_embed_ln_fwd(const int64_t* ids, const int64_t* seg, const int64_t* pos, const void* word,
                       const void* type, const void* ptab, const float* gamma, const float* beta, void* out,
                       float* stats, int64_t M, int H, float eps, int dtype, float drop_p, uint64_t seed,
                       uint32_t drop_stream, nbest_stream_t stream);
/* backward: LN backward on dout, then the sums into the fp32 table gradients - the index_add of the installed BertEmbeddings
 * backward behind /root/reference/models/model.py:43-45 - WITHOUT float atomics: a segmented reduce over the tokens sorted by
 * word id, every addition in a fixed order (bit-reproducible run to run).
 *   perm [B*S] int32 (REQUIRED): token indices sorted by ids, ties in ascending token index (any STABLE argsort of ids; the
 *        data loader builds it next to ids - nbest_amd/trainer.py EncodedSplit.host_batch, bench.py).
 * Rows word_pad_id of dword and pos_pad_id of dptab receive nothing (nn.Embedding padding_idx; pass -1 for "no padding row").
 * tables_accumulate == 0: every row of dword / dptab / dtype_tab that a token of the batch reaches (word_pad_id / pos_pad_id
 * rows excepted), and dtype_tab rows 0 and 1 (row 1 when n_types > 1), is OVERWRITTEN with the gradient; every other row is left as
 * it is.  != 0: the gradient is added to those rows.  dgamma / dbeta are overwritten unless accumulate.
 * Bit-reproducible when, in every sequence position j, all non-padding rows carry the same position key, no two positions share
 * a key, and token types are 0 / 1: BERT's arange positions and right-padded RoBERTa-family positions (cumsum of non-padding
 * tokens), in ANY row order.  Any other in-range layout (left padding, a padding id inside a row, arbitrary or repeated keys,
 * token types >= 2) is summed correctly, partly with float atomics on dptab / dtype_tab (not reproducible in the last bit).
 * Tables are fp32, 16-byte aligned.  M = B*S < 2^31.  ws: >= nbest_embed_bwd_ws_bytes(M, H) bytes. */
int nbest_embed_ln_bwd(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                       const void* type, const void* ptab, const float* gamma, const float* stats,
                       const void* dout, float* dword, float* dtype_tab, float* dptab, float* dgamma,
                       float* dbeta, int B, int S, int H, int n_types, int dtype, int64_t word_pad_id,
                       int64_t pos_pad_id, int accumulate, int tables_accumulate, float drop_p, uint64_t seed,
                       uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream);
size_t nbest_embed_bwd_ws_bytes(int64_t M, int64_t H);
/* Adversarial training on the word embeddings, the fast gradient method (new functionality: the reference has none; Miyato et al.,
 * ICLR 2017).  With delta fp32 [M][H] (device), row m of the embedding sum becomes
 *   e'[m,:] = ((word[ids[m]] + delta[m,:]) + type[seg[m]]) + ptab[pos[m]]
 * in fp32 from the stored table rows, in this order in the forward and in the backward's recomputation of x_hat; a zero delta row gives
 * the bits of the plain row.
 * nbest_embed_ln_fwd_adv: nbest_embed_ln_fwd on e' (the same kernel, one more instantiation); stats are those of e'.
 * nbest_embed_ln_bwd_adv: nbest_embed_ln_bwd for a forward that ran on e' (stats from it).  delta is a constant: it gets no gradient.
 *   perm, determinism, accumulate / tables_accumulate and the fallback layouts as documented there; same workspace.
 * nbest_embed_adv_delta forms delta from dout [B*S][H] (dtype) = the gradient w.r.t. the embedding LayerNorm output of a CLEAN pass
 * (what nbest_encoder_backward leaves in dhidden after layer_begin = 0) in two launches:
 *   1. one wave per token: g[m,:] = ((d gamma) - mean(d gamma) - x_hat mean(d gamma x_hat)) rstd, d = dout[m,:] under the forward's
 *      keep bits and scale (drop_p, seed, drop_stream: the pass's hidden_drop, seed and drop_stream_base; element index m H + c), mean,
 *      rstd and x_hat recomputed from the clean row - equal to the forward's statistics to rounding; g[m,:] = 0 exactly where
 *      key_mask[m] == 0.  g goes to delta (fp32), its sum of squares per row to the workspace.
 *   2. per utterance b: n_b = sqrt(sum of the S row values in ascending t) -> norm[b] (fp32 [B]); delta[m,:] = g[m,:] (epsilon / n_b)
 *      in place; n_b zero or not finite: every delta row of the utterance is exactly 0.
 * No atomics, fixed summation order: bit-reproducible.  epsilon finite, >= 0.  ws >= nbest_embed_adv_ws_bytes(B, S).               */
int nbest_embed_ln_fwd_adv(const int64_t* ids, const int64_t* seg, const int64_t* pos, const void* word, const void* type,
                           const void* ptab, const float* gamma, const float* beta, const float* delta, void* out, float* stats,
                           int64_t M, int H, float eps, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                           nbest_stream_t stream);
int nbest_embed_ln_bwd_adv(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                           const void* type, const void* ptab, const float* gamma, const float* stats, const float* delta,
                           const void* dout, float* dword, float* dtype_tab, float* dptab, float* dgamma,
                           float* dbeta, int B, int S, int H, int n_types, int dtype, int64_t word_pad_id,
                           int64_t pos_pad_id, int accumulate, int tables_accumulate, float drop_p, uint64_t seed,
                           uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream);
size_t nbest_embed_adv_ws_bytes(int B, int S);
int nbest_embed_adv_delta(const int64_t* ids, const int64_t* seg, const int64_t* pos, const uint8_t* key_mask, const void* word,
                          const void* type, const void* ptab, const float* gamma, const void* dout, float* delta, float* norm,
                          int B, int S, int H, float eps, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                          float epsilon, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* Integrated gradients (new functionality: the reference has no attribution; Sundararajan et al., 2017).
 * Interpolated forward: nbest_embed_ln_fwd with the word row of token m of sequence b = m / S moved along the path from the
 * baseline id base_ids[m] to ids[m] (int64 [B*S] each; alpha fp32 [B], device):
 *   E[m,:] = ((1 - a) word[base_ids[m]] + a word[ids[m]]) + type[seg[m]] + ptab[pos[m]],   a = alpha[b]
 * the lerp in fp32 from the stored table rows (one fma per element), the additions in nbest_embed_ln_fwd's order: a = 1 is
 * bit-for-bit nbest_embed_ln_fwd on ids, a = 0 on base_ids.  Then LayerNorm, dropout and stats as there.  One wave per row.   */
int nbest_embed_ln_fwd_interp(const int64_t* ids, const int64_t* base_ids, const float* alpha, const int64_t* seg, const int64_t* pos,
                              const void* word, const void* type, const void* ptab, const float* gamma, const float* beta, void* out,
                              float* stats, int B, int S, int H, float eps, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                              nbest_stream_t stream);
/* The per-token reduction of integrated gradients.  ids / base_ids / seg / pos / alpha / dhidden are those of an encoder call whose
 * embeddings were interpolated (nbest_embed_ln_fwd_interp, no dropout) and whose backward left dhidden [.][H] (dtype) = the gradient
 * w.r.t. the embedding LayerNorm output (nbest_encoder_backward with no_param_grad).  Pair p owns the m sequences p m .. p m + m - 1
 * of that call, all with the ids of sequence p m; for every token t < S
 *   attr[p S + t] = (1/m) sum_{k = 0..m-1} < LN'(dhidden[(p m + k) S + t]), word[x_t] - word[x'_t] >
 * LN' = the embedding LayerNorm backward at the row E(alpha[p m + k]), recomputed in the kernel: the row from the same lerp and
 * additions as nbest_embed_ln_fwd_interp, its mean and rstd by a restatement of the forward's statistics code, which the compiler
 * may contract differently - equal to the forward's statistics to rounding, not necessarily in every bit.  The sum
 * over k runs in ascending order in fp32; tokens with x = x' (padding included) get exactly 0.  attr fp32 [pairs][S], overwritten.
 * One wave per (pair, token), no LDS, no atomics: bit-reproducible.  Reads m S H esz bytes of dhidden per pair.                   */
int nbest_embed_attrib(const int64_t* ids, const int64_t* base_ids, const float* alpha, const int64_t* seg, const int64_t* pos,
                       const void* word, const void* type, const void* ptab, const float* gamma, const void* dhidden, float* attr,
                       int pairs, int m, int S, int H, float eps, int dtype, nbest_stream_t stream);

/* Sparse exchange of word-embedding gradient rows between data-parallel ranks (new functionality: the reference is single-process,
 * /root/reference/n_best_asr_bert.py:232-294; the table is the nn.Embedding of the installed modeling_bert.py:154-177).  With a
 * 250 002-row vocabulary only the rows of the tokens in a rank's shard are non-zero, so ranks exchange (row ids, row values):
 *   nbest_rows_gather: slot i < n_rows of ids_out / vals_out takes table row rows[i] ([.][H] fp32, H % 4 == 0); slots n_rows .. cap-1
 *                      are padding (id -1, zeros), so every rank sends the same `cap` slots;
 *   nbest_rows_zero:   table[ids[i]][:] = 0;
 *   nbest_rows_add:    table[ids[i]][:] += vals[i][:], ids unique within one call, negative ids skipped; no atomics - called once per
 *                      rank's block in rank order, every replica performs the same additions in the same order.                    */
int nbest_rows_gather(const float* table, const int64_t* rows, int64_t n_rows, int64_t cap, int64_t* ids_out, float* vals_out, int H,
                      nbest_stream_t stream);
int nbest_rows_zero(float* table, const int64_t* ids, int64_t n, int H, nbest_stream_t stream);
int nbest_rows_add(float* table, const int64_t* ids, const float* vals, int64_t n, int H, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2/K4/K6  dense GEMM on MFMA with fused epilogues
 * replaces nn.Linear inside BertSelfAttention / BertSelfOutput / BertIntermediate / BertOutput
 * (installed modeling_bert.py:154-177, 282-293, 325-351) and their autograd backward.
 *   C[M,N] = epi( op(A)[M,K] . op(B)[K,N] )
 *   trans_a = 0: A stored [M][K] (lda)          trans_a = 1: A stored [K][M]
 *   trans_b = 0: B stored [N][K] (torch Linear)  trans_b = 1: B stored [K][N]
 * N must be a multiple of 128, K of 64 unless trans_a (then K is free: token dimension); lda/ldb/ldc
 * multiples of 8 elements; pointers 16-byte aligned.                                                */
enum {
  NBEST_EPI_NONE = 0,          /* C = acc                                                    */
  NBEST_EPI_BIAS = 1,          /* C = acc + bias[n]                                          */
  NBEST_EPI_BIAS_GELU = 2,     /* u = acc + bias[n]; C = gelu_erf(u); U = gelu'(u) (both stored; U = NULL: C only) */
  NBEST_EPI_BIAS_DROP_RES = 3, /* C = drop(acc + bias[n]) + R[m,n]                           */
  NBEST_EPI_DGELU = 4,         /* C = acc * U[m,n]   (U = gelu'(u) saved by BIAS_GELU, see U) */
  NBEST_EPI_RES = 5,           /* C = acc + R[m,n]                                           */
  NBEST_EPI_F32_SPLITK = 6,    /* Cf32[N x ...] = sum over K-splits (weight gradient), fp32  */
  NBEST_EPI_BIAS_GELU_Q8 = 7   /* nbest_gemm_fp8 only: C8 = e4m3(gelu_erf(acc + bias[n]) * s_c), nothing else (inference) */
};
typedef struct nbest_gemm_args {
  const void* A;
  const void* B;
  void* C;            /* dtype output (or fp32 when epilogue == NBEST_EPI_F32_SPLITK)          */
  const float* bias;  /* [N] or NULL                                                          */
  const void* R;      /* residual [M][ldr], dtype                                             */
  void* U;            /* GELU derivative gelu'(u) [M][ldu]: written by BIAS_GELU, read by DGELU.  NBEST_F32: float.
                         NBEST_BF16: ONE BYTE per element, fixed point q = round(200 g') + 26 (step 1/200 over
                         [-0.13, 1.145], 0 and 1 exact), ldu in bytes                                       */
  void* ws;           /* split-K slabs: >= nbest_gemm_ws_bytes(args)                           */
  size_t ws_bytes;
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ldr, ldu;
  int32_t trans_a, trans_b;
  int32_t epilogue;
  int32_t dtype;
  int32_t accumulate; /* F32_SPLITK only: C += result instead of C = result                    */
  float drop_p;
  uint32_t drop_stream;
  uint64_t seed;
  float* colsum_out;        /* optional [N]: column sums of the OUTPUT C (fp32, before rounding) = the bias
                               gradient of the layer that produced A; fused into the epilogue (not for
                               F32_SPLITK).  Needs ws >= nbest_gemm_ws_bytes().                            */
  int32_t colsum_accumulate; /* colsum_out += instead of = */
  int32_t flags;             /* NBEST_GEMM_DEFER_REDUCE: F32_SPLITK leaves the per-split partial slabs in ws
                                (layout [splits][M][N] fp32) and does NOT launch the reduce; C is untouched */
  const void* B_packed;      /* optional (bf16, trans_a = trans_b = 0): the same matrix as B, pre-packed by nbest_pack_weights for tiles of
                                b_pack_bn columns.  Used when the kernel chosen for this shape has that tile width (the LDS-DMA of the B
                                tile becomes a linear copy); otherwise B is read.  Results are identical either way.               */
  int32_t b_pack_bn;         /* 256 | 192 (nbest_pack_bn(N)), 0 = none */
  int32_t pad_;
} nbest_gemm_args;
#define NBEST_GEMM_DEFER_REDUCE 1
size_t nbest_gemm_ws_bytes(const nbest_gemm_args* a);
int nbest_gemm(const nbest_gemm_args* a, nbest_stream_t stream);
/* What nbest_gemm would launch for an argument block, without launching it: the argument checks of nbest_gemm in its order (the same
 * NBEST_ERR_* for the same block, nbest_last_error() set) and then the kernel the dispatcher resolves to.  Host arithmetic on the
 * argument block only - no HIP call, nothing enqueued, no pointer dereferenced (pointers are tested for NULL and alignment, so any
 * aligned non-NULL value serves) - it answers on a machine without a GPU.  The launch path switches on this same result, so a
 * change of the shape heuristics shows here first; tests/test_gemm_plan_cpu.py pins the set the encoder's GEMMs reach.
 *   generation       0: fp32 parity kernel (gemm_f32.hip), 1: 128 x 128 x 64 bf16 (gemm_bf16.hip), 2: the LDS-ring kernels (gemm_bf16_v2.hip)
 *   bm, bn, bk       block tile; bk = the K extent of one stage
 *   wave_rows/_cols  wave grid of a workgroup (64 x rows x cols threads; 0 x 0: generation 0, no MFMA wave grid)
 *   stages           LDS stages of the operand ring
 *   form             NBEST_GEMM_FORM_*: how the operands are stored (NN: trans_a = trans_b = 0, NT: trans_b only, TT: both; TN: fp32 only)
 *   reg_epilogue     1: the epilogue runs on the accumulator registers, 0: restaged through LDS
 *   splits, k_per_split  K-splits of NBEST_EPI_F32_SPLITK (1, K rounded up: none)
 *   b_packed         1: the kernel reads B_packed instead of B
 *   kernel_epilogue  the epilogue the kernel is instantiated with: `epilogue`, or 0x102 for BIAS_GELU with U = NULL                  */
enum { NBEST_GEMM_FORM_NN = 0, NBEST_GEMM_FORM_NT = 1, NBEST_GEMM_FORM_TT = 2, NBEST_GEMM_FORM_TN = 3 };
typedef struct nbest_gemm_plan_info {
  int32_t generation;
  int32_t bm, bn, bk;
  int32_t wave_rows, wave_cols;
  int32_t stages;
  int32_t form;
  int32_t reg_epilogue;
  int32_t splits;
  int64_t k_per_split;
  int32_t b_packed;
  int32_t kernel_epilogue;
} nbest_gemm_plan_info;
int nbest_gemm_plan(const nbest_gemm_args* a, nbest_gemm_plan_info* out);

/* Two weight gradients dW = dY^T . X (bf16 operands, trans_a = trans_b = 1, NBEST_EPI_F32_SPLITK) that share the token dimension K
 * and the column count N, in ONE launch: the 256 x 256 output tiles of `b` are appended to those of `a`, every tile takes the same
 * K-splits and one reduce launch writes both gradients (a->C and b->C; a->ws / a->ws_bytes hold the slabs of both:
 * >= nbest_wgrad_pair_ws_bytes).  Used by nbest_encoder_backward for the QKV ([3H, H]) and attention-output ([H, H]) gradients of
 * a layer - the backward of the two nn.Linear of installed modeling_bert.py:154-177 / 282-293 - whose tile counts (27 + 9) add up to
 * the FFN gradients' (36): the small gradient no longer runs as a launch of 9 tiles x 28 splits of its own.  Results equal
 * nbest_gemm's on each problem up to the fp32 summation order over K-splits.  M1, M2, N multiples of 256, same `accumulate`;
 * nbest_wgrad_pair_ws_bytes returns 0 and nbest_wgrad_pair NBEST_ERR_SHAPE for pairs that do not fit (issue two nbest_gemm).   */
size_t nbest_wgrad_pair_ws_bytes(const nbest_gemm_args* a, const nbest_gemm_args* b);
int nbest_wgrad_pair(const nbest_gemm_args* a, const nbest_gemm_args* b, nbest_stream_t stream);
/* n (1 .. 8) weight gradients dW_i[M_i][N_i] (fp32) (+)= dY_i^T . X_i (bf16 operands, trans_a = trans_b = 1, NBEST_EPI_F32_SPLITK) that share
 * the token dimension K and `accumulate`, in ONE launch WITHOUT K-splits: the 256 x 256 output tiles of all problems are concatenated, one
 * workgroup walks the whole K of one tile and writes (accumulate: adds) it straight into its gradient - no slabs (ws / ws_bytes are not
 * read), no reduce launch.  Each problem has its own pointers and leading dimensions; every M_i, N_i a multiple of 256, else
 * NBEST_ERR_SHAPE and nothing is launched.  It pays when the tiles of the group fill most of the 256 CUs in one round: used by
 * nbest_encoder_backward for the four gradients of TWO bert-base layers (2 x 108 tiles) - the backward of the nn.Linear of installed
 * modeling_bert.py:154-177, 282-293, 325-351.  Each element is one fp32 chain over K in a fixed order: equal to nbest_gemm's result up to
 * the summation order, bit-reproducible run to run.                                                                                    */
int nbest_wgrad_group(const nbest_gemm_args* problems, int n, nbest_stream_t stream);
/* One window of a queue of weight-gradient tiles: the launch of nbest_wgrad_group (the same kernel program, a tile by one workgroup over
 * the whole K in the same order: bit-equal results), but entry i covers only the tiles [tile_first[i], tile_first[i] + tile_count[i]) of
 * problems[i], in the problem's tile order - row-major over its 256 x 256 tiles, a gradient wider than tall (FFN-down) by groups of 3
 * tile columns.  1 .. 16 entries (a 256-tile window touches at most 4 layers' matrices at 108 tiles per layer), at most 256 tiles in
 * all: one round of the 256 CUs.  Tiles outside the ranges are not touched.  Checked on the host before anything is enqueued: every
 * range non-empty and inside its problem, the tile total, K and `accumulate` shared by all entries (NBEST_ERR_ARG), whole tiles
 * (NBEST_ERR_SHAPE).  Used by nbest_encoder_backward in mode NBEST_WGRAD_GROUP_WINDOW, where the launch boundaries fall every 256 pending
 * tiles whichever layers they belong to.                                                                                            */
int nbest_wgrad_window(const nbest_gemm_args* problems, const int32_t* tile_first, const int32_t* tile_count, int n, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * fp8 forward GEMMs (dtype path NBEST "fp8w": BASELINE configs[4], "fp8 weights (CDNA4 fp8 MFMA)")
 * C[M][N] (bf16) = epi((A8[M][K] . W8[N][K]^T) * out_scale + bias): both operands OCP e4m3 (one byte per element, k-contiguous),
 * on the block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales; out_scale = 1 / (per-matrix weight scale).
 * Replaces the same nn.Linear forwards as nbest_gemm (installed modeling_bert.py:154-177, 282-293, 325-351); the
 * weight gradients have their own entry point (nbest_wgrad_fp8 below).  Forward epilogues: NBEST_EPI_BIAS, NBEST_EPI_BIAS_GELU
 * (writes C = gelu bf16, U = gelu' 8-bit, C8 = e4m3 copy of gelu for the next GEMM), NBEST_EPI_BIAS_DROP_RES; dgrad epilogues
 * (B = the TRANSPOSED e4m3 weight copy, A = e4m3 gradient copy): NBEST_EPI_NONE, NBEST_EPI_RES, NBEST_EPI_DGELU.
 * N % 256 == 0, K % 64 == 0.  C may be NULL for BIAS_GELU / DGELU when C8 is given (every reader takes the e4m3 copy).
 * NBEST_EPI_BIAS_GELU_Q8 (forward without a backward: the inference FFN-up): C8[m][n] = e4m3(gelu(acc * out_scale / s_a + bias[n]) * s_c)
 * and nothing else - no gelu' arithmetic, no U rows, no bf16 C, no amax record.  The value that is rounded is the fp32 gelu BIAS_GELU
 * rounds, so the C8 bytes are those BIAS_GELU writes for the same inputs; same plan (nbest_gemm_fp8_plan) as BIAS_GELU for the same
 * shape.  Refused (NBEST_ERR_ARG, nothing enqueued): C8 == NULL, bias == NULL, a non-NULL C, U or c8_amax_new.                   */
typedef struct nbest_gemm_fp8_args {
  const void* A;      /* e4m3 [M][lda] */
  const void* B;      /* e4m3 [N][ldb] (the weight matrix as stored, [out][in]) */
  void* C;            /* bf16 [M][ldc] */
  const float* bias;  /* [N] */
  const void* R;      /* bf16 residual [M][ldr] (BIAS_DROP_RES) */
  void* U;            /* 8-bit gelu' [M][ldu] (BIAS_GELU), format of nbest_gemm_args::U */
  void* C8;           /* e4m3 copy of C [M][ldc8] (BIAS_GELU) */
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ldr, ldu, ldc8;
  int32_t epilogue;
  float out_scale;
  float drop_p;
  uint32_t drop_stream;
  uint64_t seed;
  const float* out_scale_dev; /* optional DEVICE scalar that overrides out_scale (scales produced on the device by
                                 nbest_quantize_weights_fp8: no host round trip) */
  /* ---- scaled A operand (every epilogue): A8 = e4m3(a * s) with s = 2^floor(log2(T / amax)) of the amax stored (as float
   * bits) at a_amax - the DELAYED per-tensor scale its producer used: a gradient tensor (dgrad epilogues NONE, RES, DGELU:
   * T = 56, 8 x headroom) or, round 4, a forward activation (BIAS, BIAS_GELU, BIAS_DROP_RES: T = 224, 2 x headroom); the
   * accumulator is divided by s.  NULL = unit scale.
   * DGELU: C = acc * gelu'(U) in bf16; optional C8 = e4m3(C * s_c), s_c from *c8_amax_prev; max(|C|) recorded into the slot block c8_amax_new
   * (NBEST_AMAX_TENSOR_WORDS words, see nbest_fp8_amax_fold);
   * optional colsum_out[N] (+)= column sums of C (the FFN-up bias gradient), needs ws >= nbest_gemm_fp8_ws_bytes().
   * BIAS_GELU: C8 = e4m3(gelu * s_c) with the same two fields (the activation scale of the FFN-down GEMM's input).          */
  const uint32_t* a_amax;
  const uint32_t* c8_amax_prev;
  uint32_t* c8_amax_new;
  float* colsum_out;
  int32_t colsum_accumulate;
  int32_t pad;
  void* ws;
  size_t ws_bytes;
  const void* B_packed; /* optional: B pre-packed by nbest_pack_weights_fp8 for tiles of b_pack_bn columns (256 | 128); used when the kernel
                           chosen for the shape has that tile width, otherwise B is read.  Identical results.                        */
  int32_t b_pack_bn;
  int32_t pad3;
} nbest_gemm_fp8_args;
size_t nbest_gemm_fp8_ws_bytes(const nbest_gemm_fp8_args* a);
int nbest_gemm_fp8(const nbest_gemm_fp8_args* a, nbest_stream_t stream);
/* DGELU writes the e4m3 copy only where it records: C8 without c8_amax_new is refused (NBEST_ERR_ARG, nothing enqueued), as
 * nbest_layernorm_bwd_fp8 refuses out8 without amax_new.
 * What nbest_gemm_fp8 would launch for an argument block (the fp8 counterpart of nbest_gemm_plan): computed from the block alone - no
 * HIP call, nothing enqueued, no pointer dereferenced - and every refusal of nbest_gemm_fp8 with the same code and message.  The launch
 * takes its decisions from this result, nbest_pack_bn_fp8 from the same tile rule.
 *   bn, stages      256-row tiles of bn = 128 columns on a 3-stage ring or of bn = 256 columns on the 4-stage ping-pong ring
 *   tiles_m/_n      the tile grid (tiles_m = ceil(M / 256))
 *   group_cols      tile columns per L2 group: tiles run group by group, row-major inside a group of group_cols columns
 *   packed_taken    1: the kernel reads B_packed instead of B (b_pack_bn == bn, ldb == K, 16-byte aligned)                          */
typedef struct nbest_gemm_fp8_plan_info {
  int32_t bn, stages;
  int32_t tiles_m, tiles_n;
  int32_t group_cols;
  int32_t packed_taken;
} nbest_gemm_fp8_plan_info;
int nbest_gemm_fp8_plan(const nbest_gemm_fp8_args* a, nbest_gemm_fp8_plan_info* out);
/* fp8 weight gradient: dW[M][N] (fp32) (+)= sum over K tokens of dY8[k][m] * X8[k][n] / s, both operands TOKEN-major e4m3
 * ([K][lda] / [K][ldb], as their producers wrote them: the reduction dimension is read through transposed LDS reads),
 * s = the gradient scale of dY8 (from the float bits at a_amax, NULL = 1) times the activation scale of X8 (x_amax, NULL = 1).
 * M, N multiples of 256; split-K over tokens into ws (>= nbest_wgrad_fp8_ws_bytes) + deterministic reduce.  Replaces the
 * weight-gradient half of the nn.Linear backward. */
size_t nbest_wgrad_fp8_ws_bytes(int64_t M, int64_t N, int64_t K);
/* the K-split the weight gradient (a pair: M = Ma + Mb, the virtual row count) runs with: split z covers the tokens
 * [z k_per_split, min(K, (z + 1) k_per_split)); splits == 1: written directly, no workspace.  Host arithmetic only; refuses
 * (NBEST_ERR_ARG / NBEST_ERR_SHAPE) the shapes nbest_wgrad_fp8 refuses.  The workspace queries and the launches use this result. */
int nbest_wgrad_fp8_plan(int64_t M, int64_t N, int64_t K, int* splits, int64_t* k_per_split);
int nbest_wgrad_fp8(const void* dY8, const void* X8, float* dW, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                    int64_t ldc, const uint32_t* a_amax, const uint32_t* x_amax, int accumulate, void* ws, size_t ws_bytes,
                    nbest_stream_t stream);
/* Two fp8 weight gradients with the same token dimension K and column count N in ONE launch (the e4m3 counterpart of nbest_wgrad_pair;
 * nbest_encoder_backward pairs the Q|K|V and attention-output gradients of a layer): problem b's 256 x 256 output tiles are appended below
 * problem a's, each keeps its own gradient scale (amax_a / amax_b), one reduce writes dWa and dWb.  Ma, Mb, N multiples of 256; ws >=
 * nbest_wgrad_fp8_pair_ws_bytes (0 = the pair does not fit: issue two nbest_wgrad_fp8).                                                */
size_t nbest_wgrad_fp8_pair_ws_bytes(int64_t Ma, int64_t Mb, int64_t N, int64_t K);
int nbest_wgrad_fp8_pair(const void* dY8a, const void* X8a, float* dWa, int64_t Ma, int64_t lda_a, int64_t ldb_a, int64_t ldc_a,
                         const uint32_t* amax_a, const uint32_t* xamax_a, const void* dY8b, const void* X8b, float* dWb, int64_t Mb,
                         int64_t lda_b, int64_t ldb_b, int64_t ldc_b, const uint32_t* amax_b, const uint32_t* xamax_b, int64_t N, int64_t K,
                         int accumulate, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* bf16 [n] -> e4m3 [n], unit scale, saturating at +-448 (activations that feed an fp8 GEMM); n % 8 == 0 */
int nbest_cast_bf16_to_fp8(const void* src, void* dst, int64_t n, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K3  scaled-dot-product attention with a per-sample key-padding mask
 * replaces eager_attention_forward (installed modeling_bert.py:111-136); mask rule of
 * /root/reference/models/model.py:43 is applied by the CALLER (key_mask = ids > 0, uint8 [B,S]).
 *   qkv [M][3H] (Q | K | V, head h = columns h*d .. h*d+d of each third), ctx [M][H],
 *   lse [B][heads][S] = log-sum-exp of the scaled masked scores (saved for backward).
 *   P = softmax(Q K^T / sqrt(d) + (mask ? 0 : -inf)) ; ctx = drop(P) V.  d must be 64; S <= 512
 *   (bf16: S <= 256).                                                                              */
int nbest_attention_fwd(const void* qkv, const uint8_t* key_mask, void* ctx, float* lse, int B, int S,
                        int heads, int d, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                        nbest_stream_t stream);
/* CLS-query forward (inference): for every (utterance b, head h) ONE query row, q[b * ldq + h d ..], against the S keys and values
 * of the utterance, kv[(b S + j) * ldkv + h d ..] (K) and kv[(b S + j) * ldkv + H + h d ..] (V); writes ctx[b * ldctx + h d ..].
 * The semantics of row 0 of nbest_attention_fwd (same scale and key_mask rule), no dropout, no LSE.  d = 64, 1 <= S <= 512, fp32
 * or bf16; ldq, ldkv multiples of 16 bytes, q and kv 16-byte aligned.  (nbest_attention_fwd's row 0: q = qkv, ldq = 3 H S,
 * kv = qkv + H, ldkv = 3 H.)                                                                                                   */
int nbest_attention_cls_fwd(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const uint8_t* key_mask, void* ctx,
                            int64_t ldctx, int B, int S, int heads, int d, int dtype, nbest_stream_t stream);
/* Attention probabilities (an eval / predict output; the forward kernels keep P in registers).  From what the forward stashed,
 * qkv [M][3H] (layout, scale and key_mask rule of nbest_attention_fwd) and its lse [B][heads][S] (natural-log units):
 *   probs[b][h][i][j] = exp(scale q_i . k_j - lse[b][h][i]) for key_mask[b][j] != 0, exactly 0 for masked keys; fp32
 *   [B][heads][S][S], every element written.  A row with no unmasked key is all 0 in both dtypes (the bf16 forward gives NaN ctx
 *   there).  No dropout: the pre-dropout probabilities.  d = 64, 1 <= S <= 512; qkv 16-byte aligned.  bf16: Q K^T on the
 *   16x16x32 bf16 MFMA with fp32 accumulation; fp32: one sequential fma chain over d per score, as the fp32 forward.  Bit-
 *   reproducible (no atomics).  Writes S^2 x 4 bytes per (utterance, head).                                                  */
int nbest_attention_probs(const void* qkv, const uint8_t* key_mask, const float* lse, float* probs, int B, int S, int heads, int d,
                          int dtype, nbest_stream_t stream);
/* The CLS row of it (inference): arguments, strides and semantics of nbest_attention_cls_fwd, no LSE - the row is normalised with
 * the scores, max and sum that kernel computes - and no P.V.  Writes fp32 probs[(b heads + h) ldp + j], j < S (ldp >= S); masked
 * keys 0, a fully masked row all 0; unrounded in both dtypes.                                                                 */
int nbest_attention_cls_probs(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const uint8_t* key_mask, float* probs,
                              int64_t ldp, int B, int S, int heads, int d, int dtype, nbest_stream_t stream);
/* One step of the attention rollout (Abnar & Zuidema, 2020): a row vector through residual I + (1 - residual) mean_h P_h, with P
 * the probabilities of nbest_attention_probs (qkv, key_mask and lse as there: same scale, same mask rule, natural-log lse):
 *   r_out[b][j] = residual r_in[b][j] + (1 - residual) / heads * sum_h sum_i r_in[b][i] P[b][h][i][j]
 * r_in, r_out fp32 [B][S], different buffers.  No map is written: the probabilities are recomputed tile by tile (bf16: K Q^T on
 * the 16x16x32 bf16 MFMA with fp32 accumulation; fp32: one sequential fma chain over d per score - the bits of
 * nbest_attention_probs) and summed in fp32; traffic is the Q and K thirds of qkv, lse and the two vectors.  A query row with
 * lse = -inf (no unmasked key) contributes 0.  Exact where nothing else contributes: r_out = residual r_in on masked keys, and
 * r_out == r_in bit for bit at residual = 1.  Every r_out element is written exactly once; no atomics, bit-reproducible.
 * d = 64, 1 <= S <= 512, fp32 or bf16, 0 <= residual <= 1; qkv 16-byte aligned.  Refused before anything is enqueued:
 * NBEST_ERR_ARG (a null pointer, r_in == r_out, residual outside [0, 1] or not finite), NBEST_ERR_SHAPE, NBEST_ERR_DTYPE,
 * NBEST_ERR_ALIGN.                                                                                                        */
int nbest_attention_rollout_step(const void* qkv, const uint8_t* key_mask, const float* lse, const float* r_in, float* r_out,
                                 float residual, int B, int S, int heads, int d, int dtype, nbest_stream_t stream);
/* dqkv [M][3H] receives dQ | dK | dV (overwritten, no accumulation).  dbias != NULL: dbias[3H] (+)= column
 * sums of dqkv (the Q|K|V bias gradient), fused into the kernel; ws >= nbest_attention_bwd_ws_bytes().   */
size_t nbest_attention_bwd_ws_bytes(int B, int S, int heads);
int nbest_attention_bwd(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx,
                        const float* lse, void* dqkv, float* dbias, int accumulate, void* ws, size_t ws_bytes,
                        int B, int S, int heads, int d, int dtype, float drop_p, uint64_t seed,
                        uint32_t drop_stream, nbest_stream_t stream);

/* The same pair with the dropout decisions handed from the forward to the backward (bf16, S <= 256): the forward writes its
 * keep decisions as bit words keep[B * heads][ceil(S/32)][32 ceil(S/32)] (bit j of word (key block kb, query q) = key 32 kb + j
 * kept; nbest_attention_keep_bytes() bytes, 0 when the shape has no such path), the backward reads them instead of hashing
 * every score element again.  Same decisions, hence the same results as the plain pair up to fma contraction in the last bit;
 * keep may be NULL (then identical to the plain pair). */
size_t nbest_attention_keep_bytes(int B, int S, int heads);
int nbest_attention_fwd_keep(const void* qkv, const uint8_t* key_mask, void* ctx, float* lse, int B, int S,
                             int heads, int d, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream,
                             void* keep, nbest_stream_t stream);
int nbest_attention_bwd_keep(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx,
                             const float* lse, void* dqkv, float* dbias, int accumulate, void* ws, size_t ws_bytes,
                             int B, int S, int heads, int d, int dtype, float drop_p, uint64_t seed,
                             uint32_t drop_stream, const void* keep, nbest_stream_t stream);

/* Head gates (HF's head_mask: BertModel.forward(head_mask=), installed modeling_bert.py, where the post-dropout probabilities of
 * head h are multiplied by the mask; Michel et al., 2019): a factor gate[h] (fp32 [heads], device; any float: 0 prunes, 1 is the
 * identity) on head h's slice of the attention context, applied between the attention kernel and the attention-output GEMM -
 * ctx_h = (gate[h] P_h) V_h = gate[h] (P_h V_h).  d = 64, fp32 or bf16, 16-byte accesses, no atomics, bit-reproducible.
 *   nbest_head_gate_fwd: out[m][h d + k] = T(gate[h] * float(in[m][h d + k])) for the M rows (row strides ld_in, ld_out >= H =
 *     heads d, in elements, multiples of 16 bytes; both pointers 16-byte aligned).  In place (ctx_out == ctx_in, ld_out == ld_in)
 *     is allowed.  A gate of 1 leaves the bits as they are, a gate of 0 gives zeros.  Reads and writes [M][H] once.
 *   nbest_head_gate_bwd: ctx [B S][H] = the UN-gated context the forward stashed, dctx [B S][H] = the gradient w.r.t. the gated
 *     context.  One workgroup per (utterance, head): dgate[b][h] = sum_{s,k} float(ctx[b,s,h,k]) * float(dctx[b,s,h,k]) (fp32
 *     [B][heads], OVERWRITTEN; fp32 accumulation in a fixed order) = d loss / d gate[h] restricted to utterance b; then
 *     dctx <- T(gate[h] * dctx) in place = the gradient w.r.t. the un-gated context, which nbest_attention_bwd takes together with
 *     the un-gated ctx (its delta = rowsum(O * dO) is then exact for every gate value, 0 included).  The store is skipped for
 *     gate[h] == 1: an all-ones gate leaves dctx bit-identical.  dgate == NULL: scale only (ctx is not read and may be NULL).
 *     Reads [M][H] twice, writes it once.                                                                                       */
int nbest_head_gate_fwd(const void* ctx_in, int64_t ld_in, void* ctx_out, int64_t ld_out, const float* gate, int64_t M, int heads,
                        int d, int dtype, nbest_stream_t stream);
int nbest_head_gate_bwd(const void* ctx, void* dctx, const float* gate, float* dgate, int B, int S, int heads, int d, int dtype,
                        nbest_stream_t stream);

/* Compact pruned heads (inference): a layer that keeps k of its heads, idx[0..k) ascending, is an ordinary layer with a [3 64k][H]
 * QKV matrix, heads = k in the attention and an [H][64k] attention-output matrix.  The compact images of all layers, H = 64 heads:
 *   weight image (compute dtype T), two sections - the Wqkv' of every layer, then the Wo' of every layer:
 *     Wqkv' [3 64k][H]: row (t k + i) 64 + r is a bit copy of row (t heads + idx[i]) 64 + r of the layer's [3H][H] matrix, t in {Q, K, V}
 *     Wo'   [H][64k]:   element [n][i 64 + r] = T(gate[l][idx[i]] * float(Wo[n][idx[i] 64 + r])) - the gate is folded into the output
 *                       matrix (any float works); a gate of exactly 1 copies the bits
 *   bias image (fp32): bqkv' [3 64k], the mapping of Wqkv' out of the fp32 arena.
 * nbest_head_prune_layer: one layer's row of the table - element offsets of its three tensors in the arenas (src_*, as
 *   nbest_layer_offsets) and in the images (dst_*), k and the indices.
 * nbest_head_prune_plan (host arithmetic only, answers without a GPU): for the kept counts k[L] (1 <= k[l] <= heads <=
 *   NBEST_HEAD_PRUNE_MAX_HEADS) fills layers[l].k and layers[l].dst_* - tensors packed back to back, every offset a multiple of 64
 *   elements - and the byte sizes of the two weight sections and of the bias image (each pointer may be NULL).  Leaves src_* and idx
 *   alone.  dst_wo counts from the start of the weight image: the Wo' section begins at byte *wqkv_bytes.
 * nbest_head_prune_pack: ONE launch over all layers that gathers the images from wts (T) / prm (fp32) under gate [L][heads] fp32
 *   (device).  table_host and table_dev hold the same L rows (the host copy is checked: 1 <= k <= heads, idx ascending and
 *   < heads, every destination inside w_bytes / b_bytes, 16-byte alignment; the device copy is what the kernel reads).  A layer
 *   with no kept head is packed by its caller as k = 1, idx = {0}: Wo' comes out all zeros through the gate.  16-byte accesses, no
 *   atomics, bit-reproducible; writes exactly the planned bytes.  Reads and writes 4 H 64k (+ 3 64k biases) elements per layer.    */
#define NBEST_HEAD_PRUNE_MAX_HEADS 32
typedef struct nbest_head_prune_layer {
  int64_t src_wqkv, src_bqkv, src_wo;
  int64_t dst_wqkv, dst_bqkv, dst_wo;
  int32_t k, pad;
  int32_t idx[NBEST_HEAD_PRUNE_MAX_HEADS];
} nbest_head_prune_layer;
int nbest_head_prune_plan(const int32_t* k, int L, int heads, int dtype, nbest_head_prune_layer* layers, size_t* wqkv_bytes,
                          size_t* wo_bytes, size_t* bqkv_bytes);
int nbest_head_prune_pack(const void* wts, const float* prm, const float* gate, const nbest_head_prune_layer* table_host,
                          const nbest_head_prune_layer* table_dev, int L, int heads, int dtype, void* w_out, size_t w_bytes,
                          float* b_out, size_t b_bytes, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K5  LayerNorm over the hidden dimension (BertSelfOutput / BertOutput LayerNorm,
 * installed modeling_bert.py:282-293, 340-351).  stats[m] = {mean, rstd} fp32.                      */
int nbest_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats,
                        int64_t M, int H, float eps, int dtype, nbest_stream_t stream);
/* dx = LN'(dy); dgamma = sum_m dy*xhat; dbeta = sum_m dy (+= when accumulate).
 * dgamma, dbeta and dbias all NULL: dx (and dx_drop) only - no column sums, no workspace (ws may be NULL).
 * The LayerNorm input was x = drop(dense_out) + residual, so two gradients leave this kernel:
 *   dx      - gradient of the residual branch (unmasked), and
 *   dx_drop - gradient of dense_out = dropout mask (regenerated from seed/drop_stream) applied to dx;
 *             only written when drop_p > 0 (otherwise the caller uses dx for both; dx_drop may be NULL).
 * dbias != NULL: dbias = sum_m dx_drop (gradient of the dense layer's bias).
 * ws: >= nbest_rowred_ws_bytes(M, H).                                                               */
int nbest_layernorm_bwd(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                        void* dx_drop, float* dgamma, float* dbeta, float* dbias, int64_t M, int H, int dtype,
                        int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws,
                        size_t ws_bytes, nbest_stream_t stream);
size_t nbest_rowred_ws_bytes(int64_t M, int64_t N);
/* out[n] (+)= sum_m X[m][n]   (bias gradients).  ws: >= nbest_rowred_ws_bytes(M, N).               */
int nbest_colsum(const void* X, float* out, int64_t M, int64_t N, int64_t ld, int dtype, int accumulate,
                 void* ws, size_t ws_bytes, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K7  STC heads + losses, forward and analytic backward in one call
 * replaces HierarchicalClassifier.forward (/root/reference/models/modules/hierarchical_classifier.py:35-60),
 * cal_total_loss / cal_ce_loss (/root/reference/n_best_asr_bert.py:145-195), convert_labels and
 * onehot_to_scalar (/root/reference/utils/STC_util.py:4-7,29-51).
 * Label space: n_top top labels; bottom_of[...] lists, for top t, its bottom ids
 * bottom_ids[bottom_off[t] .. bottom_off[t+1]); tops with >= 2 bottoms own a softmax head whose rows
 * in the concatenated head matrix Wh [R][H] start at head_row[t] (single-bottom tops: -1); rows
 * 0..n_top-1 of Wh are the top (sigmoid) classifier.  R = n_top + sum of multi-value head sizes.
 *   cls     = hidden[b * cls_stride .. +H]  (raw CLS row, models/model.py:46-47), dtype
 *   top     [B][n_top], bott [B][R - n_top] (softmax heads concatenated in head order), final [B][n_bottom]
 *   loss_parts[4] = {BCE_sum(final,y), BCE_sum(top, y.B2T), mean_k NLL_sum_k, 0}  (fp32, overwritten)
 *   dcls [B][H] fp32 = d(sum of the three)/d cls ; dWh [R][H], dbh [R] fp32 (overwritten unless accumulate)
 * feature dropout: an independent mask per linear layer (hierarchical_classifier.py:41,46).
 * ws: >= nbest_heads_ws_bytes(B, R, H).                                                             */
typedef struct nbest_label_space {
  int32_t n_top, n_bottom, n_rows;
  const int32_t* bottom_off; /* [n_top+1] device */
  const int32_t* bottom_ids; /* [n_bottom] device */
  const int32_t* head_row;   /* [n_top] device   */
} nbest_label_space;
size_t nbest_heads_ws_bytes(int B, int R, int H);
int nbest_stc_heads(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                    const nbest_label_space* ls, const float* labels, float* top, float* bott, float* final_scores,
                    float* loss_parts, float* dcls, float* dWh, float* dbh, int B, int H, int dtype,
                    int need_grad, int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws,
                    size_t ws_bytes, nbest_stream_t stream);
/* K7 kd  knowledge distillation: nbest_stc_heads with a teacher's fp32 probabilities as a second set of targets, in the layout of
 * top / bott / final: t_top [B][n_top], t_bott [B][R - n_top], t_final [B][n_bottom] (another model's scores for the same
 * utterances).  The soft loss is the three terms above with the teacher's outputs in place of the labels:
 *   BCE_sum(final, t_final) + BCE_sum(top, t_top) + mean_k sum_j -t_bott_kj log(s_kj + 1e-12)      (no temperature)
 *   loss_parts[4] = {the three hard terms as nbest_stc_heads gives them, the soft loss}, all unscaled
 *   d(logits) = (1 - alpha) d_hard + alpha d_soft, so dcls / dWh / dbh are the gradients of (1 - alpha) hard + alpha soft
 * Same two launches, same workspace, same dropout bits as nbest_stc_heads; fixed-order sums.  0 <= alpha <= 1; the teacher
 * arrays may be null (all three) only when alpha == 0, which then is nbest_stc_heads itself (loss_parts[3] = 0).             */
int nbest_stc_heads_kd(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                       const nbest_label_space* ls, const float* labels, const float* t_top, const float* t_bott,
                       const float* t_final, float alpha, float* top, float* bott, float* final_scores, float* loss_parts,
                       float* dcls, float* dWh, float* dbh, int B, int H, int dtype, int need_grad, int accumulate,
                       float drop_p, uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* K7 kd_t  distillation at a temperature: the teacher is given by its LOGITS t_logits [B][R] (fp32, the layout of Wh's rows: what
 * nbest_stc_heads_logits returns for the teacher) and both models are softened by 1 / T (Hinton et al., 2015).  With u = z / T:
 *   p_T = sigmoid(u_t) ; s_T = softmax over a head's columns of u ; f_T = p_T * s_T  (f_T = p_T for a single-bottom top)
 *   soft_T = T^2 * [ BCE_sum(f_T^student, f_T^teacher) + BCE_sum(p_T^student, p_T^teacher)
 *                    + (1 / n_heads) sum_k sum_j -s_T^teacher_kj log(s_T^student_kj + 1e-12) ]
 * with the -100 clamps on the logs and the 1e-12 guards of K7 kd, on the tempered values; the teacher's tempered scores are
 * formed inside the kernel.  top / bott / final and loss_parts[0..2] are the T = 1 quantities of nbest_stc_heads;
 *   loss_parts[3] = soft_T (T^2 included) ; d(logits) = (1 - alpha) d_hard + alpha d_soft_T, d_soft_T = d(soft_T)/d(student logits)
 * (the K7 kd expressions on the tempered scores, times T).  Same two launches, workspace and dropout bits as nbest_stc_heads;
 * fixed-order sums.  0 <= alpha <= 1, temperature finite and > 0; t_logits may be null only when alpha == 0, which then is
 * nbest_stc_heads itself (loss_parts[3] = 0).                                                                                  */
int nbest_stc_heads_kd_t(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                         const nbest_label_space* ls, const float* labels, const float* t_logits, float alpha,
                         float temperature, float* top, float* bott, float* final_scores, float* loss_parts, float* dcls,
                         float* dWh, float* dbh, int B, int H, int dtype, int need_grad, int accumulate, float drop_p,
                         uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* K7 rdrop  R-Drop (Liang et al., 2021): the batch has B2 = 2 P rows, rows b and b' = b + P (0 <= b < P) are twins - one utterance
 * under two sets of dropout bits (the hashes are keyed on the position in the batch, so the twins' masks are independent).  With z, z'
 * the twins' head logits, p = sigmoid(z_t) the top scores and s = softmax over a multi-bottom head's columns, the pair's consistency
 * term is the symmetric KL of the model's own factorisation (n_top Bernoullis + one categorical per head, averaged over n_heads as CE):
 *   R(b, b') = sum_t 1/2 (p_t - p'_t)(z_t - z'_t) + (1 / n_heads) sum_k 1/2 sum_j (s_kj - s'_kj)(z_kj - z'_kj)
 *            = 1/2 [KL(P || P') + KL(P' || P)]     (no logarithm, no clamp, no 1e-12; no term on final)
 * and its gradient w.r.t. a row's own logits
 *   top t:            1/2 [ p_t (1 - p_t)(z_t - z'_t) + (p_t - p'_t) ]
 *   head k, column i: (1 / n_heads) 1/2 [ (s_i - s'_i) + s_i ( (z_i - z'_i) - sum_j s_j (z_j - z'_j) ) ].
 * Optimised: sum over the 2 P rows of the hard loss + alpha * sum over the P pairs of R, so
 *   top / bott / final, loss_parts[0..2] : those of nbest_stc_heads on the B2 rows, bit for bit
 *   loss_parts[3] = sum over the pairs of R (unscaled by alpha; each row of a pair contributes R / 2)
 *   d(logits) = d_hard + alpha * dR/d(own logits)      (alpha = 0: the bits of nbest_stc_heads; equal twins, dropout off: dR = 0 exactly)
 * The block of row b forms its twin's logits itself (the twin's CLS row and mask words in LDS, the arithmetic and order of its own), so
 * no grid-wide synchronisation, the same two launches, workspace and dropout bits as nbest_stc_heads; fixed-order sums.
 * alpha finite and >= 0; B2 even.  The trailing arguments are those of nbest_stc_heads.                                             */
int nbest_stc_heads_rdrop(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                          const nbest_label_space* ls, const float* labels, float alpha, float* top, float* bott,
                          float* final_scores, float* loss_parts, float* dcls, float* dWh, float* dbh, int B2, int H, int dtype,
                          int need_grad, int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws,
                          size_t ws_bytes, nbest_stream_t stream);
/* K7 logits  the logits of the heads, an inference quantity (no dropout):
 *   logits[b][r] = bh[r] + sum_h Wh[r][h] * float(hidden[b * cls_stride + h])      fp32 [B][R], r in the order of Wh's rows
 * in the arithmetic of nbest_stc_heads's logits stage (a wave per row, lanes strided over h, fma, fixed-order wave sum, + bh), so
 * these are the numbers its scores are made from at dropout 0.  hidden fp32 or bf16.  One launch, no workspace, no atomics.     */
int nbest_stc_heads_logits(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                           const nbest_label_space* ls, float* logits, int B, int H, int dtype, nbest_stream_t stream);
/* Backward of the heads for ARBITRARY upstream gradients dtop [B][n_top], dbott [B][R - n_top], dfin [B][n_bottom] (fp32) - what
 * torch autograd hands to the heads when the reference's loop calls total_loss.backward() on a loss it built itself
 * (/root/reference/n_best_asr_bert.py:255-264; nbest_amd.model's autograd bridge).  `ws` must be the workspace of the
 * nbest_stc_heads call (need_grad = 0 is enough) that produced top / bott for the same inputs and dropout seed: it holds the fp32
 * CLS rows and the dropout bits.  dcls [B][H] overwritten; dWh / dbh overwritten unless accumulate.                                */
int nbest_stc_heads_vjp(const float* Wh, const nbest_label_space* ls, const float* top, const float* bott, const float* dtop,
                        const float* dbott, const float* dfin, float* dcls, float* dWh, float* dbh, int B, int H, int accumulate,
                        float drop_p, uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream);

/* K8  pooled-CLS MSE auxiliary loss (--add_l2_loss): nn.MSELoss() between the ASR and transcript CLS
 * rows, /root/reference/n_best_asr_bert.py:166-170,574.  loss[0] = mean((a-t)^2);
 * da += grad_scale * 2(a-t)/(B*H); dt = -grad_scale * 2(a-t)/(B*H)  (the transcript branch is NOT detached). */
int nbest_cls_mse(const void* hidden_a, int64_t stride_a, const void* hidden_t, int64_t stride_t, float* loss,
                  float* da, float* dt, int B, int H, int dtype, float grad_scale, nbest_stream_t stream);
/* K8c  in-batch contrastive loss between the ASR and the transcript CLS rows (--contrastive_weight; the symmetric InfoNCE of SimCSE /
 * CLIP; Chang & Chen, Interspeech 2022 for ASR-robust SLU).  a_i / t_i: the rows nbest_cls_mse reads (raw CLS, any row stride, fp32
 * or bf16), k_i an int64 key, W = weight, T = temperature:
 *   u_i = a_i / max(||a_i||, 1e-12)     v_i = t_i / max(||t_i||, 1e-12)          (fp32; torch's F.normalize)
 *   Z_ij = <u_i, v_j> / T               keep(i, j) = (i == j) or (k_i != k_j)     (key NULL: every pair kept)
 *   lr_i = log sum_{j: keep} exp(Z_ij)  lc_j = log sum_{i: keep} exp(Z_ij)
 *   L    = 1/2 sum_i [ (lr_i - Z_ii) + (lc_i - Z_ii) ]                            (a SUM over the batch, as the BCE / CE terms)
 *   G_ij = (W / 2T) [ keep(i, j) (exp(Z_ij - lr_i) + exp(Z_ij - lc_j)) - 2 [i == j] ]
 *   du_i = sum_j G_ij v_j               dv_j = sum_i G_ij u_i
 *   da_i = (du_i - <du_i, u_i> u_i) / ||a_i||      dt_j = (dv_j - <dv_j, v_j> v_j) / ||t_j||
 * Rows with an equal key (utterances whose transcripts are identical) stay out of each other's denominators; B = 1 or all keys
 * equal give L = 0 and zero gradients exactly.
 *   out[0] = L (unweighted)   out[1] = number of rows i whose own column is the first maximum of Z_i. over the kept columns
 *   out[2] = B                out[3] = 0                                           (fp32 [4], overwritten)
 *   da [B][H] += W dL/da (the dcls the heads call wrote, as for nbest_cls_mse); dt [B][H] overwritten, or added to when
 *   accumulate_dt (the MSE wrote it first); either may be NULL, both NULL = loss only.  The transcript branch is NOT detached.
 * fp32 on the vector units throughout: the unit vectors are never rounded to bf16 (at T = 0.05 one bf16 ulp of a cosine is 0.08 in
 * a logit).  Z is formed once in `ws`, so both softmaxes read the same bits.  Four launches, no atomics, no workgroup waits for
 * another, fixed-order sums: identical bits run to run.  `ws` (16-byte aligned, nbest_cls_contrast_ws_bytes) is written before it is
 * read - its contents on entry do not matter.  Checked before the first launch: null hidden_* / out / ws, B <= 0, H <= 0,
 * B > 4096, temperature not finite or <= 0, weight not finite or < 0 -> NBEST_ERR_ARG; H > 8192 -> NBEST_ERR_SHAPE; a short ws ->
 * NBEST_ERR_WORKSPACE; a bad dtype -> NBEST_ERR_DTYPE.                                                                            */
size_t nbest_cls_contrast_ws_bytes(int B, int H);
int nbest_cls_contrast(const void* hidden_a, int64_t stride_a, const void* hidden_t, int64_t stride_t, const int64_t* key,
                       float weight, float temperature, float* out, float* da, float* dt, int accumulate_dt, int B, int H,
                       int dtype, void* ws, size_t ws_bytes, nbest_stream_t stream);

/* scatter a [B][H] fp32 CLS gradient into row 0 of every sequence of dhidden [B*S][H] (all other
 * rows zero): the backward of sequence_output[:, 0, :].                                             */
int nbest_cls_grad_scatter(const float* dcls, void* dhidden, int B, int S, int H, int dtype,
                           nbest_stream_t stream);

/* K10 device decode of pred_one_sample (/root/reference/n_best_asr_bert.py:198-215):
 * pred[b][t] = predicted bottom label index when top[b][t] > 0.5 (strict), else -1; for a
 * multi-value top the argmax of its head (first maximum), -1 when none_flag[that bottom] != 0.      */
int nbest_stc_decode(const float* top, const float* bott, const nbest_label_space* ls,
                     const uint8_t* none_flag, int32_t* pred, int B, nbest_stream_t stream);
/* `pred` may be any device-ACCESSIBLE memory - in particular mapped pinned host memory (hipHostMalloc): the rows then land on the
 * host without a copy command.  nbest_stream_stamp writes `value` to *flag (device-accessible, system-scope release) in stream order:
 * stamped after a decode into host memory it tells a polling host thread that the rows are complete - the per-step prediction
 * hand-off of the reference's loop (n_best_asr_bert.py:283-288) without a hipMemcpy, an event or a stream synchronisation. */
int nbest_stream_stamp(int32_t* flag, int32_t value, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K9  multi-tensor BertAdam over flat arenas
 * replaces BertAdam.step (/root/reference/models/optimization.py:237-302) with the per-parameter
 * grouping of the reference's n_best_asr_bert.py:540-561: per tensor c = min(1, max_grad_norm/(||g||+1e-6))
 * (1 if max_grad_norm <= 0), g' = c g; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; u = m/(sqrt(v)+eps)
 * [+ wd p if wd > 0]; p -= lr*lr_mult * u, lr_mult = warmup-linear schedule value for this step
 * (optimization.py:162-171; one scalar: every tensor that receives gradients shares the same step count).
 * The clipped gradient g' lives in registers only: the arena g is READ, never written (the reference
 * scales p.grad in place; nothing reads it between the step and the next zero_grad).  b1 and b2 are
 * doubles: the kernels use (float)b and (float)(1 - b), the values torch's kernels receive from the
 * reference's Python floats (1.f - 0.999f would be 1.29e-5 below 0.001f).
 * The arenas p, g, m, v are fp32; tensors are described by device descriptors ordered by offset.
 * block_start[t] = sum_{u<t} ceil(numel[u] / nbest_bertadam_chunk()); n_blocks = that sum over all
 * tensors.  If p_lowp != NULL the updated parameters are also written as bf16 at the same element
 * offsets (the compute copy the GEMMs read).  ws: >= (n_blocks + n_tensors) floats.                 */
typedef struct nbest_tensor_desc {
  int64_t offset;
  int64_t numel;
  float lr;            /* base learning rate of the tensor (bert_lr / lr) */
  float wd;            /* 0.01, or 0 for bias / LayerNorm */
  int32_t active;      /* 0: no gradient this step (skipped, like `p.grad is None`) */
  int32_t block_start;
} nbest_tensor_desc;
int nbest_bertadam_chunk(void);
int nbest_bertadam_step(float* p, const float* g, float* m, float* v, void* p_lowp, const nbest_tensor_desc* descs,
                        int n_tensors, int n_blocks, float lr_mult, double b1, double b2, float eps,
                        float max_grad_norm, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* The same step in two halves over a range of blocks [blk_lo, blk_hi) (new functionality: the optimizer sharded over data-parallel
 * ranks).  norms: partial[blk] = sum of squares of block blk's gradient elements, for the blocks of the range (the caller zeroes
 * `partial` [n_blocks] and SUM-all-reduces it over the ranks).  update: clip coefficients of all tensors from `partial`
 * (coef [n_tensors], scratch), then BertAdam on the blocks of the range.  norms + update over [0, n_blocks) == nbest_bertadam_step. */
int nbest_bertadam_norms(const float* g, const nbest_tensor_desc* descs, int n_tensors, int n_blocks, int blk_lo, int blk_hi,
                         float* partial, nbest_stream_t stream);
int nbest_bertadam_update(float* p, const float* g, float* m, float* v, void* p_lowp, const nbest_tensor_desc* descs,
                          int n_tensors, int n_blocks, int blk_lo, int blk_hi, const float* partial, float* coef,
                          float lr_mult, double b1, double b2, float eps, float max_grad_norm, nbest_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K9b  torch Adam / HF AdamW over the same arenas and descriptors, under ONE global-norm clip
 * (the reference's n_best_asr_bert.py:266-277,551-569, --optim_choice adam | adamw):
 *   clip: total = sqrt(sum over every tensor of ||g_t||^2), c = min(1, max_grad_norm / (total + 1e-6)) (1 if max_grad_norm <= 0)
 *         = torch.nn.utils.clip_grad_norm_;
 *   NBEST_ADAM_L2 (torch.optim.Adam, weight_decay = l2): g = c g + wd p; m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2;
 *         p -= (lr lr_mult / bc1) m / (sqrt(v) / bc2_sqrt + eps), bc1 = 1 - b1^t, bc2_sqrt = sqrt(1 - b2^t);
 *   NBEST_ADAMW (HF AdamW, correct_bias=False; pass bc1 = bc2_sqrt = 1): g = c g; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *         p -= lr lr_mult m / (sqrt(v) + eps); then, if wd > 0, p -= lr lr_mult wd p (on the updated p).
 * lr and wd are the descriptor's (torch Adam: the same lr and wd = l2 in every descriptor).  b1 and b2 are doubles: the kernels
 * use (float)b and (float)(1 - b), the values torch's kernels receive from its Python-float hyper-parameters.  Inactive tensors are
 * skipped and contribute nothing to the norm.
 * Range form: nbest_bertadam_norms writes the block sums of squares of each descriptor table; the caller lays the partials of
 * all tables back to back in one vector of n_partial floats (zeroed and SUM-all-reduced over the ranks when the optimizer is
 * sharded).  nbest_adam_clip_coef reduces it in a fixed order (fp64) into clip[0] = c, clip[1] = total norm (device memory:
 * no host synchronisation); nbest_adam_update then updates blocks [blk_lo, blk_hi) of one table, reading clip[0].
 * nbest_adam_step = norms + clip coefficient + update of one table; ws: >= (n_blocks + 2) floats.  g is read, never written.
 * A mode that is neither of the two, bc1 <= 0 or bc2_sqrt <= 0, a range outside 0 <= blk_lo <= blk_hi <= n_blocks: NBEST_ERR_ARG; a
 * short ws: NBEST_ERR_WORKSPACE; either way nothing is enqueued (the step forms check before their first launch), as in K9.        */
enum { NBEST_ADAM_L2 = 0, NBEST_ADAMW = 1 };
int nbest_adam_clip_coef(const float* partial, int n_partial, float max_grad_norm, float* clip, nbest_stream_t stream);
int nbest_adam_update(int mode, float* p, const float* g, float* m, float* v, void* p_lowp, const nbest_tensor_desc* descs,
                      int n_tensors, int n_blocks, int blk_lo, int blk_hi, const float* clip, float lr_mult, float bc1,
                      float bc2_sqrt, double b1, double b2, float eps, nbest_stream_t stream);
int nbest_adam_step(int mode, float* p, const float* g, float* m, float* v, void* p_lowp, const nbest_tensor_desc* descs,
                    int n_tensors, int n_blocks, float lr_mult, float bc1, float bc2_sqrt, double b1, double b2, float eps,
                    float max_grad_norm, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K9e  exponential moving average of the weights (--ema_decay; new functionality, the reference has none) over the same arenas and
 * descriptor tables, one launch per table, n_blocks workgroups, no workspace, bit-reproducible.
 * nbest_ema_update: for every element of every ACTIVE tensor ema = fma(one_minus_decay, p - ema, ema); inactive tensors and the
 *   elements between tensors are never written; an element whose result compares equal to its old value keeps its bits, so
 *   one_minus_decay == 0 and ema == p leave it bit-identical.  12 B per parameter (8 read, 4 written).
 * nbest_ema_exchange: swaps p and ema element by element, in place, for EVERY tensor of the table whatever its `active`; if
 *   p_lowp != NULL the new p is also written as bf16 at the same element offsets (the conversion of the optimizer kernels).  A
 *   pure move: two calls restore every bit of p and ema.  16 (+ 2) B per parameter.
 * A NULL p / ema / descs, n_tensors <= 0 or n_blocks <= 0: NBEST_ERR_ARG, nothing enqueued.                                       */
int nbest_ema_update(float* ema, const float* p, const nbest_tensor_desc* descs, int n_tensors, int n_blocks,
                     float one_minus_decay, nbest_stream_t stream);
int nbest_ema_exchange(float* p, float* ema, void* p_lowp, const nbest_tensor_desc* descs, int n_tensors, int n_blocks,
                       nbest_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K9s  sharpness-aware minimization (--sam_rho; new functionality, the reference has none): the weight-space half of a SAM step
 * (Foret et al., 2021: the gradient is taken at w + e, e = rho g / ||g||, and applied at w) and of its scale-invariant variant
 * ASAM (Kwon et al., 2021: e = rho T^2 g / ||T g||, T = diag(|w| + eta)), over the same arenas and descriptor tables, one launch
 * per table, n_blocks workgroups, no workspace, bit-reproducible.  Inactive tensors and the elements between tensors are never
 * read or written; g is read, never written.
 * nbest_sam_norms: the adaptive norm stage, partial[blk] = sum over block blk of (t g)^2, t = |p| + eta, in the summation shape
 *   of nbest_bertadam_norms (0 for the blocks of inactive tensors).  Plain SAM uses nbest_bertadam_norms itself.  Either way the
 *   caller lays the partials of all tables back to back and nbest_adam_clip_coef(partial, n, 0, clip) leaves the norm in clip[1],
 *   on the device: no other reduce kernel, no host synchronisation.  8 B per parameter.  eta finite and > 0.
 * nbest_sam_perturb: s = rho / (norm[0] + 1e-12f) (norm: device fp32[1]); for every element of every active tensor backup = p,
 *   then p = fma(s, g, p) (eta < 0: plain) or t = |p| + eta, p = fma(s, (t t) g, p) (eta > 0: adaptive), the fma explicit;
 *   p_lowp != NULL: also the bf16 (round to nearest even) of the new p at the same element offsets.  rho == 0, or a norm that is 0
 *   or not finite: s = 0 - no arithmetic on g (which may hold inf or NaN), p keeps its bits (it is not rewritten), backup and
 *   p_lowp are written all the same.  18 B per parameter (8 read, 10 written: backup, p and the bf16 copy).
 * nbest_sam_restore: p = backup and p_lowp = its bf16, for every active tensor.  A pure move: after perturb + restore every bit of
 *   p and (a p_lowp that was the bf16 of p) is what it was.  10 B per parameter.
 * Refused before any launch (NBEST_ERR_ARG): a NULL p / g / backup / descs / norm / partial, n_tensors <= 0 or n_blocks <= 0, a
 * negative or non-finite rho, eta == 0 or a non-finite eta (nbest_sam_norms: eta <= 0).                                          */
int nbest_sam_norms(const float* p, const float* g, const nbest_tensor_desc* descs, int n_tensors, int n_blocks, float eta,
                    float* partial, nbest_stream_t stream);
int nbest_sam_perturb(float* p, const float* g, float* backup, void* p_lowp, const nbest_tensor_desc* descs, int n_tensors,
                      int n_blocks, const float* norm /* device fp32[1] */, float rho, float eta /* < 0: plain */,
                      nbest_stream_t stream);
int nbest_sam_restore(float* p, const float* backup, void* p_lowp, const nbest_tensor_desc* descs, int n_tensors, int n_blocks,
                      nbest_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K9l  LoRA on merged weights (--lora_rank; new functionality, the reference has none).  The encoder keeps reading the merged
 * matrix W = W0 + s B A (s = alpha / r) from the arenas; the factors live in an adapter arena `ab` (fp32) and never appear inside
 * a layer.  One table of nbest_lora_desc, ordered by tile_start, has one entry per adapted BLOCK: a contiguous row range of one
 * arena matrix (so query / key / value, the row thirds of the fused [3H, H] matrix, are blocks of their own).  A [rank, cols] and
 * B [rows, rank] are row-major at a_off / b_off of `ab`; `base` holds a packed [rows, cols] copy of W0's block at base_off.
 * The table is passed twice: descs_host (checked on the host before anything is enqueued) and descs_dev, the same bytes in device
 * memory (what the kernels read).  nbest_lora_plan fills tile_start and ws_off of a host table (tiles of 64 rows x 256 columns)
 * and returns the tile total and the workspace of nbest_lora_grad (== nbest_lora_grad_ws_bytes).
 * nbest_lora_merge: p[i, j] = base[i, j] + scale * sum_{k < rank} B[i, k] A[k, j] for every element of every block, in fp32, k
 *   ascending; p_lowp != NULL: also the bf16 (round to nearest even) of that value at the same element offset.  One writer per
 *   element, nothing outside the blocks is written; a result that compares equal to base keeps base's bits (B = 0: p == base).
 *   8 B per element (+ 2), one launch.
 * nbest_lora_grad: g_ab[a_off + k cols + j] = scale * sum_i B[i, k] g[i, j] and g_ab[b_off + i rank + k] = scale * sum_j g[i, j] A[k, j],
 *   g the dense gradient at the offsets of p.  g is read once (4 B per element); tile partials go to ws and a second launch adds
 *   them in tile order: no atomics, bit-identical run to run whatever ws held before.  Two launches.
 * Refused before the first launch: a NULL pointer, rank outside 1 .. NBEST_LORA_MAX_RANK, a tile_start / ws_off that is not
 * nbest_lora_plan's (NBEST_ERR_ARG); cols % 4 != 0, stride != cols (NBEST_ERR_SHAPE); an offset that is no multiple of 4 elements
 * or a buffer that is not 16-byte aligned (NBEST_ERR_ALIGN); a short ws (NBEST_ERR_WORKSPACE).                                     */
#define NBEST_LORA_MAX_RANK 64
typedef struct nbest_lora_desc {
  int64_t p_off;       /* first element of the block in p / p_lowp / g */
  int64_t base_off;    /* ... of its packed copy in base */
  int64_t a_off, b_off;/* A [rank, cols], B [rows, rank] in ab / g_ab */
  int64_t ws_off;      /* nbest_lora_plan: the block's partials in ws (elements) */
  int32_t rows, cols, stride, rank;   /* stride: row stride in p (== cols) */
  float scale;         /* alpha / rank */
  int32_t tile_start;  /* nbest_lora_plan: sum of the earlier blocks' ceil(rows / 64) * ceil(cols / 256) */
} nbest_lora_desc;
int nbest_lora_plan(nbest_lora_desc* descs_host, int n, int* n_tiles, size_t* ws_bytes);
size_t nbest_lora_grad_ws_bytes(const nbest_lora_desc* descs_host, int n);
int nbest_lora_merge(float* p, void* p_lowp /* may be NULL */, const float* base, const float* ab, const nbest_lora_desc* descs_host,
                     const nbest_lora_desc* descs_dev, int n, nbest_stream_t stream);
int nbest_lora_grad(const float* g, const float* ab, float* g_ab, const nbest_lora_desc* descs_host, const nbest_lora_desc* descs_dev,
                    int n, void* ws, size_t ws_bytes, nbest_stream_t stream);
/* Transposed bf16 copy of the weight matrices (same element offsets in `dst` as in `src`): matrix t is
 * [rows][cols] in src and [cols][rows] in dst.  The backward's dgrad GEMMs read this copy so that both of
 * their operands are k-contiguous (no transposed LDS reads).  descs: DEVICE array ordered by tile_start,
 * tile_start[t] = sum_{u<t} ceil(rows/64)*ceil(cols/64); n_tiles = that sum over all matrices.          */
typedef struct nbest_matrix_desc {
  int64_t offset;
  int32_t rows, cols;
  int32_t tile_start, pad;
} nbest_matrix_desc;
/* Recording side of the delayed fp8 scales.  Every kernel that records a tensor's amax (gamax_new / aamax_new of the encoder
 * descriptor, c8_amax_new of nbest_gemm_fp8_args) is handed a block of NBEST_AMAX_TENSOR_WORDS uint32 words for that tensor, not
 * one word: it raises ONE of 16 words spaced 256 bytes apart (picked by its block index), because device-scope accesses to a
 * single word serialise (about 1 ns each: the 65 536 waves of an e4m3 cast spent 100 us on them).  nbest_fp8_amax_fold writes
 * out[t] = max over the 16 words of tensor t (the single word the NEXT pass reads as *_amax_prev / a_amax) and zeroes the slots.
 * slots: uint32 [n_tensors][NBEST_AMAX_TENSOR_WORDS], zero-initialised by the caller once. */
#define NBEST_AMAX_TENSOR_WORDS 1024
int nbest_fp8_amax_fold(void* slots, void* out, int32_t n_tensors, nbest_stream_t stream);
/* nbest_fp8_amax_fold that RAISES instead of overwriting: out[t] = max(out[t], max over the 16 slot words of tensor t), the slots
 * zeroed.  Float bits are compared as unsigned integers (non-negative floats order like their bits).  What lets a calibration run
 * over several batches: the history of the fp8 inference (nbest_encoder_infer_fp8) is folded with it.                         */
int nbest_fp8_amax_fold_max(void* slots, void* out, int32_t n_tensors, nbest_stream_t stream);
/* The fp8 PRODUCERS on their own: the kernels that write, next to their bf16 output, the e4m3 copy a later fp8 GEMM reads, and record
 * the amax the next pass scales by.  nbest_encoder_forward / _backward are their only other callers; these entries forward their
 * arguments to the same internal functions (no kernel and no dispatch of their own) so that the contract below can be tested
 * kernel by kernel.  With every extra argument NULL each one IS its plain entry (nbest_layernorm_fwd, ...): same launch, same bits.
 *   amax_prev: ONE device word, the float bits of the amax the tensor had in the previous pass (what nbest_fp8_amax_fold wrote).
 *     The copy is e4m3(v * s), saturating at +-448, round to nearest even, with s = 2^floor(log2(T / amax_prev)), the exponent
 *     clamped to +-100; T = 224 for the forward activations (layernorm_fwd, attention_fwd, cast), T = 56 for the gradients
 *     (layernorm_bwd, attention_bwd).  s = 1 for a NULL pointer and for a zero, denormal (< 2^-100) or non-finite amax.
 *   amax_new: a slot block of NBEST_AMAX_TENSOR_WORDS words (above): every workgroup RAISES one of the 16 words 64 k, k < 16 (picked
 *     by its block index), to the float bits of max |v| over its elements - never lowered; the other 1008 words are not touched.
 *   v, the value that is scaled, rounded and measured:
 *     layernorm_fwd, attention_fwd, attention_bwd, cast: the STORED bf16 value (y, ctx, dqkv, src) - the bytes are what a cast of
 *       the bf16 output gives, the recorded amax is max |bf16 output| exactly.
 *     layernorm_bwd: the fp32 value BEFORE its bf16 rounding - dx, or under dropout dx_drop = dx . keep . scale (a dropped element
 *       gives byte 0x00 and does not count in the amax).  bf16 rounding is monotone, so bf16(recorded amax) = max |bf16 output|.
 *   What each one records without a copy (out8 / y8 / ctx8 NULL, amax_new given - the calibration pass): attention_fwd,
 *   attention_bwd and layernorm_bwd record the same amax as with the copy; layernorm_fwd records NOTHING without y8 (the encoder
 *   calibrates that tensor with nbest_amax_bf16).
 *   layernorm_bwd writes its copy only where it records: out8 or amax_prev without amax_new is NBEST_ERR_ARG.
 *   bf16 only, and for the LayerNorms H in {256, 512, 768, 1024} only (the fast kernels): ANY of the copy, amax_prev and amax_new
 *   with fp32 or another H is NBEST_ERR_SHAPE, in all four entries.
 *   attention_bwd: dqkv may be NULL when out8 is given (only the copy is written).  layernorm_bwd under dropout: dx_drop may be
 *   NULL when out8 (and so amax_new) is given.  keep: as nbest_attention_fwd_keep / _bwd_keep (NULL: none).
 *   nbest_cast_bf16_to_fp8_scaled: the cast with a history (n % 8 == 0, else NBEST_ERR_ARG).  nbest_amax_bf16: slots raised by
 *   max |x| of a bf16 tensor (n % 8 == 0; the calibration pass of tensors whose producer is a bf16 kernel).                       */
int nbest_layernorm_fwd_fp8(const void* x, const float* gamma, const float* beta, void* y, void* y8, float* stats, int64_t M, int H,
                            float eps, int dtype, const uint32_t* amax_prev, uint32_t* amax_new, nbest_stream_t stream);
int nbest_layernorm_bwd_fp8(const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_drop,
                            float* dgamma, float* dbeta, float* dbias, int64_t M, int H, int dtype, int accumulate, float drop_p,
                            uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, void* out8, const uint32_t* amax_prev,
                            uint32_t* amax_new, nbest_stream_t stream);
int nbest_attention_fwd_fp8(const void* qkv, const uint8_t* key_mask, void* ctx, void* ctx8, float* lse, int B, int S, int heads,
                            int d, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, void* keep,
                            const uint32_t* amax_prev, uint32_t* amax_new, nbest_stream_t stream);
int nbest_attention_bwd_fp8(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx, const float* lse,
                            void* dqkv, float* dbias, int accumulate, void* ws, size_t ws_bytes, int B, int S, int heads, int d,
                            int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, const void* keep, void* out8,
                            const uint32_t* amax_prev, uint32_t* amax_new, nbest_stream_t stream);
int nbest_cast_bf16_to_fp8_scaled(const void* src, void* dst, int64_t n, const uint32_t* amax_prev, uint32_t* amax_new,
                                  nbest_stream_t stream);
int nbest_amax_bf16(const void* x, int64_t n, uint32_t* amax_new, nbest_stream_t stream);
/* e4m3 copy of the weight matrices (same element offsets, ONE byte per element) from the fp32 master, one scale per
 * matrix: w8 = e4m3(w * 2^floor(log2(224 / max|w|))); inv_scale[i] = 1 / scale of matrix i (device, [n_matrices]).
 * w8t (optional): the same e4m3 values written transposed ([cols][rows] at the matrix' offset; n_tiles = 64x64 tiles over all
 * matrices, descs[].tile_start as for nbest_transpose_weights) - the B operand of the fp8 dgrad GEMMs.
 * ws: >= 4 * n_matrices bytes.  Run after every optimizer step, like nbest_transpose_weights.                       */
int nbest_quantize_weights_fp8(const float* master, void* w8, void* w8t, const nbest_matrix_desc* descs, int n_matrices,
                               int n_tiles, float* inv_scale, void* ws, size_t ws_bytes, nbest_stream_t stream);
int nbest_transpose_weights(const void* src, void* dst, const nbest_matrix_desc* descs, int n_matrices, int n_tiles,
                            nbest_stream_t stream);
/* Weight matrices pre-packed for the k-contiguous GEMM kernels (nbest_gemm_args::B_packed).  For each matrix of `descs` (offset in
 * elements into both arenas, rows = N, cols = K, pad = tile width nbest_pack_bn(N) > 0, cols % 32 == 0, rows % pad == 0; tile_start =
 * running sum of (rows / pad) * (cols / 32) = index of the matrix' first (tile column, K stage) block; n_stages = that sum over all
 * matrices) `dst` receives, for every tile column and every 32-deep K stage, the pad x 32 tile in the exact order the kernel's LDS image
 * has (16-byte chunk swizzle and row permutation applied).  Same bytes as the source, N * K elements per matrix at the same offset.
 * Once per optimizer step, beside nbest_transpose_weights / the bf16 copy refresh of nbest_bertadam_step (the nn.Linear weights of the
 * installed modeling_bert.py:154-177, 282-293, 325-351 do not change inside a step).                                                   */
int nbest_pack_bn(int64_t N);
/* the same for the e4m3 copies read by nbest_gemm_fp8 (descs[].pad = nbest_pack_bn_fp8(rows, cols) = 256 | 128, cols % 64 == 0,
 * tile_start / n_stages in units of (tile column, 64-byte K stage) blocks; one byte per element at the arena's element offsets)      */
int nbest_pack_bn_fp8(int64_t N, int64_t K);
int nbest_pack_weights_fp8(const void* src, void* dst, const nbest_matrix_desc* descs, int n_matrices, int n_stages, nbest_stream_t stream);
int nbest_pack_weights(const void* src, void* dst, const nbest_matrix_desc* descs, int n_matrices, int n_stages, nbest_stream_t stream);
/* fp32 -> bf16 copy of an arena (initial compute copy / after loading a checkpoint) */
int nbest_cast_f32_to_bf16(const float* src, void* dst, int64_t n, nbest_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The whole encoder stack in one call (launch-overhead-free path used by training):
 * embeddings -> L x {QKV GEMM, attention, out-proj+residual, LN, FFN-up+GELU, FFN-down+residual, LN}.
 * Replaces the encoder(...) calls at /root/reference/models/model.py:43-45,54-56 and autograd
 * through them (/root/reference/n_best_asr_bert.py:264).
 * Parameter arenas: `wts` = matrices/tables in `dtype`, `prm` = the fp32 master arena (biases,
 * LayerNorm), `grad` = fp32 gradient arena; all three share ONE element-offset table
 * (nbest_encoder_layout).  act: activation stash written by forward, consumed by backward,
 * >= nbest_encoder_act_bytes(); ws: scratch >= nbest_encoder_ws_bytes().                            */
typedef struct nbest_layer_offsets {
  int64_t wqkv, bqkv, wo, bo, ln1_g, ln1_b, w1, b1, w2, b2, ln2_g, ln2_b;
} nbest_layer_offsets;
typedef struct nbest_encoder_desc {
  int32_t dtype, B, S, H, L, heads, F;
  int32_t vocab, max_pos, n_types;
  float ln_eps, hidden_drop, attn_drop;
  int64_t word_pad_id, pos_pad_id; /* padding_idx rows (no gradient), -1 = none */
  int64_t off_word, off_pos, off_type, off_emb_ln_g, off_emb_ln_b;
  const nbest_layer_offsets* layers_host; /* [L], HOST memory */
  uint64_t seed;
  uint32_t drop_stream_base; /* distinct per encoder pass within a step */
  int32_t wgrad_events_n;    /* entries of wgrad_events (0 = no timing) */
  /* optional in-step timing of the weight-gradient GEMMs (bench.py's roofline object): caller-created hipEvent_t
   * handles; nbest_encoder_backward records wgrad_events[2*i] before and [2*i+1] after the i-th weight-gradient
   * launch it enqueues (nbest_encoder_wgrad_launches_per_layer() per layer, highest layer first: FFN-down, FFN-up,
   * attention-out, QKV - or, bf16, FFN-down, FFN-up, QKV + attention-out as one nbest_wgrad_pair launch), on the
   * caller's stream, while i < wgrad_events_n / 2.  The library never creates, waits on or destroys events.
   * Grouped weight gradients (wgrad_group below; launches per layer == 1): ONE pair per layer, recorded so that the pairs of the
   * layers of a group add up to the group's launch - the pair of the group's first (highest) layer brackets the grouped launch, the
   * pair of its second layer is recorded back to back right after it - so the mean over the pairs is the time per LAYER's worth
   * of gradients.  A layer left without a partner issues its split-K launches back to back at its end, inside its one pair.
   * Rolling windows (NBEST_WGRAD_GROUP_WINDOW; launches per layer == 1): ONE pair per layer of the call's range; a pair brackets each
   * window launch (the peeled split-K pair launch inside the pair of the window next to it), the pairs left over are recorded back to
   * back at the end of the call - the sum over the range's pairs is the weight-gradient time of the call, the mean the time per
   * LAYER's worth of gradients.                                                                                                     */
  void** wgrad_events;
  /* optional fp8 forward ("fp8w"; dtype must be NBEST_BF16): e4m3 copy of the weight arena (one byte per element at the
   * same element offsets) and its per-matrix inverse scales [4 L] (QKV, attention-out, FFN-up, FFN-down per layer), both
   * from nbest_quantize_weights_fp8.  The forward GEMMs then run on the block-scaled fp8 MFMA; their activation operands
   * are e4m3 copies written by the producers with a DELAYED per-tensor scale (aamax_* below); everything else is the bf16 path. */
  const void* w8;
  const float* w8_inv_scale;
  /* optional fp8 dgrads (needs w8): transposed e4m3 weight copy and the per-(layer, tensor) gradient amax history gamax_prev, uint32
   * float bits [4 L]: index 4 l + {0: FFN-down input gradient, 1: FFN-up input gradient (after GELU'), 2: attention-out
   * input gradient, 3: dQ|dK|dV}.  The backward always RECORDS this pass's amax (when gamax_new is non-NULL) into gamax_new, which is
   * a SLOT ARRAY uint32 [4 L][NBEST_AMAX_TENSOR_WORDS] (see nbest_fp8_amax_fold); with fp8_bwd != 0 the producers also write e4m3
   * copies scaled from gamax_prev and the four dgrad GEMMs of a layer run on the fp8 MFMA.  Between passes the caller folds the
   * slots into the history (nbest_fp8_amax_fold(gamax_new, gamax_prev, 4 L)) and sets fp8_bwd only once a history exists.   */
  const void* w8t;
  const uint32_t* gamax_prev;
  uint32_t* gamax_new;
  int32_t fp8_bwd;
  /* (in the slot that was padding: no offset and no size changes)
   * head_gate_stash != 0 (needs head_gate): training under a head mask, see head_gate below.  Zero = no gated-context stash (the
   * behaviour without the field). */
  int32_t head_gate_stash;
  /* optional (bf16): the weight arena packed by nbest_pack_weights for the forward GEMMs (wpk: matrices as stored, [out][in]) and for
   * the dgrad GEMMs (wpkt: packed from the TRANSPOSED copy wts_t), at the arena's element offsets; NULL = the GEMMs read wts / wts_t */
  const void* wpk;
  const void* wpkt;
  /* optional (fp8w): w8 / w8t packed by nbest_pack_weights_fp8, at the arena's element offsets (bytes) */
  const void* w8p;
  const void* w8tp;
  /* REQUIRED by nbest_encoder_backward(with_embeddings): token indices of THIS pass sorted by word id (stable), int32 [B*S], device
   * memory - see nbest_embed_ln_bwd.  Set per call like `seed` (it belongs to the batch, not to the shape).                        */
  const int32_t* word_perm;
  /* fp8 forward: activation amax history aamax_prev, uint32 float bits [4 L]: index 4 l + {0: layer input x (QKV GEMM), 1: ctx
   * (attention-out GEMM), 2: x1 (FFN-up GEMM), 3: gelu(u) (FFN-down GEMM)}.  Every forward pass RECORDS this pass's amax into
   * aamax_new (when non-NULL), a SLOT ARRAY uint32 [4 L][NBEST_AMAX_TENSOR_WORDS] like gamax_new.  With fp8_act != 0 (a history
   * exists in aamax_prev) the producers write e4m3(a * s), s = 2^floor(log2(224 / amax_prev)), the GEMMs divide by s (and the fp8
   * weight gradients of the backward, which read the same copies, too); with fp8_act == 0 the forward is a CALIBRATION pass: it
   * runs the bf16 GEMMs and only records the amax.  After every step (after the backward, which reads the copies scaled by prev)
   * the caller folds: nbest_fp8_amax_fold(aamax_new, aamax_prev, 4 L), and sets fp8_act once a history exists.                  */
  const uint32_t* aamax_prev;
  uint32_t* aamax_new;
  int32_t fp8_act;
  /* (in the slot that was padding: zero = every entry point enqueues exactly the launches it did without the field, and the size
   * of the struct is unchanged)
   * cls_top != 0: the top layer (L - 1) is trained on the CLS rows only.  Everything that reads the final hidden state reads row 0
   * of each utterance, so the backward's dhidden is zero outside those B rows and, of the top layer, only the K and V rows of the
   * other positions can reach the result.  nbest_encoder_forward then runs the top layer's QKV projection over all B S rows as
   * before and everything after it on B rows: a one-query attention per (utterance, head), attention-out, LayerNorm, FFN and
   * LayerNorm, with the dropout decisions the full-width kernels take for rows b S.  The B output rows go to rows b S of the final
   * hidden state; ITS OTHER ROWS ARE NOT WRITTEN.  The compact intermediates occupy the first B rows of the top layer's stash
   * regions (the LayerNorm output rows B .. 2 B - 1 of r2 on their way to the hidden state); its lse and keep words are not
   * written.  nbest_encoder_backward with layer_end == L reads dhidden at rows b S only, runs the top layer's LayerNorm backwards,
   * FFN and attention-out dgrads on B rows, forms the gradients of Wo, W1 and W2 as plain launches over K = B token rows (they
   * honour accumulate and wgrad_skip_host and are not part of the grouped / window queue), recomputes the B heads softmax rows in a
   * one-query attention backward that writes the layer's dQ|dK|dV in full (dQ zero outside the CLS rows), and runs the QKV dgrad
   * and weight gradient unchanged.  Event pairs (wgrad_events): as many as without the flag; the top layer's bracket its small
   * launches.  Same results up to summation order (fp32) / one more rounding of the B rows (bf16); bit-reproducible run to run.
   * Refused (NBEST_ERR_ARG, nothing enqueued) with the fp8 forward (w8), head_gate without head_gate_stash, base_ids / alpha,
   * no_param_grad and S < 2.
   * first_trainable == L (nothing stashed, no backward) is accepted: the forward runs the top layer on the CLS rows of the frozen
   * layers' scratch, so the final CLS rows are the bits a trainable top layer gives.  The backward must see the value the forward of
   * its stash saw.  nbest_encoder_infer* ignore the field; nbest_encoder_act_view refuses the top layer of such a stash.           */
  int32_t cls_top;
  /* optional frozen parameters (zero = everything trainable).  first_trainable = K in [0, L]: nothing of the embeddings or of layers
   * [0, K) is trainable - nbest_encoder_forward runs those layers on scratch in `ws` (which it then needs: nbest_encoder_ws_bytes)
   * with the same dropout streams, stashes nothing of them (nbest_encoder_act_bytes covers X[K..L] and layers K..L-1 only) and, in
   * the fp8 mode, still records their activation amax; nbest_encoder_backward refuses layer_begin < K and with_embeddings unless
   * K == 0.  no_input_grad != 0: the backward leaves out the gradient w.r.t. the input of layer K (its QKV dgrad GEMM and residual
   * add; dhidden is not valid afterwards); refuses with_embeddings.  wgrad_skip_host: HOST memory [4 L] (NULL = none), non-zero =
   * the weight-gradient GEMM of that matrix (QKV, attention-out, FFN-up, FFN-down per layer) is left out and its gradient is not
   * written.  Bias and LayerNorm gradients are always written (except with no_param_grad below).                               */
  int32_t first_trainable;
  int32_t no_input_grad;
  /* optional adversarial perturbation of the word rows (FGM; nbest_embed_adv_delta): fp32 [B*S][H], device memory, set per call like
   * `seed`.  Non-NULL: nbest_encoder_forward's embedding is nbest_embed_ln_fwd_adv and nbest_encoder_backward(with_embeddings) runs
   * nbest_embed_ln_bwd_adv - the backward must see the pointer (and the values) its stash's forward saw.  Everything above the
   * embedding is unchanged, cls_top included.  NULL: the plain embedding launches.  Refused (NBEST_ERR_ARG, nothing enqueued) with the fp8 forward
   * (w8), base_ids / alpha and first_trainable > 0; nbest_encoder_infer* refuse it.                                              */
  const float* emb_delta;
  const uint8_t* wgrad_skip_host;
  /* optional head gates (NULL = none: every entry point then enqueues exactly the launches it did without these fields; the two
   * pointers sit here, ahead of the attribution fields, which stay the descriptor's last).
   * head_gate: fp32 [L][heads], device.  Layer l multiplies head h's slice of its attention context by head_gate[l][h] after
   * dropout and P.V, before the attention-output GEMM (nbest_head_gate_fwd).  nbest_encoder_forward keeps the UN-gated context in
   * the stash and writes the gated copy into the workspace (which it then needs: nbest_encoder_ws_bytes); nbest_encoder_infer /
   * _infer_attn gate in place.  Attention maps (nbest_attention_probs on the stash, cls_attn) stay the un-gated probabilities.
   * nbest_encoder_backward launches nbest_head_gate_bwd between a layer's attention-output dgrad GEMM and its attention backward.
   * head_gate_grad: fp32 [L][B][heads], device (needs head_gate): the backward writes d loss / d head_gate[l][h] per utterance b for
   * the layers of [layer_begin, layer_end) (overwritten; other layers untouched).
   * Refused (NBEST_ERR_ARG, nothing enqueued): head_gate with the fp8 forward (w8) or with first_trainable > 0, head_gate_grad
   * without head_gate, and a backward with head_gate but without no_param_grad (the attention-output weight gradient would need
   * the gated context, which is not kept) - all of this without head_gate_stash.
   * head_gate_stash != 0 (the field after fp8_bwd) keeps the gated context too, so that parameters can be trained under the gates:
   * the activation stash gains one region gctx [M][H] of the dtype per stashed layer, after everything else (the offsets of every
   * other region, and nbest_encoder_act_view, are unchanged; nbest_encoder_act_bytes grows by (L - first_trainable) [M][H] regions,
   * nbest_encoder_ws_bytes does not change).  The forward of a stashed layer writes the gated copy to gctx (not to the workspace)
   * and the attention-output GEMM reads it; ctx stays un-gated for the attention backward.  A frozen layer (l < first_trainable)
   * gates its scratch context in place, so first_trainable > 0 (up to L) is accepted; the cls_top layer gates its B compact rows
   * into the first B rows of gctx, so cls_top is accepted.  nbest_encoder_backward runs with parameter gradients: the
   * attention-output weight gradient reads gctx (plain, paired, grouped, window and cls_top launches alike - the stash outlives the
   * deferred ones), and nbest_head_gate_bwd scales dctx by the gate ahead of the attention backward (cls_top layer: over the B
   * compact rows, S = 1).  The weights of a head with gate 0 get exactly zero gradients (its Wo columns, its Q / K / V rows and
   * biases).  The backward must see the flag its stash's forward saw.  Refused with head_gate_stash (NBEST_ERR_ARG, nothing
   * enqueued): head_gate == NULL, the fp8 forward (w8), emb_delta, base_ids / alpha, no_param_grad and head_gate_grad.
   * nbest_encoder_infer* ignore head_gate_stash.                                                                                 */
  const float* head_gate;
  float* head_gate_grad;
  /* optional interpolated embeddings (integrated gradients): base_ids int64 [B*S] and alpha fp32 [B], device memory, set per call
   * like `seed`.  Both non-NULL: nbest_encoder_forward's embedding is nbest_embed_ln_fwd_interp; NULL: nbest_embed_ln_fwd, launch for
   * launch as before.  nbest_encoder_infer refuses them.                                                                         */
  const int64_t* base_ids;
  const float* alpha;
  /* no_param_grad != 0: nbest_encoder_backward forms dhidden only (down to the gradient w.r.t. the embedding LayerNorm output with
   * layer_begin = 0); grad may be NULL.  It enqueues no weight-gradient GEMM and no split-K reduce, and writes no bias or
   * LayerNorm-parameter gradient (no column sums in the LayerNorm backward, the attention backward or the DGELU epilogue, no
   * row-reduction finalize).  dhidden is bit-equal to that of the ordinary backward on the same stash.  Refuses with_embeddings,
   * first_trainable > 0, no_input_grad and the fp8 forward (w8).                                                                 */
  int32_t no_param_grad;
  /* (the descriptor's last field, in the slot that was padding: zero = the plan decides, the size of the struct is unchanged)
   * weight gradients of two layers in one launch without K-splits (nbest_wgrad_group; bf16 without the fp8 forward, H and F multiples
   * of 256): NBEST_WGRAD_GROUP_PLAN (0) - the library's plan decides from the tile counts and the token count (it groups where its
   * launch-cost model predicts a gain: bert-base / xlm-roberta-base shapes; not xlm-roberta-large, whose 192 tiles per layer leave no
   * room for a second layer), NBEST_WGRAD_GROUP_NEVER - the split-K launches of every layer, NBEST_WGRAD_GROUP_ALWAYS - group wherever the
   * shapes allow.  Layers l, l-1 of a backward call's [layer_begin, layer_end) form a group, from the top; a group never crosses the
   * range, and a layer left over runs the split-K launches.  The dY tensors of a layer then live until the group's launch: two sets
   * of them in the workspace (nbest_encoder_ws_bytes follows this field).  Same results up to the fp32 summation order over K.
   * NBEST_WGRAD_GROUP_WINDOW - rolling windows (also at most 256 tiles per layer; else as _NEVER): the gradients of a call's layers,
   * the highest first, QKV | attention-out | FFN-up | FFN-down within a layer, are a queue of 256 x 256 tiles, and a launch
   * (nbest_wgrad_window) takes the next 256 pending tiles whichever layers they belong to - 1 296 tiles of 12 bert-base layers in 5
   * rounds of the 256 CUs where the grouped launches of 216 take 6.  The rest is flushed at the end of the call (every call leaves
   * its gradients written).  Where it saves a whole round, the QKV + attention-out pair of the range's lowest layer runs as mode _NEVER's
   * split-K pair launch instead (bert-base: 1 260 tiles = 256 + 256 + 256 + 256 + 236).  The dY tensors of a layer live until its last
   * tile is launched: N buffer sets in rotation, N from the tile counts (4 at 108 tiles per layer, 2 at 192).  The plan (_PLAN) takes
   * the windows where its launch-cost model predicts at least 5 % less weight-gradient time than the better of the other two.  Window
   * launches give the bits of _ALWAYS, the peeled pair those of _NEVER.  nbest_encoder_wgrad_plan reports the resolved schedule.      */
  int32_t wgrad_group;
} nbest_encoder_desc;
enum { NBEST_WGRAD_GROUP_PLAN = 0, NBEST_WGRAD_GROUP_NEVER = 1, NBEST_WGRAD_GROUP_ALWAYS = 2, NBEST_WGRAD_GROUP_WINDOW = 3 };
size_t nbest_encoder_act_bytes(const nbest_encoder_desc* d);
/* Pointers into a stash `act` written by nbest_encoder_forward with descriptor d: layer `layer`'s qkv [M][3H] (dtype; also in the fp8
 * forward and its calibration pass) and lse [B][heads][S] (fp32) - the inputs of nbest_attention_probs.  Refuses (NBEST_ERR_ARG) a
 * layer outside [first_trainable, L): frozen layers are not stashed.  Enqueues nothing.                                           */
int nbest_encoder_act_view(const nbest_encoder_desc* d, void* act, int layer, void** qkv, float** lse);
size_t nbest_encoder_ws_bytes(const nbest_encoder_desc* d);
/* weight-gradient launches nbest_encoder_backward enqueues per layer for this descriptor = event pairs per layer in wgrad_events:
 * 1 when the gradients of two layers share one grouped launch or go out in rolling windows (desc.wgrad_group), else 3 when the attention-output gradient
 * rides with the QKV gradient (nbest_wgrad_pair; bf16, shapes that fit), else 4 */
int nbest_encoder_wgrad_launches_per_layer(const nbest_encoder_desc* d);
/* Host only, enqueues nothing: the weight-gradient schedule nbest_encoder_backward follows for this descriptor over the layers
 * [layer_begin, layer_end), as int32 words: out[0] the resolved mode (NBEST_WGRAD_GROUP_NEVER / _ALWAYS / _WINDOW), out[1] the dY
 * buffer sets (grouped: layers per launch; 0: split-K launches), out[2] the layer whose QKV + attention-out pair is peeled (-1: none),
 * out[3] the number of window launches, then per launch: the layer at whose end it is issued, its tiles, its entries n, and per entry:
 * layer, matrix (0 QKV, 1 attention-out, 2 FFN-up, 3 FFN-down), tile_first, tile_count.  Honours first_trainable, wgrad_skip_host and
 * no_param_grad.  Returns the number of words (written only when `cap` holds them all) or a negative NBEST_ERR_*.                   */
int nbest_encoder_wgrad_plan(const nbest_encoder_desc* d, int layer_begin, int layer_end, int32_t* out, int cap);
/* hidden_out: pointer to the final hidden states [M][H] inside act (returned through *hidden_out) */
int nbest_encoder_forward(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids,
                          const int64_t* seg, const int64_t* pos, const uint8_t* key_mask, void* act,
                          size_t act_bytes, void* ws, size_t ws_bytes, void** hidden_out, nbest_stream_t stream);
/* dhidden [M][H] (dtype) is consumed (overwritten): it always holds the running gradient w.r.t. the
 * input of the lowest layer processed so far.  Parameter gradients are written into `grad`
 * (overwritten; accumulate != 0: added).  Layers [layer_begin, layer_end) are processed in reverse;
 * with_embeddings != 0 also runs the embedding backward (needs layer_begin == 0).  Calling it in
 * chunks (L..k, k..0+embeddings) lets the host start the gradient all-reduce of finished layers
 * while the remaining backward runs.                                                                */
/* wts_t: optional arena holding the TRANSPOSED weight matrices (nbest_transpose_weights); NULL -> the dgrad
 * GEMMs read `wts` with transposed LDS reads.                                                            */
int nbest_encoder_backward(const nbest_encoder_desc* d, const void* wts, const void* wts_t, const float* prm, float* grad,
                           const int64_t* ids, const int64_t* seg, const int64_t* pos, const uint8_t* key_mask,
                           void* act, size_t act_bytes, void* dhidden, void* ws, size_t ws_bytes, int accumulate,
                           int layer_begin, int layer_end, int with_embeddings, nbest_stream_t stream);

/* Inference: the encoder forward without an activation stash, for the final hidden state of the B CLS rows only.  Same descriptor,
 * arenas and inputs as nbest_encoder_forward; cls_out [B][H] in the compute dtype.  Layers 0 .. L-2 are nbest_encoder_forward's
 * kernels (FFN-up without the GELU' rows); the last layer projects K|V on all B S rows and runs everything else on the B CLS rows.
 * ws >= nbest_encoder_infer_ws_bytes(d) (independent of L).  Refuses (NBEST_ERR_ARG) non-zero dropout, the fp8 forward (w8) and
 * interpolated embeddings (base_ids / alpha).                                                                                   */
size_t nbest_encoder_infer_ws_bytes(const nbest_encoder_desc* d);
int nbest_encoder_infer(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                        const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out, nbest_stream_t stream);
/* nbest_encoder_infer plus cls_attn [L][B][heads][S] fp32: the CLS row's attention probabilities of every layer
 * (nbest_attention_cls_probs, launched after the layer's QKV projection; last layer: from the CLS-row Q and the K|V it forms).
 * cls_attn == NULL is nbest_encoder_infer, launch for launch.  Same workspace.                                                  */
int nbest_encoder_infer_attn(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                             const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out, float* cls_attn,
                             nbest_stream_t stream);
/* nbest_encoder_infer on the compact images of nbest_head_prune_pack: layer l runs its QKV GEMM with N = 3 64k, K = H on Wqkv' and
 * bqkv', the attention with heads = k on qkv [M][3 64k] -> ctx [M][64k], and the attention-output GEMM with N = H, K = 64k on Wo'
 * (bias bo and the residual as always); LayerNorm and the FFN read the ordinary arena (and d->wpk).  The last layer keeps its
 * CLS-row form: K|V over all rows out of rows 64k.. of Wqkv' (N = 2 64k), Q on the B CLS rows, the one-query attention with
 * ldq = 64k, ldkv = 2 64k, heads = k.  No gate launch: the gate lives in Wo'.
 *   images: w = the weight image, w_packed = its nbest_pack_weights image or NULL (bf16; read for layers 0 .. L-2 only), bqkv =
 *   the bias image, layers_host = the table the images were packed by (k and dst_* are read).
 * d->head_gate must be NULL (NBEST_ERR_ARG); there is no attention-map output (the maps are indexed by original head).  bf16: every k
 * must be even (NBEST_ERR_SHAPE: the bf16 GEMM tiles need N = 64k to be a multiple of 128 - carry a head whose gate is 0).
 * The other refusals and the workspace are those of nbest_encoder_infer: every compact tensor is no larger than its full-width
 * counterpart.  Nothing is enqueued when a refusal is returned.                                                                   */
typedef struct nbest_head_prune_images {
  const void* w;
  const void* w_packed;
  const float* bqkv;
  const nbest_head_prune_layer* layers_host;
} nbest_head_prune_images;
int nbest_encoder_infer_pruned(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                               const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out,
                               const nbest_head_prune_images* images, nbest_stream_t stream);

/* nbest_encoder_infer for a model with the fp8 forward (desc.w8): same arguments, same cls_out [B][H] bf16.  The descriptor's fp8
 * fields mean what they mean for nbest_encoder_forward, and two kinds of pass follow from them:
 *   calibration pass (w8, w8_inv_scale, aamax_new set, fp8_act == 0): the launches of nbest_encoder_infer (cls_out has the same bits)
 *     plus the nbest_amax_bf16 launches that record the GEMM inputs into their slot blocks of aamax_new: layers 0 .. L-2 record
 *     x, ctx, x1, gelu(u) at index 4 l + {0, 1, 2, 3}, layer L-1 records x only, at 4 (L-1).  The caller folds the slots
 *     (nbest_fp8_amax_fold_max over several batches) into the history the fp8 pass reads.
 *   fp8 pass (fp8_act != 0, aamax_prev set): layers 0 .. L-2 run their four GEMMs on the block-scaled fp8 MFMA, on e4m3 copies in four
 *     regions at the end of the workspace; FFN-up is NBEST_EPI_BIAS_GELU_Q8 (no bf16 gelu(u), no gelu' rows).  The scales are STATIC:
 *     every producer scales by aamax_prev and records nothing (aamax_new is not read, no atomics).  Last layer: the K|V projection
 *     over all M rows is an fp8 GEMM on the e4m3 copy of the layer input; the B CLS rows stay bf16.  L = 1 works.
 *     A value beyond twice the calibrated amax saturates silently in the e4m3 cast (the scale is 2^floor(log2(224 / amax))).
 * ws >= nbest_encoder_infer_fp8_ws_bytes(d) = nbest_encoder_infer_ws_bytes(d) + the four e4m3 regions (>= M (3 H + F) bytes;
 * independent of L, the same for both passes).  Refuses, before the first launch: non-zero dropout, a dtype other than bf16, the shapes
 * the fp8 forward refuses, no w8 / w8_inv_scale, fp8_act != 0 without aamax_prev, fp8_act == 0 without aamax_new, head_gate,
 * base_ids / alpha, emb_delta (NBEST_ERR_ARG / _DTYPE / _SHAPE) and a short workspace (NBEST_ERR_WORKSPACE).                        */
size_t nbest_encoder_infer_fp8_ws_bytes(const nbest_encoder_desc* d);
int nbest_encoder_infer_fp8(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                            const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out, nbest_stream_t stream);

/* ---- token elimination between layers (PoWER-BERT, Goyal et al., ICML 2020, at a fixed count per layer) -----------------------------
 * nbest_token_select: per utterance, the k positions to keep out of S, by a score.  Position 0 is always kept; the other k - 1 are
 * the first of the remaining positions in this total order: unmasked before masked, then a score that is a number before a NaN, then
 * the higher score (-0 = +0, +inf highest), then the lower index.  score fp32 [B][S], key_mask u8 [B][S], 1 <= k <= S <= 512.
 *   idx_out   int32 [B][k]  the kept positions, ascending (so idx_out[b][0] == 0)
 *   mask_out  u8    [B][k]  key_mask of the kept positions (1 / 0); maskf_out fp32 [B][k] the same as 1.0 / 0.0
 *   origin_out int32 [B][k] origin_in[b][idx_out[b][r]] - origin_in int32 [B][S], NULL: the identity; origin_out may be NULL
 * One workgroup per utterance, ranks by counting over keys in LDS, slots by ballot and popcount: no atomics, bit-reproducible, every
 * output element written once.  Refused before anything is enqueued: a null pointer, idx_out equal to an input, mask_out == key_mask,
 * maskf_out == score or origin_out == origin_in (NBEST_ERR_ARG), a bad k or S (NBEST_ERR_SHAPE), NBEST_ERR_ALIGN.                    */
int nbest_token_select(const float* score, const uint8_t* key_mask, const int32_t* origin_in, int k, int32_t* idx_out, uint8_t* mask_out,
                       float* maskf_out, int32_t* origin_out, int B, int S, nbest_stream_t stream);
/* dst[b][r][:] = src[b][idx[b][r]][:] for r < k: src [B][S][H], dst [B][k][H] of dtype (bf16 or fp32), idx int32 [B][k] in [0, S)
 * (an index outside is clamped into it).  16-byte accesses: H a multiple of 8 (bf16) or 4 (fp32), src and dst 16-byte aligned and
 * different buffers.  Every dst element is written once.  NBEST_ERR_ARG / _SHAPE / _DTYPE / _ALIGN before anything is enqueued.      */
int nbest_rows_compact(const void* src, const int32_t* idx, void* dst, int B, int S, int k, int H, int dtype, nbest_stream_t stream);
/* nbest_encoder_infer that drops tokens between layers.  keep_host: n_keep == L - 1 positive, non-increasing int32 on the host;
 * keep_host[l] tokens per utterance leave layer l.  S_0 = S, S_{l+1} = min(keep_host[l], S_l).  Where S_{l+1} == S_l nothing is
 * launched for the layer, so a schedule of entries >= S is nbest_encoder_infer launch for launch.  Otherwise, after layer l:
 *   score[b][j] = (1 / heads) sum_h sum_{i unmasked} P_l[b][h][i][j]   (nbest_attention_rollout_step on the layer's qkv and lse, r_in
 *                                                                       the current mask as 1.0 / 0.0, residual 0)
 *   nbest_token_select keeps S_{l+1} positions; nbest_rows_compact gathers the layer's output rows; the key mask shrinks with them.
 * Layer l + 1 then runs on B S_{l+1} rows with sequence length S_{l+1}; the last layer reads the CLS rows (row 0 stays row 0).
 * token_kept: NULL or int32 [L-1][B][S] on the device; row l = the ORIGINAL positions of the tokens that leave layer l, ascending,
 * then -1 (a layer that eliminated nothing repeats the row below it; layer 0: the identity).
 * ws >= nbest_encoder_infer_tokens_ws_bytes(d) = nbest_encoder_infer_ws_bytes(d) + score, index, origin and mask rows (22 B S bytes,
 * each region rounded up to 256).  Refuses, before the first launch, what nbest_encoder_infer refuses, and desc.head_gate, desc.w8, a null or
 * wrong-length schedule, an entry < 1, an increasing schedule (NBEST_ERR_ARG).                                                       */
size_t nbest_encoder_infer_tokens_ws_bytes(const nbest_encoder_desc* d);
int nbest_encoder_infer_tokens(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                               const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out,
                               const int32_t* keep_host, int n_keep, int32_t* token_kept, nbest_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NBEST_HIP_H */
