// Host call trace of csrc/encoder.hip, which holds no kernel: every function it calls in the other sources and in the HIP runtime is a
// stub here that prints its name and arguments and returns success, so nbest_encoder_forward / nbest_encoder_backward run on fake
// addresses without a GPU and without the HIP runtime, and what they print is the exact sequence of launches, memsets and event records
// with every argument.  Two builds of encoder.hip behave the same for the traced descriptors when the outputs are byte-identical:
//
//   cd n-best-asr-transformer_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -c encoder.hip -o /tmp/encoder.o
//   hipcc -O1 -std=c++17 -c ../../tools/encoder_calltrace.cpp -o /tmp/calltrace.o
//   /opt/rocm/lib/llvm/bin/clang++ /tmp/encoder.o /tmp/calltrace.o -o /tmp/calltrace && /tmp/calltrace > new.txt
//   (the same with the other encoder.hip) ; cmp old.txt new.txt
//
// (-Xarch_host -fsanitize=address,undefined on the hipcc lines and -fsanitize=address,undefined on the link: the fixed tables of the
// weight-gradient schedules under the sanitizers.)  nbest_wgrad_pair_ws_bytes / nbest_wgrad_fp8_pair_ws_bytes answer non-zero or zero by
// a switch, so both answers of the pairing rule are traced.  Refused combinations print their error text and return code.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../n-best-asr-transformer_amd/csrc/internal.h"

struct Fp8Grad {   // csrc/common.h
  uint8_t* out8;
  const uint32_t* amax_prev;
  uint32_t* amax_new;
};

namespace {
bool g_pair_fits = true;

template <class T> void pr(T* p) { printf(" %#zx", (size_t)p); }
void pr(int v) { printf(" %d", v); }
void pr(long v) { printf(" %ld", v); }
void pr(long long v) { printf(" %lld", v); }
void pr(unsigned v) { printf(" %u", v); }
void pr(unsigned long v) { printf(" %lu", v); }
void pr(unsigned long long v) { printf(" %llu", v); }
void pr(float v) { printf(" %g", v); }
void pr(const Fp8Grad& f) { printf(" {%#zx %#zx %#zx}", (size_t)f.out8, (size_t)f.amax_prev, (size_t)f.amax_new); }
void pr(const nbest_gemm_args& g) {
  printf(" {A %#zx B %#zx C %#zx bias %#zx R %#zx U %#zx ws %#zx %zu | %ld %ld %ld | ld %ld %ld %ld %ld %ld | t %d %d epi %d dt %d acc %d | drop %g %u %lu |"
         " colsum %#zx %d flags %d | packed %#zx %d}",
         (size_t)g.A, (size_t)g.B, (size_t)g.C, (size_t)g.bias, (size_t)g.R, (size_t)g.U, (size_t)g.ws, g.ws_bytes, (long)g.M, (long)g.N, (long)g.K,
         (long)g.lda, (long)g.ldb, (long)g.ldc, (long)g.ldr, (long)g.ldu, g.trans_a, g.trans_b, g.epilogue, g.dtype, g.accumulate, g.drop_p,
         g.drop_stream, (unsigned long)g.seed, (size_t)g.colsum_out, g.colsum_accumulate, g.flags, (size_t)g.B_packed, g.b_pack_bn);
}
void pr(const nbest_gemm_fp8_args& g) {
  printf(" {A %#zx B %#zx C %#zx bias %#zx R %#zx U %#zx C8 %#zx | %ld %ld %ld | ld %ld %ld %ld %ld %ld %ld | epi %d scale %g %#zx | drop %g %u %lu |"
         " amax %#zx %#zx %#zx | colsum %#zx %d ws %#zx %zu | packed %#zx %d}",
         (size_t)g.A, (size_t)g.B, (size_t)g.C, (size_t)g.bias, (size_t)g.R, (size_t)g.U, (size_t)g.C8, (long)g.M, (long)g.N, (long)g.K, (long)g.lda,
         (long)g.ldb, (long)g.ldc, (long)g.ldr, (long)g.ldu, (long)g.ldc8, g.epilogue, g.out_scale, (size_t)g.out_scale_dev, g.drop_p, g.drop_stream,
         (unsigned long)g.seed, (size_t)g.a_amax, (size_t)g.c8_amax_prev, (size_t)g.c8_amax_new, (size_t)g.colsum_out, g.colsum_accumulate,
         (size_t)g.ws, g.ws_bytes, (size_t)g.B_packed, g.b_pack_bn);
}
void prs() {}
template <class T, class... R> void prs(const T& v, const R&... r) { pr(v); prs(r...); }
}  // namespace
#define TRACE(...) do { printf("  %s", __func__); prs(__VA_ARGS__); printf("\n"); } while (0)
#define STUB(...) { TRACE(__VA_ARGS__); return 0; }

// ---- the HIP runtime and api.cpp -------------------------------------------------------------------------------------------------
extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { TRACE(e, s); return hipSuccess; }
extern "C" hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t s) { TRACE(p, v, n, s); return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "stub"; }
void nbest_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  printf("  error: ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
}

// ---- sizes: fixed answers --------------------------------------------------------------------------------------------------------
extern "C" size_t nbest_gemm_ws_bytes(const nbest_gemm_args* a) { return (size_t)8 * a->M * a->N * sizeof(float); }
extern "C" size_t nbest_wgrad_fp8_ws_bytes(int64_t M, int64_t N, int64_t) { return (size_t)8 * M * N * sizeof(float); }
extern "C" size_t nbest_wgrad_pair_ws_bytes(const nbest_gemm_args* a, const nbest_gemm_args* b) {
  return g_pair_fits ? (size_t)8 * (a->M + b->M) * a->N * sizeof(float) : 0;
}
extern "C" size_t nbest_wgrad_fp8_pair_ws_bytes(int64_t Ma, int64_t Mb, int64_t N, int64_t) {
  return g_pair_fits ? (size_t)8 * (Ma + Mb) * N * sizeof(float) : 0;
}
extern "C" size_t nbest_attention_bwd_ws_bytes(int, int, int) { return 4096; }
extern "C" size_t nbest_embed_bwd_ws_bytes(int64_t, int64_t) { return 8192; }
extern "C" size_t nbest_rowred_ws_bytes(int64_t, int64_t) { return 16384; }
size_t nbest_internal_attention_keep_bytes(int B, int S, int heads) { return S <= 256 ? (size_t)B * heads * 1024 : 0; }
extern "C" int nbest_pack_bn(int64_t) { return 256; }
extern "C" int nbest_pack_bn_fp8(int64_t, int64_t) { return 128; }

// ---- launching entry points ------------------------------------------------------------------------------------------------------
extern "C" int nbest_gemm(const nbest_gemm_args* a, nbest_stream_t s) STUB(*a, s)
extern "C" int nbest_gemm_fp8(const nbest_gemm_fp8_args* a, nbest_stream_t s) STUB(*a, s)
extern "C" int nbest_wgrad_pair(const nbest_gemm_args* a, const nbest_gemm_args* b, nbest_stream_t s) STUB(*a, *b, s)
extern "C" int nbest_wgrad_group(const nbest_gemm_args* p, int n, nbest_stream_t s) {
  TRACE(n, s);
  for (int i = 0; i < n; ++i) { printf("   "); pr(p[i]); printf("\n"); }
  return 0;
}
extern "C" int nbest_wgrad_window(const nbest_gemm_args* p, const int32_t* first, const int32_t* count, int n, nbest_stream_t s) {
  TRACE(n, s);
  for (int i = 0; i < n; ++i) { printf("    [%d, +%d)", first[i], count[i]); pr(p[i]); printf("\n"); }
  return 0;
}
extern "C" int nbest_wgrad_fp8(const void* dY8, const void* X8, float* dW, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                               const uint32_t* a_amax, const uint32_t* x_amax, int accumulate, void* ws, size_t ws_bytes, nbest_stream_t s)
    STUB(dY8, X8, dW, M, N, K, lda, ldb, ldc, a_amax, x_amax, accumulate, ws, ws_bytes, s)
extern "C" int nbest_wgrad_fp8_pair(const void* dY8a, const void* X8a, float* dWa, int64_t Ma, int64_t lda_a, int64_t ldb_a, int64_t ldc_a,
                                    const uint32_t* amax_a, const uint32_t* xamax_a, const void* dY8b, const void* X8b, float* dWb, int64_t Mb,
                                    int64_t lda_b, int64_t ldb_b, int64_t ldc_b, const uint32_t* amax_b, const uint32_t* xamax_b, int64_t N,
                                    int64_t K, int accumulate, void* ws, size_t ws_bytes, nbest_stream_t s)
    STUB(dY8a, X8a, dWa, Ma, lda_a, ldb_a, ldc_a, amax_a, xamax_a, dY8b, X8b, dWb, Mb, lda_b, ldb_b, ldc_b, amax_b, xamax_b, N, K, accumulate, ws,
         ws_bytes, s)
extern "C" int nbest_colsum(const void* X, float* out, int64_t M, int64_t N, int64_t ld, int dtype, int accumulate, void* ws, size_t ws_bytes,
                            nbest_stream_t s) STUB(X, out, M, N, ld, dtype, accumulate, ws, ws_bytes, s)
extern "C" int nbest_head_gate_fwd(const void* in, int64_t ld_in, void* out, int64_t ld_out, const float* gate, int64_t M, int heads, int d,
                                   int dtype, nbest_stream_t s) STUB(in, ld_in, out, ld_out, gate, M, heads, d, dtype, s)
extern "C" int nbest_head_gate_bwd(const void* ctx, void* dctx, const float* gate, float* dgate, int B, int S, int heads, int d, int dtype,
                                   nbest_stream_t s) STUB(ctx, dctx, gate, dgate, B, S, heads, d, dtype, s)
extern "C" int nbest_embed_ln_fwd(const int64_t* ids, const int64_t* seg, const int64_t* pos, const void* word, const void* type, const void* ptab,
                                  const float* gamma, const float* beta, void* out, float* stats, int64_t M, int H, float eps, int dtype,
                                  float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t s)
    STUB(ids, seg, pos, word, type, ptab, gamma, beta, out, stats, M, H, eps, dtype, drop_p, seed, drop_stream, s)
extern "C" int nbest_embed_ln_fwd_adv(const int64_t* ids, const int64_t* seg, const int64_t* pos, const void* word, const void* type,
                                      const void* ptab, const float* gamma, const float* beta, const float* delta, void* out, float* stats,
                                      int64_t M, int H, float eps, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t s)
    STUB(ids, seg, pos, word, type, ptab, gamma, beta, delta, out, stats, M, H, eps, dtype, drop_p, seed, drop_stream, s)
extern "C" int nbest_embed_ln_fwd_interp(const int64_t* ids, const int64_t* base_ids, const float* alpha, const int64_t* seg, const int64_t* pos,
                                         const void* word, const void* type, const void* ptab, const float* gamma, const float* beta, void* out,
                                         float* stats, int B, int S, int H, float eps, int dtype, float drop_p, uint64_t seed,
                                         uint32_t drop_stream, nbest_stream_t s)
    STUB(ids, base_ids, alpha, seg, pos, word, type, ptab, gamma, beta, out, stats, B, S, H, eps, dtype, drop_p, seed, drop_stream, s)
extern "C" int nbest_embed_ln_bwd(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                                  const void* type, const void* ptab, const float* gamma, const float* stats, const void* dout, float* dword,
                                  float* dtype_tab, float* dptab, float* dgamma, float* dbeta, int B, int S, int H, int n_types, int dtype,
                                  int64_t word_pad_id, int64_t pos_pad_id, int accumulate, int tables_accumulate, float drop_p, uint64_t seed,
                                  uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t s)
    STUB(ids, seg, pos, perm, word, type, ptab, gamma, stats, dout, dword, dtype_tab, dptab, dgamma, dbeta, B, S, H, n_types, dtype, word_pad_id,
         pos_pad_id, accumulate, tables_accumulate, drop_p, seed, drop_stream, ws, ws_bytes, s)
extern "C" int nbest_embed_ln_bwd_adv(const int64_t* ids, const int64_t* seg, const int64_t* pos, const int32_t* perm, const void* word,
                                      const void* type, const void* ptab, const float* gamma, const float* stats, const float* delta,
                                      const void* dout, float* dword, float* dtype_tab, float* dptab, float* dgamma, float* dbeta, int B, int S,
                                      int H, int n_types, int dtype, int64_t word_pad_id, int64_t pos_pad_id, int accumulate,
                                      int tables_accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes,
                                      nbest_stream_t s)
    STUB(ids, seg, pos, perm, word, type, ptab, gamma, stats, delta, dout, dword, dtype_tab, dptab, dgamma, dbeta, B, S, H, n_types, dtype,
         word_pad_id, pos_pad_id, accumulate, tables_accumulate, drop_p, seed, drop_stream, ws, ws_bytes, s)

int nbest_internal_layernorm_fwd8(const void* x, const float* gamma, const float* beta, void* y, void* y8, float* stats, int64_t M, int H,
                                  float eps, int dtype, nbest_stream_t s, const uint32_t* a_prev, uint32_t* a_new)
    STUB(x, gamma, beta, y, y8, stats, M, H, eps, dtype, s, a_prev, a_new)
int nbest_internal_layernorm_bwd8(const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_drop, float* dgamma,
                                  float* dbeta, float* dbias, int64_t M, int H, int dtype, int accumulate, float drop_p, uint64_t seed,
                                  uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t s, Fp8Grad f8)
    STUB(dy, x, stats, gamma, dx, dx_drop, dgamma, dbeta, dbias, M, H, dtype, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, s, f8)
int nbest_internal_rows_drop_res(const void* x, int64_t ldx, const void* R, int64_t ldr, void* y, int64_t ldy, int64_t rows, int N,
                                 int64_t row_mul, int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, hipStream_t s)
    STUB(x, ldx, R, ldr, y, ldy, rows, N, row_mul, dtype, drop_p, seed, drop_stream, s)
void nbest_internal_rowred_batch_begin() { TRACE(); }
void nbest_internal_rowred_batch_abort() { TRACE(); }
int nbest_internal_rowred_batch_flush(hipStream_t s) STUB(s)
int nbest_internal_attention_fwd8(const void* qkv, const uint8_t* key_mask, void* ctx, void* ctx8, float* lse, int B, int S, int heads, int d,
                                  int dtype, float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t s, uint32_t* keep,
                                  const uint32_t* a_prev, uint32_t* a_new)
    STUB(qkv, key_mask, ctx, ctx8, lse, B, S, heads, d, dtype, drop_p, seed, drop_stream, s, keep, a_prev, a_new)
int nbest_internal_attention_bwd8(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx, const float* lse, void* dqkv,
                                  float* dbias, int accumulate, void* ws, size_t ws_bytes, int B, int S, int heads, int d, int dtype,
                                  float drop_p, uint64_t seed, uint32_t drop_stream, nbest_stream_t s, Fp8Grad f8, const uint32_t* keep)
    STUB(qkv, key_mask, ctx, dctx, lse, dqkv, dbias, accumulate, ws, ws_bytes, B, S, heads, d, dtype, drop_p, seed, drop_stream, s, f8, keep)
int nbest_attention_cls_fwd_internal(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const uint8_t* key_mask, void* ctx, int64_t ldctx,
                                     int B, int S, int heads, int d, int dtype, nbest_stream_t s, float drop_p, uint64_t seed,
                                     uint32_t drop_stream)
    STUB(q, ldq, kv, ldkv, key_mask, ctx, ldctx, B, S, heads, d, dtype, s, drop_p, seed, drop_stream)
int nbest_internal_attention_cls_bwd(const void* qkv, const uint8_t* key_mask, const void* ctx, const void* dctx, void* dqkv, float* dbias,
                                     int accumulate, void* ws, size_t ws_bytes, int B, int S, int heads, int d, int dtype, float drop_p,
                                     uint64_t seed, uint32_t drop_stream, nbest_stream_t s)
    STUB(qkv, key_mask, ctx, dctx, dqkv, dbias, accumulate, ws, ws_bytes, B, S, heads, d, dtype, drop_p, seed, drop_stream, s)
int nbest_internal_attention_cls_probs(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const uint8_t* key_mask, float* probs,
                                       int64_t ldp, int B, int S, int heads, int d, int dtype, nbest_stream_t s)
    STUB(q, ldq, kv, ldkv, key_mask, probs, ldp, B, S, heads, d, dtype, s)
int nbest_internal_amax_bf16(const void* x, int64_t n, uint32_t* out, hipStream_t s) STUB(x, n, out, s)
int nbest_internal_cast_bf16_to_fp8(const void* src, void* dst, int64_t n, const uint32_t* a_prev, uint32_t* a_new, hipStream_t s)
    STUB(src, dst, n, a_prev, a_new, s)

// ---- the descriptors and the calls -----------------------------------------------------------------------------------------------
namespace {
template <class T> T* fake(size_t a) { return (T*)a; }
enum { F32, BF16, FP8_CALIB, FP8 };   // fp8: the forward and the backward on the fp8 GEMMs; its calibration pass: the bf16 GEMMs + amax records

struct Case {
  int mode = NBEST_WGRAD_GROUP_PLAN, prec = BF16, H = 768, L = 3, cls_top = 0, first_trainable = 0, no_input_grad = 0, no_param_grad = 0;
  int accumulate = 0, chunk = 0 /* layers per backward call; 0: the whole range */, with_embeddings = 1, events = 64;
  int gate = 0 /* 1: head_gate + head_gate_grad, 2: head_gate + head_gate_stash */, emb_delta = 0, interp = 0, transposed = 1;
  float hidden_drop = 0.1f;
  bool pair_fits = true, skip = false;
};

void run(const Case& c) {
  g_pair_fits = c.pair_fits;
  std::vector<nbest_layer_offsets> lo(c.L);
  const int64_t H = c.H, F = 4 * H;
  int64_t off = 1000 * H;
  for (auto& o : lo) {
    int64_t* f = &o.wqkv;
    const int64_t n[12] = {3 * H * H, 3 * H, H * H, H, H, H, F * H, F, H * F, H, H, H};
    for (int i = 0; i < 12; ++i) { f[i] = off; off += n[i]; }
  }
  std::vector<uint8_t> skip((size_t)4 * c.L, 0);
  for (size_t i = 0; i < skip.size(); ++i) skip[i] = (i % 3 == 1) || i / 4 == 1 || i == skip.size() - 4;   // layer 1 whole, the top QKV, every third
  std::vector<void*> ev(c.events);
  for (int i = 0; i < c.events; ++i) ev[i] = fake<void>(0xE000 + i);
  nbest_encoder_desc d = {};
  d.dtype = c.prec == F32 ? NBEST_F32 : NBEST_BF16;
  d.B = 4; d.S = 128; d.H = c.H; d.L = c.L; d.heads = c.H / 64; d.F = (int)F;
  d.vocab = 1000; d.max_pos = 512; d.n_types = 2;
  d.ln_eps = 1e-12f; d.hidden_drop = c.hidden_drop; d.attn_drop = 0.1f;
  d.word_pad_id = 0; d.pos_pad_id = -1;
  d.off_word = 0; d.off_pos = 400 * H; d.off_type = 990 * H; d.off_emb_ln_g = 995 * H; d.off_emb_ln_b = 996 * H;
  d.layers_host = lo.data(); d.seed = 77; d.drop_stream_base = 40;
  d.wgrad_events_n = c.events; d.wgrad_events = c.events ? ev.data() : nullptr;
  d.wpk = fake<void>(0x2000000000); d.wpkt = fake<void>(0x2100000000);
  d.word_perm = fake<int32_t>(0x2200000000);
  if (c.prec >= FP8_CALIB) {
    d.w8 = fake<void>(0x3000000000); d.w8_inv_scale = fake<float>(0x3100000000); d.w8t = fake<void>(0x3200000000);
    d.w8p = fake<void>(0x3300000000); d.w8tp = fake<void>(0x3400000000);
    d.gamax_prev = fake<uint32_t>(0x3500000000); d.gamax_new = fake<uint32_t>(0x3600000000);
    d.aamax_prev = fake<uint32_t>(0x3700000000); d.aamax_new = fake<uint32_t>(0x3800000000);
    d.fp8_act = d.fp8_bwd = c.prec == FP8;
  }
  d.cls_top = c.cls_top; d.first_trainable = c.first_trainable; d.no_input_grad = c.no_input_grad; d.no_param_grad = c.no_param_grad;
  if (c.emb_delta) d.emb_delta = fake<float>(0x3900000000);
  if (c.skip) d.wgrad_skip_host = skip.data();
  if (c.gate) d.head_gate = fake<float>(0x3A00000000);
  if (c.gate == 1) d.head_gate_grad = fake<float>(0x3B00000000);
  d.head_gate_stash = c.gate == 2;
  if (c.interp) { d.base_ids = fake<int64_t>(0x3C00000000); d.alpha = fake<float>(0x3D00000000); }
  d.wgrad_group = c.mode;

  printf("case mode %d prec %d H %d L %d cls_top %d hidden_drop %g pair_fits %d first_trainable %d no_input_grad %d no_param_grad %d skip %d gate %d "
         "emb_delta %d interp %d accumulate %d chunk %d with_embeddings %d events %d transposed %d\n",
         c.mode, c.prec, c.H, c.L, c.cls_top, c.hidden_drop, (int)c.pair_fits, c.first_trainable, c.no_input_grad, c.no_param_grad, (int)c.skip,
         c.gate, c.emb_delta, c.interp, c.accumulate, c.chunk, c.with_embeddings, c.events, c.transposed);
  const size_t act_bytes = nbest_encoder_act_bytes(&d), ws_bytes = nbest_encoder_ws_bytes(&d);
  printf(" act_bytes %zu ws_bytes %zu launches_per_layer %d\n", act_bytes, ws_bytes, nbest_encoder_wgrad_launches_per_layer(&d));
  const void* wts = fake<void>(0x1000000000);
  const void* wts_t = c.transposed ? fake<void>(0x1100000000) : nullptr;
  const float* prm = fake<float>(0x1200000000);
  float* grad = fake<float>(0x1300000000);
  const int64_t *ids = fake<int64_t>(0x1400000000), *seg = fake<int64_t>(0x1410000000), *pos = fake<int64_t>(0x1420000000);
  const uint8_t* key_mask = fake<uint8_t>(0x1430000000);
  void *act = fake<void>(0x4000000000), *ws = fake<void>(0x6000000000), *dhidden = fake<void>(0x1500000000), *stream = fake<void>(0x57);
  void* hidden = nullptr;
  int rc = nbest_encoder_forward(&d, wts, prm, ids, seg, pos, key_mask, act, act_bytes, ws, ws_bytes, &hidden, stream);
  printf(" forward -> %d hidden %#zx\n", rc, (size_t)hidden);
  const int step = c.chunk ? c.chunk : c.L;
  for (int end = c.L; end > c.first_trainable || end == c.L; end -= step) {
    const int begin = end - step > c.first_trainable ? end - step : c.first_trainable;
    int32_t plan[4096];
    const int n = nbest_encoder_wgrad_plan(&d, begin, end, plan, 4096);
    printf(" plan [%d, %d):", begin, end);
    for (int i = 0; i < n && i < 4096; ++i) printf(" %d", plan[i]);
    printf(" (%d)\n", n);
    rc = nbest_encoder_backward(&d, wts, wts_t, prm, c.no_param_grad ? nullptr : grad, ids, seg, pos, key_mask, act, act_bytes, dhidden, ws, ws_bytes,
                                c.accumulate, begin, end, c.with_embeddings && begin == c.first_trainable, stream);
    printf(" backward [%d, %d) -> %d\n", begin, end, rc);
    if (begin == end) break;
  }
}
}  // namespace

int main() {
  const int modes[4] = {NBEST_WGRAD_GROUP_PLAN, NBEST_WGRAD_GROUP_NEVER, NBEST_WGRAD_GROUP_ALWAYS, NBEST_WGRAD_GROUP_WINDOW};
  // every schedule x pairing x cls_top, under: the precisions, hidden dropout, L odd / even, accumulate, whole range / 2-layer chunks
  for (int mode : modes)
    for (int pf = 0; pf < 2; ++pf)
      for (int cls = 0; cls < 2; ++cls) {
        Case b;
        b.mode = mode; b.pair_fits = pf; b.cls_top = cls;
        for (int prec = F32; prec <= FP8; ++prec)
          for (float hd : {0.f, 0.1f})
            for (int L : {3, 4})
              for (int acc = 0; acc < 2; ++acc)
                for (int chunk : {0, 2}) {
                  Case c = b;
                  c.prec = prec; c.hidden_drop = hd; c.L = L; c.accumulate = acc; c.chunk = chunk;
                  run(c);
                }
        // one option at a time on top of it (bf16; L = 4 and the odd L = 3, whole and in chunks where the option changes the schedule)
        for (int L : {3, 4})
          for (int chunk : {0, 2}) {
            Case c = b;
            c.L = L; c.chunk = chunk;
            Case v = c; v.first_trainable = 1; v.with_embeddings = 0; run(v);
            v.no_input_grad = 1; run(v);
            v = c; v.skip = true; run(v);
            v.first_trainable = 1; v.no_input_grad = 1; v.with_embeddings = 0; run(v);
            v = c; v.no_param_grad = 1; v.with_embeddings = 0; run(v);
            v.gate = 1; run(v);
            v = c; v.gate = 2; run(v);
            v.first_trainable = 2; v.with_embeddings = 0; run(v);
            v = c; v.gate = 1; run(v);                       // refused: the parameter gradients need the gated context
            v = c; v.emb_delta = 1; run(v);
            v = c; v.with_embeddings = 0; run(v);
            v = c; v.events = 0; run(v);
            v = c; v.events = 7; run(v);                     // fewer events than pairs: the records stop, the launches do not
            v = c; v.transposed = 0; run(v);
            v = c; v.prec = F32; v.interp = 1; v.no_param_grad = 1; v.with_embeddings = 0; run(v);
          }
        Case c = b; c.L = 12; run(c);
        c.chunk = 2; run(c);
        c.skip = true; run(c);
        // 256 / 1024: 12 tiles per layer - L = 6 cuts a window at the 16-entry table, L = 10 flushes for want of a free buffer set
        for (int L : {6, 10, 12}) {
          Case s = b; s.H = 256; s.L = L; run(s);
          s.skip = true; run(s);
          s.skip = false; s.chunk = 2; run(s);
        }
        Case f = b; f.H = 256; f.L = 10; f.prec = FP8; run(f);
      }
  // refusals of the backward's own checks, in their order
  Case r; r.first_trainable = 1; run(r);                     // with_embeddings under first_trainable > 0
  r = Case(); r.no_param_grad = 1; run(r);                   // no_param_grad with with_embeddings
  r = Case(); r.cls_top = 1; r.prec = FP8; run(r);
  r = Case(); r.gate = 2; r.emb_delta = 1; run(r);
  return 0;
}
