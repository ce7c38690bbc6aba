// The whole encoder stack behind one C-ABI call each way (forward / backward): every kernel of
// every layer is enqueued on the caller's stream from C++, so a training step costs a handful of
// Python->C transitions instead of ~400, and the sequence is hipGraph-capturable (no allocation, no
// synchronisation, no default-stream work inside).
//
// Activation stash `act` (written by forward, read by backward; act_layout), T = dtype, K = desc.first_trainable:
//   X[K..L]   [M][H] T      X[0] = embedding output, X[l+1] = output of layer l
//   emb_stats [M][2] f32    (K == 0 only)
//   per layer K..L-1 (stashed_layer):
//              qkv [M][3H] T | ctx [M][H] T | lse [B*heads*S] f32 | r1 [M][H] T | st1 [M][2] f32 | x1 [M][H] T |
//              u = gelu'(pre-activation) [M][F] (fp32, or 8-bit fixed point in the bf16 path) | hact [M][F] T | r2 [M][H] T |
//              st2 [M][2] f32 | keep: the attention-dropout keep words (bf16) |
//              fp8 forward (desc.w8) only: x8 | ctx8 | x18 [M][H] e4m3, h8 [M][F] e4m3, the copies of the layer's four GEMM inputs
// Scratch `ws` (ws_layout): dR | dRd | dB1 | dctx [M][H] T, dBig [M][F] T, dqkv [M][3H] T, (grouped weight gradients: the dY buffers
//   of the group positions; weight gradients in rolling windows: the dY buffer sets the layers rotate over, WsLayout::gset), four regions of column-reduction
//   partials, split-K slabs, embedding-backward buffer, f8 (bf16: the e4m3 copies of ONE layer - forward: a frozen layer's GEMM
//   inputs, backward: the gradients the fp8 dgrads read), fz (K > 0: X0 | X1 | emb_stats | lse | st1 | st2 | u).
//   Layers 0..K-1 are not stashed: their forward runs on fz plus the backward's layer-gradient buffers, which are idle
//   during a forward (frozen_layer).
// Head gates (desc.head_gate): the forward's gated copy of a layer's ctx borrows dctx; the stash keeps the un-gated ctx.
//   desc.head_gate_stash (training under the gates): the stash ends with gctx [M][H] T per layer K..L-1, the gated copy - the X operand
//   of the attention-output weight gradient, which a deferred (grouped / window) launch reads long after dctx is reused.  ctx stays
//   un-gated (the attention backward's O); a frozen layer gates its scratch ctx in place; dctx is not borrowed.
// Inference workspace: infer_layout, below.
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
// the next `bytes` of a layout under construction (o: its size so far): their offset
static inline size_t take(size_t& o, size_t bytes) { const size_t at = o; o += bytes; return at; }

// the buffer sizes every layout is made of (256-byte aligned): [M][H], [M][F], [M][3H] of the dtype, [M][H] and [M][F] of one
// byte per element, a LayerNorm's [M][2] statistics, an attention's [B heads S] log-sum-exp
struct Sizes {
  size_t esz, MH, MF, M3H, MH8, MF8, st, lse;
  int64_t M;
};

static Sizes sizes(const nbest_encoder_desc* d) {
  Sizes z;
  z.esz = d->dtype == NBEST_BF16 ? 2 : 4;
  z.M = (int64_t)d->B * d->S;
  const size_t MHe = (size_t)z.M * d->H, MFe = (size_t)z.M * d->F;
  z.MH = al(MHe * z.esz); z.MF = al(MFe * z.esz); z.M3H = al(3 * MHe * z.esz);
  z.MH8 = al(MHe); z.MF8 = al(MFe);
  z.st = al((size_t)z.M * 2 * sizeof(float));
  z.lse = al((size_t)d->B * d->heads * d->S * sizeof(float));
  return z;
}

struct ActLayout {
  size_t X, emb_stats, layer0, layer_stride;
  size_t o_qkv, o_ctx, o_lse, o_r1, o_st1, o_x1, o_u, o_hact, o_r2, o_st2;
  size_t o_x8, o_ctx8, o_x18, o_h8;   // fp8 forward ("fp8w"): e4m3 copies of the four GEMM inputs of the layer, kept for the fp8 weight gradients
  size_t o_keep, keep_bytes;          // bf16, S <= 256: attention-dropout keep words of the layer (forward -> backward)
  size_t gctx, gctx_stride;           // desc.head_gate_stash: the gated contexts [L - K][M][H], after every layer block (else 0 bytes)
  size_t total;
  int K;                              // first stashed layer (desc.first_trainable)
};

static int first_trainable(const nbest_encoder_desc* d) { return d->first_trainable < 0 ? 0 : (d->first_trainable > d->L ? d->L : d->first_trainable); }

// training under head gates: the gated context of every stashed layer is kept (include/nbest_hip.h, head_gate)
static bool gate_stashed(const nbest_encoder_desc* d) { return d->head_gate && d->head_gate_stash; }

static ActLayout act_layout(const nbest_encoder_desc* d, const Sizes& z) {
  ActLayout a;
  const bool bf16 = d->dtype == NBEST_BF16;
  a.K = first_trainable(d);
  size_t o = 0, p = 0;
  a.X = take(o, (size_t)(d->L + 1 - a.K) * z.MH);
  a.emb_stats = take(o, a.K ? 0 : z.st);
  a.layer0 = o;
  a.o_qkv = take(p, z.M3H); a.o_ctx = take(p, z.MH); a.o_lse = take(p, z.lse);
  a.o_r1 = take(p, z.MH); a.o_st1 = take(p, z.st); a.o_x1 = take(p, z.MH);
  a.o_u = take(p, bf16 ? z.MF8 : z.MF);   // GELU': 8 bits per element in the bf16 path
  a.o_hact = take(p, z.MF); a.o_r2 = take(p, z.MH); a.o_st2 = take(p, z.st);
  a.keep_bytes = bf16 ? nbest_internal_attention_keep_bytes(d->B, d->S, d->heads) : 0;
  a.o_keep = take(p, al(a.keep_bytes));
  a.o_x8 = a.o_ctx8 = a.o_x18 = a.o_h8 = 0;
  if (d->w8) {   // only the fp8 mode pays for them (+ (3 H + F) bytes per token and layer)
    a.o_x8 = take(p, z.MH8); a.o_ctx8 = take(p, z.MH8); a.o_x18 = take(p, z.MH8); a.o_h8 = take(p, z.MF8);
  }
  a.layer_stride = p;
  o += (size_t)(d->L - a.K) * p;
  a.gctx = take(o, gate_stashed(d) ? (size_t)(d->L - a.K) * z.MH : 0);   // last: every other offset is what it is without it
  a.gctx_stride = z.MH;
  a.total = o;
  return a;
}

struct WsLayout {
  size_t dR, dRd, dB1, dctx, dBig, dqkv, red, slab, slab_bytes, red_bytes, emb, emb_bytes, f8, f8_bytes, total;
  // deferred weight gradients (grouped or in windows): the four dY tensors of a layer - dRd after LN2, dBig, dRd after LN1, dqkv - per
  // position of the layer in its group / per buffer set of the windows; set 0 shares dRd, dBig and dqkv above
  size_t gset[8][4];
  size_t fz_x0, fz_x1, fz_emb_stats, fz_lse, fz_st1, fz_st2, fz_u;   // forward of the frozen layers 0..K-1 (first_trainable = K > 0)
};

// a weight gradient dW[rows][cols] (fp32) = dY[tokens][rows]^T . X[tokens][cols] on split-K slabs: everything of the problem but
// its pointers, `accumulate` and the workspace.  The workspace sizes, the pairing rule and the launches all take their plan from here.
static nbest_gemm_args wgrad_args(int dtype, int64_t rows, int64_t cols, int64_t tokens) {
  nbest_gemm_args g = {};
  g.M = rows; g.N = cols; g.K = tokens; g.lda = rows; g.ldb = cols; g.ldc = cols;
  g.trans_a = g.trans_b = 1; g.epilogue = NBEST_EPI_F32_SPLITK; g.dtype = dtype;
  return g;
}

// slab bytes of the QKV + attention-output gradients of a layer as ONE launch (bf16 or e4m3 operands); 0: the pair does not fit
static size_t wgrad_pair_bytes(const nbest_encoder_desc* d, bool fp8) {
  const int64_t H = d->H, M = (int64_t)d->B * d->S;
  if (fp8) return nbest_wgrad_fp8_pair_ws_bytes(3 * H, H, H, M);
  const nbest_gemm_args g1 = wgrad_args(NBEST_BF16, 3 * H, H, M), g2 = wgrad_args(NBEST_BF16, H, H, M);
  return nbest_wgrad_pair_ws_bytes(&g1, &g2);
}

static size_t max_splitk_bytes(const nbest_encoder_desc* d, int64_t M) {
  size_t mx = 0;
  const int64_t shapes[4][2] = {{3 * (int64_t)d->H, d->H}, {d->H, d->H}, {d->F, d->H}, {d->H, d->F}};
  for (int i = 0; i < 4; ++i) {
    const nbest_gemm_args g = wgrad_args(d->dtype, shapes[i][0], shapes[i][1], M);
    mx = std::max(mx, nbest_gemm_ws_bytes(&g));
    if (d->dtype == NBEST_BF16 && shapes[i][0] % 256 == 0 && shapes[i][1] % 256 == 0)   // fp8 weight gradients: own split plan
      mx = std::max(mx, nbest_wgrad_fp8_ws_bytes(shapes[i][0], shapes[i][1], M));
  }
  if (d->dtype == NBEST_BF16) mx = std::max(mx, std::max(wgrad_pair_bytes(d, false), wgrad_pair_bytes(d, true)));
  return mx;
}

// the attention-output weight gradient of a layer is issued together with the QKV gradient (nbest_wgrad_pair / nbest_wgrad_fp8_pair:
// 3 weight-gradient launches per layer instead of 4) when the pair fits one 256 x 256 split-K launch
static bool wgrad_paired(const nbest_encoder_desc* d, bool f8b) { return d->dtype == NBEST_BF16 && wgrad_pair_bytes(d, f8b) > 0; }

// ---- grouped weight gradients: the plan ----------------------------------------------------------------------------------------
// Launch-cost model of the 256 x 256 weight-gradient kernel (us), fitted on the FFN-down gradient alone, cold operands, at K = 32 768,
// 65 536 and 131 072 token rows: a launch costs kWgA + kWgB per 32-row K stage a workgroup walks, per round of 256
// workgroups; a split-K reduce launch costs kWgRed.
constexpr double kWgA = 24.5, kWgB = 0.705, kWgRed = 12.7;
static double wgrad_splitk_us(int64_t rows, int64_t cols, int64_t M) {
  const nbest_gemm_args g = wgrad_args(NBEST_BF16, rows, cols, M);
  const size_t ws = nbest_gemm_ws_bytes(&g);
  const int64_t splits = ws ? (int64_t)(ws / ((size_t)rows * cols * sizeof(float))) : 1;
  const int64_t stages = ((M + splits - 1) / splits + 31) / 32, wgs = (rows / 256) * (cols / 256) * splits;
  return kWgA + kWgB * (double)(stages * ((wgs + 255) / 256)) + (splits > 1 ? kWgRed : 0.0);
}
// ---- rolling windows (NBEST_WGRAD_GROUP_WINDOW): the schedule ----------------------------------------------------------------------------
// The non-skipped gradients of the layers of a backward call's range form a queue of 256 x 256 tiles: the highest layer first, QKV |
// attention-out | FFN-up | FFN-down within a layer, a matrix's tiles in the order of nbest_wgrad_group.  A launch (nbest_wgrad_window)
// takes the next 256 pending tiles whichever layers they belong to, as soon as 256 are pending; the rest goes out at the end of the
// call, so a call leaves all of its gradients written.  Where it saves a whole round, the QKV + attention-out pair of the range's lowest
// layer is peeled off the queue and runs as the split-K launches of mode NEVER (one pair launch where the two fit it).  A layer's dY tensors live until its last tile is launched:
// `sets` buffer sets in rotation (layer i of the range from the top takes set i % sets); a window is also cut short where the table
// is full (kWinEntries) and the queue is flushed where the next layer would find no free set (skipped matrices make layers small).
constexpr int kWinEntries = 16, kMaxSets = 8, kWinTiles = 256;
// a window of more than 216 tiles against the launch of 216: 1.023 for lone launches (profiles/wgrad_window_fit.txt), 1.078 inside the
// training step (profiles/wgrad_window_ab.txt) - the plan decides for the step, so it takes the in-step figure
constexpr double kWgFull = 1.078;
struct WinEntry { int layer, j, first, count; };
struct WinLaunch { int after_layer, tiles, n; WinEntry e[kWinEntries]; };   // issued at the end of layer `after_layer`
struct WinPlan {
  int sets = 0, peel_layer = -1, max_live = 0;   // max_live: most layers with unlaunched tiles while a further layer writes its dY
  std::vector<WinLaunch> launches;
};
static void matrix_tiles(const nbest_encoder_desc* d, int t[4]) {
  const int h = d->H / 256, f = d->F / 256;
  t[0] = 3 * h * h; t[1] = h * h; t[2] = f * h; t[3] = h * f;
}
// skip: [4 L] flags as desc.wgrad_skip_host or NULL; peel: the schedule of a call (false: only the buffer sets are asked for)
static WinPlan window_plan(const nbest_encoder_desc* d, int layer_begin, int layer_end, const uint8_t* skip, bool all_skipped, bool peel,
                           int sets) {
  WinPlan wp;
  wp.sets = sets;
  int t[4];
  matrix_tiles(d, t);
  auto live = [&](int l, int j) { return !all_skipped && !(skip && skip[4 * l + j]); };
  int64_t total = 0;
  for (int l = layer_begin; l < layer_end; ++l)
    for (int j = 0; j < 4; ++j) total += live(l, j) ? t[j] : 0;
  if (peel && layer_begin < layer_end) {
    const int64_t pair = (live(layer_begin, 0) ? t[0] : 0) + (live(layer_begin, 1) ? t[1] : 0);
    if (pair > 0 && (total - pair + kWinTiles - 1) / kWinTiles < (total + kWinTiles - 1) / kWinTiles) wp.peel_layer = layer_begin;
  }
  std::vector<WinEntry> q;   // pending, front at `head`
  size_t head = 0;
  int64_t pending = 0;
  auto emit = [&](int after) {
    WinLaunch w = {};
    w.after_layer = after;
    while (head < q.size() && w.tiles < kWinTiles && w.n < kWinEntries) {
      WinEntry& f = q[head];
      const int c = std::min(f.count, kWinTiles - w.tiles);
      w.e[w.n++] = WinEntry{f.layer, f.j, f.first, c};
      w.tiles += c; f.first += c; f.count -= c; pending -= c;
      if (f.count == 0) ++head;
    }
    wp.launches.push_back(w);
  };
  for (int l = layer_end - 1; l >= layer_begin; --l) {
    const int n_live = head < q.size() ? q[head].layer - l : 0;   // layers l + 1 .. q[head].layer still have tiles pending
    wp.max_live = std::max(wp.max_live, n_live);
    if (n_live >= sets)   // no free set for this layer: everything pending goes out now, at the end of layer l + 1
      while (pending > 0) emit(l + 1);
    for (int j = 0; j < 4; ++j)
      if (live(l, j) && !(l == wp.peel_layer && j < 2)) { q.push_back(WinEntry{l, j, 0, t[j]}); pending += t[j]; }
    while (pending >= kWinTiles) emit(l);
  }
  while (pending > 0) emit(layer_begin);
  return wp;
}
static bool window_shapes_ok(const nbest_encoder_desc* d) {
  if (d->dtype != NBEST_BF16 || d->w8 || d->H % 256 || d->F % 256) return false;
  return (4 * (int64_t)d->H * d->H + 2 * (int64_t)d->H * d->F) / (256 * 256) <= kWinTiles;
}
// The window schedule of the whole trainable range, nothing skipped, built once: its buffer sets (a shorter range runs a prefix of the
// same schedule; skipped matrices are covered by the flush rule of window_plan) and its model time (us).  The time is that of ONE call
// over the whole range: a backward in chunks (the 2-layer chunks of the data-parallel reducer) flushes per call and runs mode ALWAYS's
// 216-tile launches at bert-base tile counts, 256 + 128 tiles per chunk at 192 tiles per layer - the prediction does not hold there.
struct WindowModel { int sets; double us; };
static WindowModel window_model(const nbest_encoder_desc* d) {
  const int64_t H = d->H, M = (int64_t)d->B * d->S;
  const WinPlan wp = window_plan(d, first_trainable(d), d->L, nullptr, false, true, kMaxSets);   // (the peel does not change max_live)
  const double round = kWgA + kWgB * (double)((M + 31) / 32);
  double us = 0.0;
  if (wp.peel_layer >= 0) us = wgrad_paired(d, false) ? wgrad_splitk_us(4 * H, H, M) : wgrad_splitk_us(3 * H, H, M) + wgrad_splitk_us(H, H, M);
  for (const WinLaunch& w : wp.launches) us += round * (w.tiles > 216 ? kWgFull : 1.0);
  return WindowModel{std::min(wp.max_live + 1, kMaxSets), us};
}

// How the weight gradients of this descriptor are launched (include/nbest_hip.h, desc.wgrad_group), resolved:
//   mode NEVER: every layer issues its split-K launches (gl = 0);  ALWAYS / the plan's grouping: gl layers per nbest_wgrad_group launch;
//   WINDOW: rolling windows over `sets` dY buffer sets (gl = 0).
// Grouping and windows need the bf16 path without the fp8 forward (whose backward has its own weight-gradient kernels) and whole
// 256 x 256 tiles.  The plan groups two layers when their tiles fit one round of the 256 CUs and the model above predicts at least 5 %
// less time than the three split-K launches + reduces of each layer; it takes the windows where the model predicts at least 5 % less
// than the better of those two over the trainable layers.  At small token counts the fixed cost of a launch dominates and the
// windows' extra pair launch keeps them out.
struct WgradMode { int mode, gl, sets; };
static WgradMode wgrad_mode(const nbest_encoder_desc* d) {
  const WgradMode never = {NBEST_WGRAD_GROUP_NEVER, 0, 0};
  if (d->wgrad_group == NBEST_WGRAD_GROUP_NEVER) return never;
  if (d->dtype != NBEST_BF16 || d->w8 || d->H % 256 || d->F % 256) return never;
  const int64_t H = d->H, F = d->F, M = (int64_t)d->B * d->S;
  const int64_t tiles = (4 * H * H + 2 * H * F) / (256 * 256);   // of one layer's four gradients
  if (d->wgrad_group == NBEST_WGRAD_GROUP_ALWAYS) return WgradMode{NBEST_WGRAD_GROUP_ALWAYS, 2 * tiles <= 256 ? 2 : 1, 0};
  if (d->wgrad_group == NBEST_WGRAD_GROUP_WINDOW)
    return window_shapes_ok(d) ? WgradMode{NBEST_WGRAD_GROUP_WINDOW, 0, window_model(d).sets} : never;
  const int nl = d->L - first_trainable(d);
  const double today = wgrad_splitk_us(4 * H, H, M) + wgrad_splitk_us(F, H, M) + wgrad_splitk_us(H, F, M);
  const double round = kWgA + kWgB * (double)((M + 31) / 32);
  if (window_shapes_ok(d) && nl > 0) {   // against the better of the other two modes, whichever of them the plan would take
    const int gl = 2 * tiles <= 256 ? 2 : 1;
    const WindowModel wm = window_model(d);
    if (wm.us < 0.95 * std::min(today * nl, round * ((nl + gl - 1) / gl))) return WgradMode{NBEST_WGRAD_GROUP_WINDOW, 0, wm.sets};
  }
  if (2 * tiles > 256 || !wgrad_paired(d, false)) return never;
  return round / 2.0 < 0.95 * today ? WgradMode{NBEST_WGRAD_GROUP_ALWAYS, 2, 0} : never;
}
// weight-gradient launches = event pairs (desc.wgrad_events) per layer: one when the gradients are deferred to a grouped or window launch
static int wgrad_launches_per_layer(const WgradMode& wm, bool paired) { return (wm.gl > 0 || wm.sets > 0) ? 1 : paired ? 3 : 4; }
// wm: wgrad_mode(d), resolved once by the caller
static WsLayout ws_layout(const nbest_encoder_desc* d, const Sizes& z, const WgradMode& wm) {
  WsLayout w;
  const int64_t M = z.M;
  size_t o = 0;
  w.dR = take(o, z.MH); w.dRd = take(o, z.MH); w.dB1 = take(o, z.MH); w.dctx = take(o, z.MH);
  w.dBig = take(o, z.MF); w.dqkv = take(o, z.M3H);
  static_assert(sizeof(w.gset) / sizeof(w.gset[0]) == kMaxSets, "one row per buffer set");
  for (int s = 0; s < kMaxSets; ++s) { w.gset[s][0] = w.dRd; w.gset[s][1] = w.dBig; w.gset[s][2] = w.dRd; w.gset[s][3] = w.dqkv; }
  const int n_sets = wm.gl + wm.sets;   // one of the two is 0
  if (n_sets > 0) {
    w.gset[0][2] = take(o, z.MH);
    for (int s = 1; s < n_sets; ++s) { w.gset[s][0] = take(o, z.MH); w.gset[s][1] = take(o, z.MF); w.gset[s][2] = take(o, z.MH); w.gset[s][3] = take(o, z.M3H); }
  }
  const int64_t maxN = d->F > 3 * d->H ? d->F : 3 * d->H;
  w.red_bytes = al(nbest_rowred_ws_bytes(M, maxN));
  w.red_bytes = std::max(w.red_bytes, al(nbest_attention_bwd_ws_bytes(d->B, d->S, d->heads)));
  w.red_bytes = std::max(w.red_bytes, al((size_t)((M + 127) / 128) * 2 * d->F * sizeof(float)));   // fused column sums of the dU GEMM
  w.red = take(o, 4 * w.red_bytes);     // four regions: the partial rows of a layer's four producers live until its one finalize
  w.slab_bytes = al(max_splitk_bytes(d, M));
  // desc.cls_top: the top layer's gradients over K = B rows (whatever the flag says: it is set per call, the workspace is sized once)
  w.slab_bytes = std::max(w.slab_bytes, al(max_splitk_bytes(d, d->B)));
  w.slab = take(o, w.slab_bytes);
  w.emb_bytes = al(nbest_embed_bwd_ws_bytes(M, d->H));
  w.emb = take(o, w.emb_bytes);
  // fp8 forward: e4m3 copies of the GEMM inputs of ONE layer (x | ctx | x1: [M][H] bytes each, gelu(u): [M][F] bytes)
  // (backward, fp8 dgrads: dQ|dK|dV copy over the first three blocks, FFN gradient copy over the fourth, a fifth [M][H] block)
  w.f8_bytes = (d->dtype == NBEST_BF16) ? 4 * z.MH8 + z.MF8 : 0;
  w.f8 = take(o, w.f8_bytes);
  // frozen layers (first_trainable > 0): their forward runs without a stash, on the ping-pong layer inputs X0 | X1 and these
  // small buffers; qkv, ctx, r1, x1, r2, gelu(u) and the e4m3 copies reuse dqkv, dctx, dR, dRd, dB1, dBig and f8 above.
  // fp8 forward: the GELU' rows have no reader but the fp8 epilogue writes them (u, [M][F] bytes).
  w.fz_x0 = w.fz_x1 = w.fz_emb_stats = w.fz_lse = w.fz_st1 = w.fz_st2 = w.fz_u = o;
  if (first_trainable(d) > 0) {
    w.fz_x0 = take(o, z.MH); w.fz_x1 = take(o, z.MH); w.fz_emb_stats = take(o, z.st);
    w.fz_lse = take(o, z.lse); w.fz_st1 = take(o, z.st); w.fz_st2 = take(o, z.st);
    w.fz_u = take(o, d->w8 ? z.MF8 : 0);
  }
  w.total = o;
  return w;
}

// the forward of this pass runs its GEMMs in fp8: needs the activation amax history (fp8_act; without one the pass is a calibration
// pass on the bf16 GEMMs that records it)
static bool fp8_forward_active(const nbest_encoder_desc* d) {
  return d->dtype == NBEST_BF16 && d->w8 && d->w8_inv_scale && d->fp8_act && d->aamax_prev;
}
// the backward of this pass runs its dgrad / wgrad GEMMs in fp8 (same answer in the forward, which then leaves out the
// bf16 tensors only a bf16 backward would read, and in the backward)
static bool fp8_backward_active(const nbest_encoder_desc* d) {
  return fp8_forward_active(d) && d->fp8_bwd && d->w8t && d->gamax_prev && d->gamax_new;   // reads the forward's e4m3 activation copies
}

// train: a training entry point (the inference ones ignore head_gate_stash, as they ignore cls_top)
static int check_desc(const nbest_encoder_desc* d, bool train = true) {
  NB_CHECK(d && d->layers_host, NBEST_ERR_ARG, "encoder: null descriptor");
  NB_CHECK(d->dtype == NBEST_F32 || d->dtype == NBEST_BF16, NBEST_ERR_DTYPE, "encoder: bad dtype %d", d->dtype);
  NB_CHECK(d->B > 0 && d->S > 0 && d->L > 0 && d->heads > 0, NBEST_ERR_SHAPE, "encoder: bad shape");
  NB_CHECK(d->H == d->heads * 64, NBEST_ERR_SHAPE, "encoder: hidden %d != heads %d x 64", d->H, d->heads);
  // the reference never truncates (utils/bert_xlnet_inputs.py:87-94) and would index past the position table; fail up
  // front instead, before anything is enqueued (RoBERTa-family positions start at pad_id + 1)
  NB_CHECK(d->S + (d->pos_pad_id >= 0 ? (int)d->pos_pad_id + 1 : 0) <= d->max_pos, NBEST_ERR_SHAPE,
           "encoder: S=%d does not fit the position table (%d rows)", d->S, d->max_pos);
  NB_CHECK(d->S <= 512, NBEST_ERR_SHAPE, "encoder: S=%d > 512", d->S);
  if (d->dtype == NBEST_BF16)
    NB_CHECK(d->H % 128 == 0 && d->F % 128 == 0, NBEST_ERR_SHAPE, "encoder(bf16): H and F must be multiples of 128");
  if (d->w8) NB_CHECK(d->dtype == NBEST_BF16 && d->w8_inv_scale && d->H % 256 == 0 && d->H <= 1024 && d->F % 256 == 0, NBEST_ERR_SHAPE,
                      "encoder(fp8 forward): needs the bf16 path, inverse scales and H, F multiples of 256");
  NB_CHECK(0 <= d->first_trainable && d->first_trainable <= d->L, NBEST_ERR_ARG, "encoder: first_trainable %d outside [0, L=%d]",
           d->first_trainable, d->L);
  NB_CHECK(!d->base_ids == !d->alpha, NBEST_ERR_ARG, "encoder: interpolated embeddings need both base_ids and alpha (or neither)");
  // head_gate_stash: the gated context is kept in the stash, parameters train under the gates (frozen layers gate in place)
  if (train && d->head_gate_stash) {
    NB_CHECK(d->head_gate, NBEST_ERR_ARG, "encoder: head_gate_stash without head_gate");
    NB_CHECK(!d->w8, NBEST_ERR_ARG, "encoder: head_gate_stash is not supported with the fp8 forward (desc.w8)");
    NB_CHECK(!d->emb_delta, NBEST_ERR_ARG, "encoder: head_gate_stash is not supported with perturbed embeddings (emb_delta)");
    NB_CHECK(!d->base_ids && !d->alpha, NBEST_ERR_ARG, "encoder: head_gate_stash is not supported with interpolated embeddings (base_ids / alpha)");
    NB_CHECK(!d->no_param_grad, NBEST_ERR_ARG, "encoder: head_gate_stash is not supported with no_param_grad (it exists for the parameter gradients)");
    NB_CHECK(!d->head_gate_grad, NBEST_ERR_ARG, "encoder: head_gate_stash is not supported with head_gate_grad");
  }
  // head gates (desc.head_gate) without it: the gated context is a scratch copy the bf16 / fp32 attention-output GEMM reads - the fp8
  // forward's e4m3 copy of ctx comes out of the attention kernel, and a frozen layer's forward already lives in that scratch
  NB_CHECK(!d->head_gate || !d->w8, NBEST_ERR_ARG, "encoder: head_gate is not supported with the fp8 forward (desc.w8)");
  NB_CHECK(!d->head_gate || d->first_trainable == 0 || (train && d->head_gate_stash), NBEST_ERR_ARG, "encoder: head_gate needs first_trainable == 0 (got %d) or head_gate_stash", d->first_trainable);
  NB_CHECK(!d->head_gate_grad || d->head_gate, NBEST_ERR_ARG, "encoder: head_gate_grad without head_gate");
  // adversarial perturbation of the word rows (desc.emb_delta): the embedding kernels' _adv entry points, bf16 / fp32 forward, full stash
  NB_CHECK(!d->emb_delta || !d->w8, NBEST_ERR_ARG, "encoder: emb_delta is not supported with the fp8 forward (desc.w8)");
  NB_CHECK(!d->emb_delta || (!d->base_ids && !d->alpha), NBEST_ERR_ARG, "encoder: emb_delta is not supported with interpolated embeddings (base_ids / alpha)");
  NB_CHECK(!d->emb_delta || d->first_trainable == 0, NBEST_ERR_ARG, "encoder: emb_delta needs first_trainable == 0 (got %d): the perturbation "
           "is formed from the gradient w.r.t. trainable embeddings", d->first_trainable);
  return NBEST_OK;
}

// desc.cls_top (the top layer on the CLS rows only; include/nbest_hip.h): what the training entry points refuse it with.  The inference
// entry points ignore the field and do not come here.
static int check_cls_top(const nbest_encoder_desc* d) {
  if (!d->cls_top) return NBEST_OK;
  NB_CHECK(!d->w8, NBEST_ERR_ARG, "encoder: cls_top is not supported with the fp8 forward / backward (desc.w8)");
  NB_CHECK(!d->head_gate || d->head_gate_stash, NBEST_ERR_ARG, "encoder: cls_top is not supported with head_gate (the gate runs on the "
           "full-width context) unless head_gate_stash keeps the gated rows");
  NB_CHECK(!d->base_ids && !d->alpha, NBEST_ERR_ARG, "encoder: cls_top is not supported with interpolated embeddings (base_ids / alpha)");
  NB_CHECK(!d->no_param_grad, NBEST_ERR_ARG, "encoder: cls_top is not supported with no_param_grad");
  // (first_trainable == L is NOT refused: the forward then runs the top layer on the CLS rows of the frozen layers' scratch, and the heads of
  // an all-frozen encoder see the bits they see above a trainable one - tests/test_freeze_gpu.py holds their gradients to bit equality)
  NB_CHECK(d->S >= 2, NBEST_ERR_SHAPE, "encoder: cls_top needs S >= 2 (got %d)", d->S);
  return NBEST_OK;
}
static bool cls_layer_of(const nbest_encoder_desc* d, int l) { return d->cls_top && l == d->L - 1; }

// The flags of the grouped / window queue of a backward call that ends at layer_end: desc.wgrad_skip_host (NULL: none), plus - cls_top,
// layer_end == L - the top layer's attention-out, FFN-up and FFN-down gradients, which are plain launches over the B CLS rows.
static std::vector<uint8_t> queue_skip(const nbest_encoder_desc* d, int layer_end) {
  std::vector<uint8_t> s((size_t)4 * d->L, 0);
  if (d->wgrad_skip_host) std::copy(d->wgrad_skip_host, d->wgrad_skip_host + (size_t)4 * d->L, s.begin());
  if (d->cls_top && layer_end == d->L)
    for (int j = 1; j < 4; ++j) s[(size_t)4 * (d->L - 1) + j] = 1;
  return s;
}

struct Ptrs {
  const char* wts;   // matrices / tables, dtype
  const float* prm;  // fp32 master (biases, LayerNorm)
  size_t esz;
  const void* W(int64_t off) const { return wts + (size_t)off * esz; }
  const float* P(int64_t off) const { return prm + off; }
};

#define RUN(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

// ---- GEMM argument blocks ---------------------------------------------------------------------------------------------------------
// C[M][N] = A[M][K] . B[N][K]^T with both operands k-contiguous and every row packed (lda = ldb = K, ldc = N).  What a call adds
// (epilogue and its operands, other leading dimensions, dropout, column sums, the packed operand) it assigns by name.
static nbest_gemm_args gemm_nt(int dtype, const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K) {
  nbest_gemm_args g = {};
  g.A = A; g.B = B; g.C = C; g.dtype = dtype;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N;
  return g;
}

// the pre-packed image of the B operand (weight matrix at element offset `off` of `arena`; NULL arena: none).  bf16: the packed
// tiles serve the k-contiguous kernels only (neither operand transposed).
static void use_packed(nbest_gemm_args& g, const void* arena, int64_t off) {
  if (!arena || g.dtype != NBEST_BF16 || g.trans_a || g.trans_b) return;
  g.B_packed = (const char*)arena + off * 2;
  g.b_pack_bn = nbest_pack_bn(g.N);
}
static void use_packed(nbest_gemm_fp8_args& g, const void* arena, int64_t off) {
  if (!arena) return;
  g.B_packed = (const uint8_t*)arena + off;
  g.b_pack_bn = nbest_pack_bn_fp8(g.N, g.K);
}

// The GEMMs of a layer against one of its weight matrices, C[M][N] = epi(A[M][K] . W^T) over all M rows: the forward's four and
// the backward's four dgrads.  GemmPass: what those of one call share; GemmOp: one of them.
struct GemmPass {
  int dtype; int64_t M; nbest_stream_t stream;
  uint64_t seed;                                             // of the dropout (backward: 0, a dgrad drops nothing)
  // nbest_gemm: the weight arena (backward: the dgrad operand), its pre-packed image (NULL: none); b_kn: B is [K][N], not [N][K]
  // (a dgrad on the weights as the forward reads them: no transposed arena)
  Ptrs W; const void* packed; bool b_kn;
  // fp8: nbest_gemm_fp8 instead, on the e4m3 copies of A and of the arena (backward: the transposed copy), with the per-matrix
  // output scales, the delayed amax of the pass's activations (backward: gradients) and the slot blocks this pass records them in
  bool fp8; const void *w8, *w8_packed; const float* inv_scale; const uint32_t* amax_prev; uint32_t* amax_new;
  void* colsum_ws; size_t colsum_ws_bytes; int accumulate;   // DGELU: partial rows of the fused column sums, (+)= into GemmOp::colsum
};
struct GemmOp {   // fields after `bias` (a dgrad: after `epilogue`) are zero unless the call names them
  const void* A; const uint8_t* A8; int a_idx;           // the rows of A; fp8: their e4m3 copy and the index of its amax
  int64_t w_off; int mat;                                // element offset of the matrix in the arenas, index 4 l + {0..3} of its scale
  void* C; int64_t N, K; int epilogue;                   // (C == NULL with C8: every reader takes the e4m3 copy)
  const float* bias;
  const void* R; float drop_p; uint32_t drop_stream;     // BIAS_DROP_RES, RES: the residual rows; the dropout of BIAS_DROP_RES
  void* U; float* colsum;                                // BIAS_GELU (NULL: not kept), DGELU: the GELU' rows; DGELU: column sums of C
  uint8_t* C8; int c_idx;                                // fp8, BIAS_GELU and DGELU: the e4m3 copy of C and the index of its amax
  // a matrix outside the pass's arena (the compact images of pruned heads): read instead of W.W(w_off), with its own packed image or
  // NULL; bf16 / fp32 GEMMs only
  const void* Wm; const void* Wm_packed;
};

static int layer_gemm(const GemmPass& c, const GemmOp& o) {
  if (c.fp8) {
    nbest_gemm_fp8_args g = {};
    g.A = o.A8; g.B = (const uint8_t*)c.w8 + o.w_off; g.C = o.C; g.bias = o.bias; g.R = o.R; g.U = o.U; g.C8 = o.C8;
    g.M = c.M; g.N = o.N; g.K = o.K;
    g.lda = g.ldb = o.K; g.ldc = g.ldr = g.ldu = g.ldc8 = o.N;
    use_packed(g, c.w8_packed, o.w_off);
    g.epilogue = o.epilogue; g.out_scale = 1.f; g.out_scale_dev = c.inv_scale + o.mat;
    g.drop_p = o.drop_p; g.drop_stream = o.drop_stream; g.seed = c.seed;
    g.a_amax = c.amax_prev + o.a_idx;   // the A operand's delayed scale
    if (o.C8) {
      g.c8_amax_prev = c.amax_prev + o.c_idx;
      g.c8_amax_new = c.amax_new ? c.amax_new + (int64_t)o.c_idx * NBEST_AMAX_TENSOR_WORDS : nullptr;
    }
    g.colsum_out = o.colsum; g.colsum_accumulate = c.accumulate; g.ws = c.colsum_ws; g.ws_bytes = c.colsum_ws_bytes;
    return nbest_gemm_fp8(&g, c.stream);
  }
  nbest_gemm_args g = gemm_nt(c.dtype, o.A, o.Wm ? o.Wm : c.W.W(o.w_off), o.C, c.M, o.N, o.K);
  if (c.b_kn) { g.trans_b = 1; g.ldb = o.N; }
  g.epilogue = o.epilogue; g.bias = o.bias;
  if (o.R) { g.R = o.R; g.ldr = o.N; }
  if (o.epilogue == NBEST_EPI_BIAS_DROP_RES) { g.drop_p = o.drop_p; g.drop_stream = o.drop_stream; g.seed = c.seed; }
  if (o.epilogue == NBEST_EPI_BIAS_GELU || o.epilogue == NBEST_EPI_DGELU) { g.U = o.U; g.ldu = o.N; }   // (BIAS_GELU, U == NULL: no GELU' rows)
  if (o.epilogue == NBEST_EPI_DGELU) {
    g.colsum_out = o.colsum; g.colsum_accumulate = g.accumulate = c.accumulate; g.ws = c.colsum_ws; g.ws_bytes = c.colsum_ws_bytes;
  }
  if (o.Wm) use_packed(g, o.Wm_packed, 0);
  else use_packed(g, c.packed, o.w_off);
  return nbest_gemm(&g, c.stream);
}

// ---- one layer's buffers ----------------------------------------------------------------------------------------------------------
// NULL = this pass does not keep that tensor: u (GELU' rows) without a backward, hact (gelu(u) of the dtype) when the fp8 GEMMs
// read h8 instead and no bf16 weight gradient follows, keep (attention-dropout words) without attention dropout, the e4m3 copies
// outside the fp8 forward.
struct LayerBufs {
  void *qkv, *ctx, *r1, *x1, *u, *hact, *r2;
  void* gctx;   // head gates: where the gated context goes and what the attention-output GEMM reads; NULL: ctx is gated in place
  float *lse, *st1, *st2;
  uint32_t* keep;
  uint8_t *x8, *ctx8, *x18, *h8;
};

// X[l] of the activation stash, l >= first_trainable: the input of layer l (l = L: the final hidden state)
static void* stash_x(const ActLayout& a, const Sizes& z, void* act, int l) { return (char*)act + a.X + (size_t)(l - a.K) * z.MH; }

// layer l >= first_trainable: its block of the activation stash (what the forward writes is what the backward reads)
static LayerBufs stashed_layer(const nbest_encoder_desc* d, const ActLayout& a, void* act, int l) {
  char* Lb = (char*)act + a.layer0 + (size_t)(l - a.K) * a.layer_stride;
  LayerBufs b = {};
  b.qkv = Lb + a.o_qkv; b.ctx = Lb + a.o_ctx; b.lse = (float*)(Lb + a.o_lse);
  b.r1 = Lb + a.o_r1; b.st1 = (float*)(Lb + a.o_st1); b.x1 = Lb + a.o_x1;
  b.u = Lb + a.o_u; b.r2 = Lb + a.o_r2; b.st2 = (float*)(Lb + a.o_st2);
  // (bf16 gelu(u) has one reader under the fp8 forward, the bf16 FFN-down weight gradient: not written when the backward runs in fp8)
  b.hact = fp8_backward_active(d) ? nullptr : Lb + a.o_hact;
  if (a.keep_bytes && d->attn_drop > 0.f) b.keep = (uint32_t*)(Lb + a.o_keep);
  if (fp8_forward_active(d)) {
    b.x8 = (uint8_t*)(Lb + a.o_x8); b.ctx8 = (uint8_t*)(Lb + a.o_ctx8);
    b.x18 = (uint8_t*)(Lb + a.o_x18); b.h8 = (uint8_t*)(Lb + a.o_h8);
  }
  if (gate_stashed(d)) b.gctx = (char*)act + a.gctx + (size_t)(l - a.K) * a.gctx_stride;
  return b;
}

// layer l < first_trainable: nothing of it is kept, so it borrows the backward's layer-gradient buffers (see ws_layout).  It keeps
// no GELU' rows (BIAS_GELU without U, as the inference), except in the fp8 epilogue, which writes them; fp8: no bf16 gelu(u) either
static LayerBufs frozen_layer(const nbest_encoder_desc* d, const WsLayout& w, const Sizes& z, void* ws) {
  char* W = (char*)ws;
  const bool f8 = fp8_forward_active(d);
  LayerBufs b = {};
  b.qkv = W + w.dqkv; b.ctx = W + w.dctx; b.lse = (float*)(W + w.fz_lse);
  b.r1 = W + w.dR; b.st1 = (float*)(W + w.fz_st1); b.x1 = W + w.dRd;
  b.r2 = W + w.dB1; b.st2 = (float*)(W + w.fz_st2);
  b.u = f8 ? W + w.fz_u : nullptr; b.hact = f8 ? nullptr : W + w.dBig;
  if (f8) { b.x8 = (uint8_t*)(W + w.f8); b.ctx8 = b.x8 + z.MH8; b.x18 = b.ctx8 + z.MH8; b.h8 = b.x18 + z.MH8; }
  return b;
}

// ---- one layer forward --------------------------------------------------------------------------------------------------------------
// what the layers of one forward / inference call share
struct Fwd {
  const nbest_encoder_desc* d;
  GemmPass g;   // g.fp8: the four GEMMs of a layer on the block-scaled fp8 MFMA, their A operands the e4m3 copies x8 | ctx8 | x18 | h8
  const uint8_t* key_mask;
  bool arec;    // record the activation amax of this pass (fp8, or the calibration pass: fp8 mode without an activation history)
  bool q8;      // fp8 inference (nbest_encoder_infer_fp8): no backward follows, so FFN-up writes the e4m3 copy of gelu(u) and nothing else
  // delayed scale of activation idx = 4 l + {x, ctx, x1, gelu} and the slot block its producer records this pass's amax in (fp8 pass)
  const uint32_t* AP(int idx) const { return g.fp8 ? d->aamax_prev + idx : nullptr; }
  uint32_t* AN(int idx) const { return (g.fp8 && arec) ? d->aamax_new + (int64_t)idx * NBEST_AMAX_TENSOR_WORDS : nullptr; }
  // calibration pass: bf16 GEMMs, the amax of the four GEMM inputs of every layer recorded by a launch of its own
  int calib(const void* t, int64_t n, int idx) const {
    if (!arec || g.fp8) return NBEST_OK;
    return nbest_internal_amax_bf16(t, n, d->aamax_new + (int64_t)idx * NBEST_AMAX_TENSOR_WORDS, (hipStream_t)g.stream);
  }
};

static Fwd make_fwd(const nbest_encoder_desc* d, const void* wts, const float* prm, const Sizes& z, const uint8_t* key_mask,
                    nbest_stream_t stream) {
  const GemmPass g = {d->dtype, z.M, stream, d->seed, Ptrs{(const char*)wts, prm, z.esz}, d->wpk, false, fp8_forward_active(d),
                      d->w8, d->w8p, d->w8_inv_scale, d->aamax_prev, d->aamax_new, nullptr, 0, 0};
  return Fwd{d, g, key_mask, d->w8 && d->aamax_new && d->dtype == NBEST_BF16, false};
}

// Layer l over all M rows: xin -> xout through the buffers `b`.  x8_next: where the last LayerNorm leaves the e4m3 copy of xout for
// the next layer's QKV GEMM (fp8 pass; NULL: no reader).  cls_probs != NULL: also the CLS rows' attention probabilities
// [B][heads][S] fp32, launched right after the QKV projection.  pl != NULL (nbest_encoder_infer_pruned; bf16 / fp32, no cls_probs,
// no head gate): the layer keeps pl->k heads - QKV and attention-out read the compact matrices, qkv is [M][3 64k], ctx [M][64k].
struct PrunedLayer {
  int k;
  const void *wqkv, *wqkv_packed, *wo, *wo_packed;   // Wqkv' [3 64k][H], Wo' [H][64k] and their packed images (NULL: none)
  const float* bqkv;                                 // bqkv' [3 64k]
};
static int layer_forward(const Fwd& c, int l, const void* xin, void* xout, const LayerBufs& b, uint8_t* x8_next, float* cls_probs,
                         const PrunedLayer* pl = nullptr) {
  const nbest_encoder_desc* d = c.d;
  const nbest_layer_offsets& o = d->layers_host[l];
  const Ptrs& P = c.g.W;
  const nbest_stream_t stream = c.g.stream;
  const int64_t M = c.g.M;
  const int H = d->H, F = d->F, dt = d->dtype, t = 4 * l;   // t + {0, 1, 2, 3}: the layer's matrices, and their A operands x, ctx, x1, gelu(u)
  const uint32_t s0 = d->drop_stream_base + 1 + 4 * l;
  const int heads = pl ? pl->k : d->heads, Hk = 64 * heads;   // Hk = H unless the layer is pruned
  // QKV projection: [M,H] x [3H,H]^T + b
  if (c.g.fp8 && l == 0)   // later layers: written by the previous layer's LayerNorm
    RUN(nbest_internal_cast_bf16_to_fp8(xin, b.x8, M * H, c.AP(0), c.AN(0), (hipStream_t)stream));
  GemmOp wqkv = {xin, b.x8, t + 0, o.wqkv, t + 0, b.qkv, 3 * Hk, H, NBEST_EPI_BIAS, pl ? pl->bqkv : P.P(o.bqkv)};
  if (pl) { wqkv.Wm = pl->wqkv; wqkv.Wm_packed = pl->wqkv_packed; }
  RUN(layer_gemm(c.g, wqkv));
  if (cls_probs)   // q = row 0 of each utterance (ldq = S 3H), K | V = the second and third thirds of every row
    RUN(nbest_internal_attention_cls_probs(b.qkv, (int64_t)d->S * H * 3, (const char*)b.qkv + H * P.esz, 3 * H, c.key_mask, cls_probs, d->S,
                                           d->B, d->S, d->heads, 64, dt, stream));
  RUN(c.calib(xin, M * H, t + 0));
  RUN(nbest_internal_attention_fwd8(b.qkv, c.key_mask, b.ctx, b.ctx8, b.lse, d->B, d->S, heads, 64, dt, d->attn_drop, d->seed, s0 + 0,
                                    stream, b.keep, c.AP(t + 1), c.AN(t + 1)));
  RUN(c.calib(b.ctx, M * Hk, t + 1));
  const void* ctx = b.ctx;   // what the attention-output GEMM reads: the context, or its gated copy
  if (d->head_gate && !pl) {   // (pruned: the gate is folded into Wo')
    void* gated = b.gctx ? b.gctx : b.ctx;
    RUN(nbest_head_gate_fwd(b.ctx, H, gated, H, d->head_gate + (int64_t)l * d->heads, M, d->heads, 64, dt, stream));
    ctx = gated;
  }
  // attention output projection + dropout + residual, then LayerNorm
  GemmOp wo = {ctx, b.ctx8, t + 1, o.wo, t + 1, b.r1, H, Hk, NBEST_EPI_BIAS_DROP_RES, P.P(o.bo)};
  wo.R = xin; wo.drop_p = d->hidden_drop; wo.drop_stream = s0 + 1;
  if (pl) { wo.Wm = pl->wo; wo.Wm_packed = pl->wo_packed; }
  RUN(layer_gemm(c.g, wo));
  RUN(nbest_internal_layernorm_fwd8(b.r1, P.P(o.ln1_g), P.P(o.ln1_b), b.x1, b.x18, b.st1, M, H, d->ln_eps, dt, stream, c.AP(t + 2), c.AN(t + 2)));
  RUN(c.calib(b.x1, M * H, t + 2));
  // FFN up + bias + GELU (GELU' of the pre-activation kept for the backward; fp8: also gelu(u) in e4m3, scaled by its own amax)
  // (fp8 inference: NBEST_EPI_BIAS_GELU_Q8, the e4m3 copy alone - no bf16 gelu(u); b.u is NULL there)
  GemmOp w1 = {b.x1, b.x18, t + 2, o.w1, t + 2, c.q8 ? nullptr : b.hact, F, H, c.q8 ? NBEST_EPI_BIAS_GELU_Q8 : NBEST_EPI_BIAS_GELU, P.P(o.b1)};
  w1.U = b.u; w1.C8 = b.h8; w1.c_idx = t + 3;
  RUN(layer_gemm(c.g, w1));
  // FFN down + dropout + residual, then LayerNorm
  GemmOp w2 = {b.hact, b.h8, t + 3, o.w2, t + 3, b.r2, H, F, NBEST_EPI_BIAS_DROP_RES, P.P(o.b2)};
  w2.R = b.x1; w2.drop_p = d->hidden_drop; w2.drop_stream = s0 + 2;
  RUN(layer_gemm(c.g, w2));
  RUN(c.calib(b.hact, M * F, t + 3));
  RUN(nbest_internal_layernorm_fwd8(b.r2, P.P(o.ln2_g), P.P(o.ln2_b), xout, x8_next, b.st2, M, H, d->ln_eps, dt, stream,
                                    x8_next ? c.AP(t + 4) : nullptr, x8_next ? c.AN(t + 4) : nullptr));
  return NBEST_OK;
}

// The top layer with desc.cls_top: the QKV projection over all M rows as layer_forward, everything after it on the B CLS rows (row 0 of
// each utterance).  The compact tensors are the first B rows of the layer's stash regions; rows B .. 2B-1 of r2 are scratch (the GEMM
// outputs ahead of the dropout, then the LayerNorm output on its way to rows b S of xout).  Dropout: the attention kernel hashes
// query 0's counters; the hidden dropout follows the GEMMs (bias-only epilogue) in a small kernel that hashes row b S of the
// full-width tensor (nbest_internal_rows_drop_res) - the GEMM kernels are untouched.  Weights are read unpacked.
static int layer_forward_cls(const Fwd& c, int l, const void* xin, void* xout, const LayerBufs& b) {
  const nbest_encoder_desc* d = c.d;
  const nbest_layer_offsets& o = d->layers_host[l];
  const Ptrs& P = c.g.W;
  const nbest_stream_t stream = c.g.stream;
  hipStream_t st = (hipStream_t)stream;
  const int H = d->H, F = d->F, dt = d->dtype, t = 4 * l;
  const int64_t B = d->B, SH = (int64_t)d->S * H;
  const uint32_t s0 = d->drop_stream_base + 1 + 4 * l;
  const bool hdrop = d->hidden_drop > 0.f;
  void* tmp = (char*)b.r2 + (size_t)B * H * P.esz;
  const GemmOp wqkv = {xin, nullptr, t + 0, o.wqkv, t + 0, b.qkv, 3 * H, H, NBEST_EPI_BIAS, P.P(o.bqkv)};
  RUN(layer_gemm(c.g, wqkv));
  // q = row 0 of each utterance (ldq = S 3H), K | V = the second and third thirds of every row -> ctx [B][H]
  RUN(nbest_attention_cls_fwd_internal(b.qkv, SH * 3, (const char*)b.qkv + H * P.esz, 3 * H, c.key_mask, b.ctx, H, d->B, d->S, d->heads, 64, dt,
                                       stream, d->attn_drop, d->seed, s0 + 0));
  // a GEMM of the B rows + bias, dropout and the residual rows R (row stride ldr) -> out [B][N]
  auto dense_drop_res = [&](const void* A, int64_t w_off, const float* bias, int64_t N, int64_t K, const void* R, int64_t ldr, uint32_t ds,
                            void* out) -> int {
    nbest_gemm_args g = gemm_nt(dt, A, P.W(w_off), hdrop ? tmp : out, B, N, K);
    g.bias = bias;
    if (hdrop) {
      g.epilogue = NBEST_EPI_BIAS;
      RUN(nbest_gemm(&g, stream));
      return nbest_internal_rows_drop_res(tmp, N, R, ldr, out, N, B, (int)N, d->S, dt, d->hidden_drop, d->seed, ds, st);
    }
    g.epilogue = NBEST_EPI_BIAS_DROP_RES; g.R = R; g.ldr = ldr;
    return nbest_gemm(&g, stream);
  };
  const void* ctx = b.ctx;   // head gates (head_gate_stash): the B compact rows gated into gctx (a frozen top layer: in place)
  if (d->head_gate) {
    void* gated = b.gctx ? b.gctx : b.ctx;
    RUN(nbest_head_gate_fwd(b.ctx, H, gated, H, d->head_gate + (int64_t)l * d->heads, B, d->heads, 64, dt, stream));
    ctx = gated;
  }
  RUN(dense_drop_res(ctx, o.wo, P.P(o.bo), H, H, xin, SH, s0 + 1, b.r1));
  RUN(nbest_internal_layernorm_fwd8(b.r1, P.P(o.ln1_g), P.P(o.ln1_b), b.x1, nullptr, b.st1, B, H, d->ln_eps, dt, stream, nullptr, nullptr));
  nbest_gemm_args g = gemm_nt(dt, b.x1, P.W(o.w1), b.hact, B, F, H);
  g.epilogue = NBEST_EPI_BIAS_GELU; g.bias = P.P(o.b1); g.U = b.u; g.ldu = F;
  RUN(nbest_gemm(&g, stream));
  RUN(dense_drop_res(b.hact, o.w2, P.P(o.b2), H, F, b.x1, H, s0 + 2, b.r2));
  RUN(nbest_internal_layernorm_fwd8(b.r2, P.P(o.ln2_g), P.P(o.ln2_b), tmp, nullptr, b.st2, B, H, d->ln_eps, dt, stream, nullptr, nullptr));
  return nbest_internal_rows_drop_res(tmp, H, nullptr, 0, xout, SH, B, H, 1, dt, 0.f, 0, 0, st);   // -> rows b S of the hidden state
}

}  // namespace

extern "C" size_t nbest_encoder_act_bytes(const nbest_encoder_desc* d) { return d ? act_layout(d, sizes(d)).total : 0; }

extern "C" int nbest_encoder_act_view(const nbest_encoder_desc* d, void* act, int layer, void** qkv, float** lse) {
  RUN(check_desc(d));
  RUN(check_cls_top(d));
  NB_CHECK(act && qkv && lse, NBEST_ERR_ARG, "encoder_act_view: null pointer");
  NB_CHECK(0 <= layer && layer < d->L, NBEST_ERR_ARG, "encoder_act_view: layer %d outside [0, L=%d)", layer, d->L);
  const ActLayout a = act_layout(d, sizes(d));
  NB_CHECK(layer >= a.K, NBEST_ERR_ARG, "encoder_act_view: layer %d < first_trainable %d (frozen layers are not stashed)", layer, a.K);
  NB_CHECK(!cls_layer_of(d, layer), NBEST_ERR_ARG, "encoder_act_view: layer %d of a cls_top stash has no lse (its attention ran on the CLS rows only)", layer);
  const LayerBufs b = stashed_layer(d, a, act, layer);
  *qkv = b.qkv; *lse = b.lse;
  return NBEST_OK;
}
extern "C" size_t nbest_encoder_ws_bytes(const nbest_encoder_desc* d) { return d ? ws_layout(d, sizes(d), wgrad_mode(d)).total : 0; }
extern "C" int nbest_encoder_wgrad_launches_per_layer(const nbest_encoder_desc* d) {
  if (!d) return 0;
  return wgrad_launches_per_layer(wgrad_mode(d), wgrad_paired(d, fp8_backward_active(d)));
}

// host only, enqueues nothing: the resolved weight-gradient schedule of a backward call over [layer_begin, layer_end) as int32 words
//   out[0] mode (NBEST_WGRAD_GROUP_NEVER / _ALWAYS / _WINDOW), out[1] dY buffer sets (layers per grouped launch; 0: split-K launches),
//   out[2] the layer whose QKV + attention-out pair is peeled (-1: none), out[3] window launches, then per launch: the layer at whose
//   end it is issued, its tiles, its entries n, and per entry: layer, matrix (0 QKV, 1 attention-out, 2 FFN-up, 3 FFN-down), tile_first,
//   tile_count.  Returns the number of words of the schedule (written only when cap holds them all) or a negative NBEST_ERR_*.
extern "C" int nbest_encoder_wgrad_plan(const nbest_encoder_desc* d, int layer_begin, int layer_end, int32_t* out, int cap) {
  NB_CHECK(d && d->B > 0 && d->S > 0 && d->L > 0 && d->H > 0 && d->F > 0, NBEST_ERR_ARG, "encoder_wgrad_plan: bad descriptor");
  NB_CHECK(first_trainable(d) <= layer_begin && layer_begin <= layer_end && layer_end <= d->L, NBEST_ERR_ARG, "encoder_wgrad_plan: bad layer range");
  NB_CHECK(out || cap <= 0, NBEST_ERR_ARG, "encoder_wgrad_plan: null pointer");
  RUN(check_cls_top(d));
  const WgradMode wm = wgrad_mode(d);
  std::vector<int32_t> v = {wm.mode, wm.gl + wm.sets, -1, 0};
  if (wm.sets > 0) {
    const std::vector<uint8_t> qskip = queue_skip(d, layer_end);
    const WinPlan wp = window_plan(d, layer_begin, layer_end, qskip.data(), d->no_param_grad != 0, true, wm.sets);
    v[2] = wp.peel_layer; v[3] = (int32_t)wp.launches.size();
    for (const WinLaunch& w : wp.launches) {
      v.insert(v.end(), {w.after_layer, w.tiles, w.n});
      for (int i = 0; i < w.n; ++i) v.insert(v.end(), {w.e[i].layer, w.e[i].j, w.e[i].first, w.e[i].count});
    }
  }
  if ((int)v.size() <= cap) std::copy(v.begin(), v.end(), out);
  return (int)v.size();
}

extern "C" int nbest_encoder_forward(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids,
                                     const int64_t* seg, const int64_t* pos, const uint8_t* key_mask, void* act, size_t act_bytes,
                                     void* ws, size_t ws_bytes, void** hidden_out, nbest_stream_t stream) {
  RUN(check_desc(d));
  RUN(check_cls_top(d));
  NB_CHECK(wts && prm && ids && pos && key_mask && act, NBEST_ERR_ARG, "encoder_forward: null pointer");
  const Sizes z = sizes(d);
  const ActLayout a = act_layout(d, z);
  NB_CHECK(act_bytes >= a.total, NBEST_ERR_WORKSPACE, "encoder_forward: activation stash too small (%zu < %zu)", act_bytes, a.total);
  Fwd c = make_fwd(d, wts, prm, z, key_mask, stream);
  const WsLayout wl = ws_layout(d, z, wgrad_mode(d));
  const int FT = a.K;   // layers 0..FT-1 are frozen: run on scratch in ws, nothing of them stashed
  const bool gscratch = d->head_gate && !gate_stashed(d);
  if (c.g.fp8 || FT > 0 || gscratch)
    NB_CHECK(ws && ws_bytes >= wl.total, NBEST_ERR_WORKSPACE, "encoder_forward(%s): workspace too small (%zu < %zu)",
             FT > 0 ? "first_trainable > 0" : gscratch ? "head_gate" : "fp8", ws_bytes, wl.total);
  // head gates: the stash keeps the un-gated context (the backward's operand); the gated copy lives in the backward's dctx buffer,
  // idle during a forward (first_trainable == 0: no frozen layer borrows it).  head_gate_stash: the stashed layers' gctx instead
  // (stashed_layer), a frozen layer in place
  const Ptrs& P = c.g.W;
  char *A = (char*)act, *W = (char*)ws;
  const int H = d->H, dt = d->dtype;
  auto X = [&](int l) { return l >= FT ? stash_x(a, z, act, l) : (void*)(W + ((l & 1) ? wl.fz_x1 : wl.fz_x0)); };
  auto bufs = [&](int l) {
    LayerBufs b = l >= FT ? stashed_layer(d, a, act, l) : frozen_layer(d, wl, z, ws);
    if (gscratch) b.gctx = W + wl.dctx;
    return b;
  };

  float* emb_stats = (float*)(FT > 0 ? W + wl.fz_emb_stats : A + a.emb_stats);
  if (d->base_ids)   // integrated gradients: the word rows at the path points alpha (desc.base_ids / alpha)
    RUN(nbest_embed_ln_fwd_interp(ids, d->base_ids, d->alpha, seg, pos, P.W(d->off_word), P.W(d->off_type), P.W(d->off_pos),
                                  P.P(d->off_emb_ln_g), P.P(d->off_emb_ln_b), X(0), emb_stats, d->B, d->S, H, d->ln_eps, dt,
                                  d->hidden_drop, d->seed, d->drop_stream_base, (hipStream_t)stream));
  else if (d->emb_delta)   // FGM: the word rows moved by desc.emb_delta
    RUN(nbest_embed_ln_fwd_adv(ids, seg, pos, P.W(d->off_word), P.W(d->off_type), P.W(d->off_pos), P.P(d->off_emb_ln_g),
                               P.P(d->off_emb_ln_b), d->emb_delta, X(0), emb_stats, z.M, H, d->ln_eps, dt, d->hidden_drop, d->seed,
                               d->drop_stream_base, (hipStream_t)stream));
  else
    RUN(nbest_embed_ln_fwd(ids, seg, pos, P.W(d->off_word), P.W(d->off_type), P.W(d->off_pos), P.P(d->off_emb_ln_g),
                           P.P(d->off_emb_ln_b), X(0), emb_stats, z.M, H, d->ln_eps, dt, d->hidden_drop, d->seed, d->drop_stream_base,
                           (hipStream_t)stream));
  for (int l = 0; l < d->L; ++l) {
    uint8_t* x8_next = (l + 1 < d->L) ? bufs(l + 1).x8 : nullptr;   // the last LayerNorm's copy has no reader
    if (cls_layer_of(d, l)) RUN(layer_forward_cls(c, l, X(l), X(l + 1), bufs(l)));
    else RUN(layer_forward(c, l, X(l), X(l + 1), bufs(l), x8_next, nullptr));
  }
  if (hidden_out) *hidden_out = X(d->L);
  return NBEST_OK;
}

namespace {
// ---- one layer backward ------------------------------------------------------------------------------------------------------------
// what the layers of one backward call share
struct Bwd {
  const nbest_encoder_desc* d;
  // the dgrad GEMMs: B = the transposed weight arena when there is one (both operands k-contiguous), else the forward's as [K][N];
  // fp8 backward: on the transposed e4m3 weight copy.  Partial rows of the column sums fused into the DGELU one: region 1
  GemmPass dg;
  Ptrs P;
  Sizes z; ActLayout a; WsLayout w;
  char *act, *ws;
  const uint8_t* key_mask;
  float* grad; int accumulate;
  bool npg;     // no_param_grad: dhidden only (attribution) - no weight-gradient GEMM, no bias / LayerNorm-parameter gradient, grad may be NULL
  // fp8 dgrads (descriptor: w8t, gamax_prev / gamax_new, fp8_bwd): the gradient amax of every dgrad operand is recorded in every pass
  // (rec); with a history (f8b) the producers also write e4m3 copies and the four dgrad GEMMs of a layer run in fp8
  bool f8b, rec, hdrop;
  void* red(int i) const { return ws + w.red + (size_t)i * w.red_bytes; }   // region i of the column-reduction partials
  float* G(int64_t off) const { return grad + off; }
  float* GP(int64_t off) const { return npg ? nullptr : grad + off; }   // a bias / LayerNorm-parameter gradient (none: no_param_grad)
  uint32_t* GN(int idx) const { return d->gamax_new + (int64_t)idx * NBEST_AMAX_TENSOR_WORDS; }   // slot block of gradient tensor idx
  Fp8Grad fg(uint8_t* out8, int idx) const {
    if (!rec) return Fp8Grad{nullptr, nullptr, nullptr};
    return Fp8Grad{f8b ? out8 : nullptr, f8b ? d->gamax_prev + idx : nullptr, GN(idx)};
  }
};

static Bwd make_bwd(const nbest_encoder_desc* d, const void* wts, const void* wts_t, const float* prm, float* grad, const uint8_t* key_mask,
                    void* act, void* ws, const Sizes& z, const ActLayout& a, const WsLayout& w, int accumulate, nbest_stream_t stream) {
  const bool wt = (wts_t != nullptr), npg = d->no_param_grad != 0, f8b = fp8_backward_active(d);
  const GemmPass dg = {d->dtype, z.M, stream, 0, Ptrs{(const char*)(wt ? wts_t : wts), prm, z.esz}, wt ? d->wpkt : nullptr, !wt, f8b,
                       d->w8t, d->w8tp, d->w8_inv_scale, d->gamax_prev, d->gamax_new, (char*)ws + w.red + w.red_bytes, w.red_bytes, accumulate};
  return Bwd{d, dg, Ptrs{(const char*)wts, prm, z.esz}, z, a, w, (char*)act, (char*)ws, key_mask, grad, accumulate, npg, f8b,
             !npg && d->gamax_new && d->dtype == NBEST_BF16, d->hidden_drop > 0.f};
}

// The gradient buffers of one layer.  dR2 / dRd2: residual- and dense-branch gradients out of the LN2 backward, dR1 / dRd1: out of the
// LN1 backward (one buffer each without hidden dropout); dRd2, dBig, dRd1 and dqkv are the dY operands of the weight gradients.
struct LayerGrads {
  void *dR2, *dRd2, *dBig, *dB1, *dR1, *dRd1, *dctx, *dqkv;
  uint8_t *dqkv8, *dBig8, *dRd8;   // fp8 backward: the e4m3 copies [M][3H], [M][F], [M][H] the fp8 dgrads and weight gradients read
};
// set < 0: the shared buffers; else those of buffer set `set` (WsLayout::gset), which the layers of the other sets leave alone while
// this layer's weight gradients wait.  cls (desc.cls_top, top layer): everything but dqkv is [B][.], the CLS rows - two compact buffers
// in each of the shared dR, dRd and dB1 regions (S >= 2), one in dctx and dBig.
static LayerGrads layer_grads(const Bwd& c, int set, bool cls) {
  char* W = c.ws;
  const WsLayout& w = c.w;
  const size_t* s = w.gset[set < 0 ? 0 : set];   // (no sets in the workspace: every row names the shared buffers)
  LayerGrads g = {};
  g.dB1 = W + w.dB1; g.dctx = W + w.dctx;
  g.dRd2 = W + s[0]; g.dBig = W + s[1]; g.dRd1 = W + s[2]; g.dqkv = W + s[3];
  g.dR2 = g.dR1 = W + w.dR;
  if (!c.hdrop && set < 0) g.dRd2 = g.dRd1 = g.dR2;
  if (!c.hdrop && set >= 0) { g.dR2 = g.dRd2; g.dR1 = g.dRd1; }
  if (cls) {
    const size_t bh = (size_t)c.d->B * c.d->H * c.z.esz;   // (a multiple of 128 bytes: H % 64 == 0)
    g.dR2 = W + w.dR; g.dR1 = W + w.dB1 + bh; g.dBig = W + w.dBig;
    g.dRd2 = c.hdrop ? (void*)(W + w.dRd) : g.dR2; g.dRd1 = c.hdrop ? (void*)(W + w.dRd + bh) : g.dR1;
  }
  if (c.f8b) { g.dqkv8 = (uint8_t*)W + w.f8; g.dBig8 = g.dqkv8 + 3 * c.z.MH8; g.dRd8 = g.dBig8 + c.z.MF8; }
  return g;
}

// ---- the weight gradients of a backward call: every launch and every event stamp ---------------------------------------------------
// one weight gradient of a layer: dW (fp32, at w_off of `grad`) [rows][cols] (+)= dY^T . X over the token rows
struct WGrad {
  const void *dY, *X;
  const uint8_t *dY8, *X8;   // their e4m3 copies (fp8 backward) ...
  int64_t w_off, rows, cols;
  int g_idx, a_idx;          // ... and the indices of their gradient / activation amax
};

// Every weight-gradient launch and every event stamp (desc.wgrad_events) of one call over the layers [l0, l1), by the resolved mode:
//   NEVER    ready(j), where the layer routine has gradient j's operands complete: its split-K launch between two stamps - the
//            attention-out gradient with QKV's as ONE launch when paired.  A skipped gradient launches nothing (its stamps are still
//            recorded); of a pair with one half skipped the other goes alone.
//   grouped  layer_end: the gradients of a layer wait for the end of its group (their dY tensors in the buffer set of the layer's position,
//            their X tensors in the stash, which the backward only reads) and go out as ONE nbest_wgrad_group launch: per layer QKV,
//            attention-out, FFN-up, FFN-down, the higher layer first.  A layer left without a partner (odd range; the plan's grouping)
//            issues mode NEVER's launches back to back instead.  One event pair per layer (include/nbest_hip.h, wgrad_events).
//   windows  layer_end: the queue of window_plan; a launch goes out at the end of the layer that completes it, the peeled pair and the
//            remainder at the end of the lowest layer.  One event pair per layer of the range: a pair brackets each window launch (the
//            peeled pair launch inside the pair of the window next to it), the pairs left over are recorded back to back at the end.
// desc.cls_top: the top layer's attention-out, FFN-up and FFN-down gradients are plain launches over its K = B token rows in every
// mode (rows), inside the layer's own event pair(s); only its QKV gradient takes part in a group or a window.
struct WgradSched {
  const Bwd& c;
  const WgradMode wm;
  const bool paired;
  const int l0, l1;
  const std::vector<uint8_t> qskip;          // queue_skip: no weight-gradient GEMM for [4 l + {0: QKV, 1: attention-out, 2: FFN-up, 3: FFN-down}]
  int ev_i;                                  // the next event pair
  int l = -1; bool cls = false; WGrad wg[4];   // the current layer (begin)
  nbest_gemm_args pend[8];                   // grouped: the problems of the open group
  int n_pend = 0, cls_pair = 0;              // cls_pair: the group's first layer (desc.cls_top) has recorded its pair already
  WinPlan wp;                                // windows: the plan, its next launch, the problems [4 (l1 - 1 - l) + j], the pairs recorded
  size_t wi = 0; std::vector<nbest_gemm_args> wargs; int pairs_used = 0; bool pair_open = false;

  WgradSched(const Bwd& c_, const WgradMode& wm_, int layer_begin, int layer_end)
      : c(c_), wm(wm_), paired(wgrad_paired(c_.d, c_.f8b)), l0(layer_begin), l1(layer_end), qskip(queue_skip(c_.d, layer_end)),
        ev_i(wgrad_launches_per_layer(wm_, paired) * (c_.d->L - layer_end)) {
    if (wm.sets > 0) {
      wp = window_plan(c.d, l0, l1, qskip.data(), c.npg, true, wm.sets);
      wargs.resize((size_t)4 * (l1 - l0));
    }
  }
  bool deferred() const { return wm.gl > 0 || wm.sets > 0; }
  // the buffer set layer l writes its dY tensors to (-1: the shared buffers): groups are formed from l1 - 1 downwards, gl layers per
  // nbest_wgrad_group launch; the layers of a window schedule rotate over wm.sets sets
  int set_of(int layer) const { return deferred() ? (l1 - 1 - layer) % (wm.gl + wm.sets) : -1; }
  void begin(int layer, const LayerBufs& b, const LayerGrads& g) {
    const nbest_layer_offsets& o = c.d->layers_host[layer];
    const int64_t H = c.d->H, F = c.d->F;
    const int t = 4 * layer;
    l = layer; cls = cls_layer_of(c.d, layer);
    wg[0] = {g.dqkv, stash_x(c.a, c.z, c.act, layer), g.dqkv8, b.x8, o.wqkv, 3 * H, H, t + 3, t + 0};
    wg[1] = {g.dRd1, b.gctx ? b.gctx : b.ctx, g.dRd8, b.ctx8, o.wo, H, H, t + 2, t + 1};   // (head_gate_stash: the gated context)
    wg[2] = {g.dBig, b.x1, g.dBig8, b.x18, o.w1, F, H, t + 1, t + 2};
    wg[3] = {g.dRd2, b.hact, g.dRd8, b.h8, o.w2, H, F, t + 0, t + 3};
  }
  int ready(int j) {
    if (deferred() || (j == 1 && paired)) return NBEST_OK;   // at layer_end / with the QKV gradient
    stamp(0);
    if (cls && j == 0 && paired) RUN(rows(1));
    RUN(cls && j > 0 ? rows(j) : splitk(j, j == 0 && paired ? 1 : -1));
    stamp(1);
    return NBEST_OK;
  }
  int layer_end() { return wm.sets > 0 ? window_layer_end() : wm.gl > 0 ? group_layer_end() : NBEST_OK; }

 private:
  bool skip(int j) const { return c.npg || qskip[4 * l + j]; }
  void stamp(int which) {
    if (c.d->wgrad_events && 2 * ev_i + which < c.d->wgrad_events_n)
      (void)hipEventRecord((hipEvent_t)c.d->wgrad_events[2 * ev_i + which], (hipStream_t)c.dg.stream);
    ev_i += which;
  }
  nbest_gemm_args args_of(const WGrad& x, int64_t tokens) const {
    nbest_gemm_args g = wgrad_args(c.d->dtype, x.rows, x.cols, tokens);
    g.A = x.dY; g.B = x.X; g.C = c.G(x.w_off); g.accumulate = c.accumulate;
    return g;
  }
  // gradient j of the current layer as its split-K launch, or gradients j and j2 as one paired launch
  int splitk(int j, int j2 = -1) {
    const nbest_stream_t stream = c.dg.stream;
    const int64_t M = c.z.M;
    void* slab = c.ws + c.w.slab;
    const WGrad* p = skip(j) ? nullptr : wg + j;
    const WGrad* q = (j2 >= 0 && !skip(j2)) ? wg + j2 : nullptr;
    if (!p) { p = q; q = nullptr; }
    if (p && c.f8b) {
      const uint32_t *gp = c.d->gamax_prev, *ap = c.d->aamax_prev;
      if (q)
        RUN(nbest_wgrad_fp8_pair(p->dY8, p->X8, c.G(p->w_off), p->rows, p->rows, p->cols, p->cols, gp + p->g_idx, ap + p->a_idx, q->dY8, q->X8,
                                 c.G(q->w_off), q->rows, q->rows, q->cols, q->cols, gp + q->g_idx, ap + q->a_idx, p->cols, M, c.accumulate, slab,
                                 c.w.slab_bytes, stream));
      else
        RUN(nbest_wgrad_fp8(p->dY8, p->X8, c.G(p->w_off), p->rows, p->cols, M, p->rows, p->cols, p->cols, gp + p->g_idx, ap + p->a_idx,
                            c.accumulate, slab, c.w.slab_bytes, stream));
    } else if (p) {
      nbest_gemm_args g1 = args_of(*p, M), g2 = args_of(q ? *q : *p, M);
      g1.ws = slab; g1.ws_bytes = c.w.slab_bytes;   // (a pair: the slabs of both)
      RUN(q ? nbest_wgrad_pair(&g1, &g2, stream) : nbest_gemm(&g1, stream));
    }
    return NBEST_OK;
  }
  // the attention-out and QKV gradients at the end of a layer, as mode NEVER launches them: one launch where the pair fits it
  int low_pair() { if (!paired) RUN(splitk(1)); return splitk(0, paired ? 1 : -1); }
  // cls_top layer: gradient j (1: attention-out, 2: FFN-up, 3: FFN-down) over its K = B token rows, one plain launch (the caller's
  // flags alone decide: the queue's flags name these three as skipped)
  int rows(int j) {
    if (c.npg || (c.d->wgrad_skip_host && c.d->wgrad_skip_host[4 * l + j])) return NBEST_OK;
    nbest_gemm_args g = args_of(wg[j], c.d->B);
    g.ws = c.ws + c.w.slab; g.ws_bytes = c.w.slab_bytes;
    return nbest_gemm(&g, c.dg.stream);
  }
  int rows_all() { RUN(rows(3)); RUN(rows(2)); return rows(1); }
  int group_layer_end() {
    const int gpos = set_of(l);
    const bool group_ends = gpos == wm.gl - 1 || l == l0;
    if (group_ends && gpos + 1 < wm.gl && c.d->wgrad_group != NBEST_WGRAD_GROUP_ALWAYS) {   // no partner: mode NEVER's launches, one event pair
      stamp(0);
      if (cls) RUN(rows_all());
      RUN(splitk(3)); RUN(splitk(2)); RUN(low_pair());
      stamp(1);
      return NBEST_OK;
    }
    for (int j = 0; j < 4; ++j)
      if (!skip(j)) pend[n_pend++] = args_of(wg[j], c.z.M);
    if (cls && !group_ends) {   // the top layer's own pair brackets its small launches; its QKV gradient waits for the group
      stamp(0);
      RUN(rows_all());
      stamp(1);
      cls_pair = 1;
    }
    if (group_ends) {
      stamp(0);
      if (cls) RUN(rows_all());
      if (n_pend) RUN(nbest_wgrad_group(pend, n_pend, c.dg.stream));
      stamp(1);
      for (int i = 0; i < gpos - cls_pair; ++i) { stamp(0); stamp(1); }
      n_pend = 0; cls_pair = 0;
    }
    return NBEST_OK;
  }
  void pair_begin() { if (!pair_open && pairs_used < l1 - l0) { stamp(0); pair_open = true; } }
  void pair_end() { if (pair_open) { stamp(1); ++pairs_used; pair_open = false; } }
  int window_layer_end() {
    for (int j = 0; j < 4; ++j)
      if (!skip(j)) wargs[(size_t)4 * (l1 - 1 - l) + j] = args_of(wg[j], c.z.M);
    if (cls) {   // the top layer's small launches open its pair
      pair_begin();
      RUN(rows_all());
    }
    if (l == wp.peel_layer) {
      pair_begin();
      RUN(low_pair());
    }
    for (; wi < wp.launches.size() && wp.launches[wi].after_layer == l; ++wi) {
      const WinLaunch& wl = wp.launches[wi];
      nbest_gemm_args tab[kWinEntries];
      int32_t first[kWinEntries], count[kWinEntries];
      for (int i = 0; i < wl.n; ++i) {
        tab[i] = wargs[(size_t)4 * (l1 - 1 - wl.e[i].layer) + wl.e[i].j];
        first[i] = wl.e[i].first; count[i] = wl.e[i].count;
      }
      pair_begin();
      RUN(nbest_wgrad_window(tab, first, count, wl.n, c.dg.stream));
      pair_end();
    }
    pair_end();   // (a peeled pair with no window after it)
    if (l == l0)
      for (; pairs_used < l1 - l0; ++pairs_used) { stamp(0); stamp(1); }
    return NBEST_OK;
  }
};

// Layer l over all M rows: dA, the gradient w.r.t. its output, becomes the gradient w.r.t. its input (not formed for layer
// first_trainable under desc.no_input_grad: it has no reader).  LN2 bwd -> FFN-down dgrad -> FFN-up dgrad -> LN1 bwd -> attention-out
// dgrad -> head gates -> attention bwd -> QKV dgrad; sched.ready(j) where the operands of weight gradient j are complete - without
// deferral dRd2 and dRd1 are one buffer, so FFN-down's must be issued before the LN1 backward overwrites it.
static int layer_backward(const Bwd& c, int l, const LayerBufs& b, const LayerGrads& g, void* dA, WgradSched& sched) {
  const nbest_encoder_desc* d = c.d;
  const nbest_layer_offsets& o = d->layers_host[l];
  const Ptrs& P = c.P;
  const nbest_stream_t stream = c.dg.stream;
  const int64_t M = c.z.M;
  const int H = d->H, F = d->F, dt = d->dtype, t = 4 * l, accumulate = c.accumulate;
  const uint32_t s0 = d->drop_stream_base + 1 + 4 * l;
  const bool f8b = c.f8b, hdrop = c.hdrop;
  // LN2 backward: dR (residual branch), dRd (dense branch, under the dropout mask), db2
  // (with fp8 dgrads / wgrads the bf16 forms of dRd, dBig and dqkv have no reader: only their e4m3 copies are written)
  RUN(nbest_internal_layernorm_bwd8(dA, b.r2, b.st2, P.P(o.ln2_g), g.dR2, (hdrop && !f8b) ? g.dRd2 : nullptr, c.GP(o.ln2_g), c.GP(o.ln2_b),
                                    c.GP(o.b2), M, H, dt, accumulate, d->hidden_drop, d->seed, s0 + 2, c.red(0), c.w.red_bytes, stream,
                                    c.fg(g.dRd8, t + 0)));
  // FFN-down: dgrad fused with GELU' -> dU (the FFN-up bias gradient = column sums of dU is fused into this epilogue)
  GemmOp dw2 = {g.dRd2, g.dRd8, t + 0, o.w2, t + 3, f8b ? nullptr : g.dBig, F, H, NBEST_EPI_DGELU};
  dw2.U = b.u; dw2.colsum = c.GP(o.b1); dw2.C8 = g.dBig8; dw2.c_idx = t + 1;
  RUN(layer_gemm(c.dg, dw2));
  if (c.rec && !f8b) RUN(nbest_internal_amax_bf16(g.dBig, M * F, c.GN(t + 1), (hipStream_t)stream));   // calibration pass: this producer is a bf16 kernel
  RUN(sched.ready(3));
  // FFN-up: dgrad + residual gradient
  GemmOp dw1 = {g.dBig, g.dBig8, t + 1, o.w1, t + 2, g.dB1, H, F, NBEST_EPI_RES};
  dw1.R = g.dR2;
  RUN(layer_gemm(c.dg, dw1));
  RUN(sched.ready(2));
  // LN1 backward
  RUN(nbest_internal_layernorm_bwd8(g.dB1, b.r1, b.st1, P.P(o.ln1_g), g.dR1, (hdrop && !f8b) ? g.dRd1 : nullptr, c.GP(o.ln1_g), c.GP(o.ln1_b),
                                    c.GP(o.bo), M, H, dt, accumulate, d->hidden_drop, d->seed, s0 + 1, c.red(2), c.w.red_bytes, stream,
                                    c.fg(g.dRd8, t + 2)));
  // attention output projection: dgrad
  const GemmOp dwo = {g.dRd1, g.dRd8, t + 2, o.wo, t + 1, g.dctx, H, H, NBEST_EPI_NONE};
  RUN(layer_gemm(c.dg, dwo));
  RUN(sched.ready(1));   // (paired: dRd1 and ctx stay untouched until the next layer's LayerNorm backward - issued with QKV's)
  // head gates: dctx is the gradient w.r.t. the gated context - its product with the stashed un-gated one is the gate's gradient
  // (per utterance), and scaled by the gate it is the gradient the attention backward takes
  if (d->head_gate)
    RUN(nbest_head_gate_bwd(b.ctx, g.dctx, d->head_gate + (int64_t)l * d->heads,
                            d->head_gate_grad ? d->head_gate_grad + (int64_t)l * d->B * d->heads : nullptr, d->B, d->S, d->heads, 64, dt, stream));
  // attention backward -> dqkv ; QKV bias gradient
  RUN(nbest_internal_attention_bwd8(b.qkv, c.key_mask, b.ctx, g.dctx, b.lse, f8b ? nullptr : g.dqkv, c.GP(o.bqkv), accumulate, c.red(3),
                                    c.w.red_bytes, d->B, d->S, d->heads, 64, dt, d->attn_drop, d->seed, s0 + 0, stream, c.fg(g.dqkv8, t + 3),
                                    b.keep));
  // QKV projection: dgrad + residual gradient -> gradient wrt the layer input
  if (!(d->no_input_grad && l == c.a.K)) {
    GemmOp dwqkv = {g.dqkv, g.dqkv8, t + 3, o.wqkv, t + 0, dA, H, 3 * H, NBEST_EPI_RES};
    dwqkv.R = g.dR1;
    RUN(layer_gemm(c.dg, dwqkv));
  }
  return sched.ready(0);
}

// The top layer with desc.cls_top (layer_forward_cls): dA is read at the CLS rows only; the LayerNorm backwards, the FFN and
// attention-out dgrads run on B rows (weights read unpacked), a one-query attention backward writes the layer's dQ|dK|dV in full and the
// QKV dgrad runs as ever.  The weight gradients read the compact buffers and the first B rows of the stash regions: all four at the end.
static int layer_backward_cls(const Bwd& c, int l, const LayerBufs& b, const LayerGrads& g, void* dA, WgradSched& sched) {
  const nbest_encoder_desc* d = c.d;
  const nbest_layer_offsets& o = d->layers_host[l];
  const Ptrs& P = c.P;
  const nbest_stream_t stream = c.dg.stream;
  hipStream_t st = (hipStream_t)stream;
  const int H = d->H, F = d->F, dt = d->dtype, t = 4 * l, accumulate = c.accumulate;
  const uint32_t s0 = d->drop_stream_base + 1 + 4 * l;
  const bool hdrop = c.hdrop;
  const int64_t Bn = d->B, SH = (int64_t)d->S * H;
  const size_t bh = (size_t)Bn * H * c.z.esz, half = c.w.red_bytes / 2;
  void* dAc = c.ws + c.w.dR + bh;   // the CLS rows of dhidden
  GemmPass dgc = c.dg;              // the dgrads of the B rows: weights read unpacked
  dgc.M = Bn; dgc.packed = nullptr;
  RUN(nbest_internal_rows_drop_res(dA, SH, nullptr, 0, dAc, H, Bn, H, 1, dt, 0.f, 0, 0, st));
  // a LayerNorm backward of the B rows (parameters at ln_g, ln_b) without dropout: dR; the dense branch's mask (the decisions of rows b S,
  // stream ds) -> dRd and the bias gradient under it follow in a small kernel and a fixed-order column sum (partial rows: the upper half
  // of the LayerNorm's region `red`)
  auto ln_bwd = [&](const void* dy, const void* x, const float* stats, int64_t ln_g, int64_t ln_b, int64_t bias, void* dR, void* dRd, void* red,
                    uint32_t ds) -> int {
    RUN(nbest_internal_layernorm_bwd8(dy, x, stats, P.P(ln_g), dR, nullptr, c.G(ln_g), c.G(ln_b), hdrop ? nullptr : c.G(bias), Bn, H, dt,
                                      accumulate, 0.f, 0, 0, red, half, stream, Fp8Grad{nullptr, nullptr, nullptr}));
    if (!hdrop) return NBEST_OK;
    RUN(nbest_internal_rows_drop_res(dR, H, nullptr, 0, dRd, H, Bn, H, d->S, dt, d->hidden_drop, d->seed, ds, st));
    return nbest_colsum(dRd, c.G(bias), Bn, H, H, dt, accumulate, (char*)red + half, half, stream);
  };
  RUN(ln_bwd(dAc, b.r2, b.st2, o.ln2_g, o.ln2_b, o.b2, g.dR2, g.dRd2, c.red(0), s0 + 2));
  GemmOp dw2 = {g.dRd2, nullptr, t + 0, o.w2, t + 3, g.dBig, F, H, NBEST_EPI_DGELU};
  dw2.U = b.u; dw2.colsum = c.G(o.b1);
  RUN(layer_gemm(dgc, dw2));
  GemmOp dw1 = {g.dBig, nullptr, t + 1, o.w1, t + 2, g.dB1, H, F, NBEST_EPI_RES};
  dw1.R = g.dR2;
  RUN(layer_gemm(dgc, dw1));
  RUN(ln_bwd(g.dB1, b.r1, b.st1, o.ln1_g, o.ln1_b, o.bo, g.dR1, g.dRd1, c.red(2), s0 + 1));
  const GemmOp dwo = {g.dRd1, nullptr, t + 2, o.wo, t + 1, g.dctx, H, H, NBEST_EPI_NONE};
  RUN(layer_gemm(dgc, dwo));
  if (d->head_gate)   // (head_gate_stash) the B compact rows: dctx scaled by the gate, the attention backward takes the un-gated ctx
    RUN(nbest_head_gate_bwd(b.ctx, g.dctx, d->head_gate + (int64_t)l * d->heads, nullptr, d->B, 1, d->heads, 64, dt, stream));
  // one-query attention backward: the layer's dQ|dK|dV in full (dQ zero outside the CLS rows) ; QKV bias gradient
  RUN(nbest_internal_attention_cls_bwd(b.qkv, c.key_mask, b.ctx, g.dctx, g.dqkv, c.G(o.bqkv), accumulate, c.red(3), c.w.red_bytes, d->B, d->S,
                                       d->heads, 64, dt, d->attn_drop, d->seed, s0 + 0, stream));
  // QKV dgrad as ever, its residual gradient zero outside the CLS rows (dctx [M][H] is free again)
  if (!(d->no_input_grad && l == c.a.K)) {
    NB_CHECK(hipMemsetAsync(g.dctx, 0, (size_t)c.z.M * H * c.z.esz, st) == hipSuccess, NBEST_ERR_LAUNCH, "encoder_backward: memset failed");
    RUN(nbest_internal_rows_drop_res(g.dR1, H, nullptr, 0, g.dctx, SH, Bn, H, 1, dt, 0.f, 0, 0, st));
    GemmOp dwqkv = {g.dqkv, nullptr, t + 3, o.wqkv, t + 0, dA, H, 3 * H, NBEST_EPI_RES};
    dwqkv.R = g.dctx;
    RUN(layer_gemm(c.dg, dwqkv));
  }
  for (int j = 3; j >= 0; --j) RUN(sched.ready(j));
  return NBEST_OK;
}
}  // namespace

extern "C" int nbest_encoder_backward(const nbest_encoder_desc* d, const void* wts, const void* wts_t, const float* prm, float* grad,
                                      const int64_t* ids, const int64_t* seg, const int64_t* pos, const uint8_t* key_mask,
                                      void* act, size_t act_bytes, void* dhidden, void* ws, size_t ws_bytes, int accumulate,
                                      int layer_begin, int layer_end, int with_embeddings, nbest_stream_t stream) {
  RUN(check_desc(d));
  RUN(check_cls_top(d));
  NB_CHECK(0 <= layer_begin && layer_begin <= layer_end && layer_end <= d->L, NBEST_ERR_ARG, "encoder_backward: bad layer range");
  const bool npg = d->no_param_grad != 0;
  NB_CHECK(!npg || (!with_embeddings && d->first_trainable == 0 && !d->no_input_grad && !d->w8), NBEST_ERR_ARG,
           "encoder_backward: no_param_grad refuses with_embeddings (%d), first_trainable > 0 (%d), no_input_grad (%d) and the fp8 "
           "forward (w8): it forms the input gradient only, of a full stash", with_embeddings, d->first_trainable, d->no_input_grad);
  NB_CHECK(!d->head_gate || npg || d->head_gate_stash, NBEST_ERR_ARG, "encoder_backward: head_gate needs no_param_grad (the attention-output weight gradient would "
           "need the gated context, which the forward keeps only with head_gate_stash)");
  NB_CHECK(wts && prm && (grad || npg) && ids && pos && key_mask && act && dhidden && ws, NBEST_ERR_ARG, "encoder_backward: null pointer");
  NB_CHECK(!with_embeddings || d->word_perm, NBEST_ERR_ARG, "encoder_backward: desc.word_perm (stable argsort of this pass's ids) is required");
  NB_CHECK(layer_begin >= d->first_trainable, NBEST_ERR_ARG, "encoder_backward: layer_begin %d < first_trainable %d (those layers are not stashed)",
           layer_begin, d->first_trainable);
  NB_CHECK(!with_embeddings || (d->first_trainable == 0 && !d->no_input_grad), NBEST_ERR_ARG,
           "encoder_backward: with_embeddings needs first_trainable == 0 and no_input_grad == 0");
  const Sizes z = sizes(d);
  const ActLayout a = act_layout(d, z);
  const WgradMode wm = wgrad_mode(d);   // once per call: the workspace layout and the weight-gradient schedule follow it
  const WsLayout w = ws_layout(d, z, wm);
  NB_CHECK(act_bytes >= a.total, NBEST_ERR_WORKSPACE, "encoder_backward: activation stash too small");
  NB_CHECK(ws_bytes >= w.total, NBEST_ERR_WORKSPACE, "encoder_backward: workspace too small (%zu < %zu)", ws_bytes, w.total);
  const Bwd c = make_bwd(d, wts, wts_t, prm, grad, key_mask, act, ws, z, a, w, accumulate, stream);
  WgradSched sched(c, wm, layer_begin, layer_end);
  void* dA = dhidden;   // the running gradient w.r.t. the input of the lowest layer processed so far

  struct BatchGuard { ~BatchGuard() { nbest_internal_rowred_batch_abort(); } } batch_guard;   // an error return mid-layer must not leave it open
  for (int l = layer_end - 1; l >= layer_begin; --l) {
    const LayerBufs b = stashed_layer(d, a, act, l);
    const bool cls = cls_layer_of(d, l);
    const LayerGrads g = layer_grads(c, sched.set_of(l), cls);
    sched.begin(l, b, g);
    if (!npg) nbest_internal_rowred_batch_begin();    // the layer's four bias / LayerNorm-parameter reductions: one finalize launch at its end
    RUN(cls ? layer_backward_cls(c, l, b, g, dA, sched) : layer_backward(c, l, b, g, dA, sched));
    RUN(sched.layer_end());
    if (!npg) RUN(nbest_internal_rowred_batch_flush((hipStream_t)stream));
  }
  if (!with_embeddings) return NBEST_OK;
  hipStream_t st = (hipStream_t)stream;
  const Ptrs& P = c.P;
  const int H = d->H;
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(c.G(d->off_word), 0, (size_t)d->vocab * H * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(c.G(d->off_pos), 0, (size_t)d->max_pos * H * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(c.G(d->off_type), 0, (size_t)d->n_types * H * sizeof(float), st);
    NB_CHECK(e == hipSuccess, NBEST_ERR_LAUNCH, "encoder_backward: memset failed: %s", hipGetErrorString(e));
  }
  const float* emb_stats = (const float*)(c.act + a.emb_stats);
  if (d->emb_delta)   // the stash's forward ran on the perturbed word rows: x_hat is recomputed from them (delta gets no gradient)
    RUN(nbest_embed_ln_bwd_adv(ids, seg, pos, d->word_perm, P.W(d->off_word), P.W(d->off_type), P.W(d->off_pos), P.P(d->off_emb_ln_g),
                               emb_stats, d->emb_delta, dA, c.G(d->off_word), c.G(d->off_type), c.G(d->off_pos),
                               c.G(d->off_emb_ln_g), c.G(d->off_emb_ln_b), d->B, d->S, H, d->n_types, d->dtype, d->word_pad_id, d->pos_pad_id,
                               accumulate, accumulate, d->hidden_drop, d->seed, d->drop_stream_base, c.ws + w.emb, w.emb_bytes, stream));
  else
    RUN(nbest_embed_ln_bwd(ids, seg, pos, d->word_perm, P.W(d->off_word), P.W(d->off_type), P.W(d->off_pos), P.P(d->off_emb_ln_g),
                           emb_stats, dA, c.G(d->off_word), c.G(d->off_type), c.G(d->off_pos), c.G(d->off_emb_ln_g),
                           c.G(d->off_emb_ln_b), d->B, d->S, H, d->n_types, d->dtype, d->word_pad_id, d->pos_pad_id, accumulate, accumulate,
                           d->hidden_drop, d->seed, d->drop_stream_base, c.ws + w.emb, w.emb_bytes, stream));
  return NBEST_OK;
}

// ---- inference: forward only, final hidden state of the B CLS rows ---------------------------------------------------------------
// Layers 0 .. L-2 are layer_forward (dropout 0) on buffers reused from layer to layer; FFN-up leaves out the GELU' rows (BIAS_GELU
// with U == NULL).  Layer L-1: K|V over all M rows, then Q, attention, attention-out, LayerNorm, FFN and LayerNorm on the B CLS
// rows only (row 0 of each utterance: the one row the STC heads read).
//   X[2] [M][H] T (ping-pong) | emb_stats [M][2] f32 | qkv [M][3H] T (last layer: K|V [M][2H]) | ctx | r1 | x1 | r2 [M][H] T |
//   hact [M][F] T | lse [B heads S] f32 | st1 | st2 [M][2] f32.   Last layer: Q -> ctx, context -> r1, x1 -> x1, gelu -> hact,
//   attention-out and FFN-down sums -> r2.  Independent of L.  Head gates (desc.head_gate) are applied in place, on ctx [M][H] of
//   layers 0 .. L-2 and on the [B][H] CLS context of the last layer.
//   Compact pruned heads (nbest_encoder_infer_pruned): layer l keeps k heads - qkv [M][3 64k], ctx [M][64k] (last layer: K|V [M][2 64k],
//   Q and context [B][64k]) in the same buffers; no gate launch, the gate is in the compact attention-output matrix.
//   fp8 (nbest_encoder_infer_fp8): four regions more, at the end - x8 | ctx8 | x18 [M][H] e4m3, h8 [M][F] e4m3, the copies of a layer's
//   four GEMM inputs.  The fp8 pass uses [B][F] of hact only (the full-width FFN-up writes h8), the calibration pass none of the four
//   regions: one size for both.  Last layer: K|V is an fp8 GEMM on x8; the B CLS rows are bf16 as above.
namespace {
struct InferLayout {
  size_t X0, X1, emb_stats, qkv, ctx, r1, x1, r2, hact, lse, st1, st2;
  size_t x8, ctx8, x18, h8;   // fp8 only (else 0 bytes)
  size_t total;
};
static InferLayout infer_layout(const Sizes& z, bool fp8 = false) {
  InferLayout w;
  size_t o = 0;
  w.X0 = take(o, z.MH); w.X1 = take(o, z.MH); w.emb_stats = take(o, z.st);
  w.qkv = take(o, z.M3H); w.ctx = take(o, z.MH); w.r1 = take(o, z.MH); w.x1 = take(o, z.MH); w.r2 = take(o, z.MH);
  w.hact = take(o, z.MF); w.lse = take(o, z.lse); w.st1 = take(o, z.st); w.st2 = take(o, z.st);
  w.x8 = take(o, fp8 ? z.MH8 : 0); w.ctx8 = take(o, fp8 ? z.MH8 : 0); w.x18 = take(o, fp8 ? z.MH8 : 0); w.h8 = take(o, fp8 ? z.MF8 : 0);
  w.total = o;
  return w;
}
// every layer runs on the same buffers; nothing is kept for a backward (no GELU' rows, no keep words).  fp8_pass: the GEMMs read the
// e4m3 copies, and gelu(u) of the full-width layers exists in e4m3 only (hact serves the last layer's B CLS rows)
static LayerBufs infer_layer(const InferLayout& w, void* ws, bool fp8_pass) {
  char* W = (char*)ws;
  LayerBufs b = {};
  b.qkv = W + w.qkv; b.ctx = W + w.ctx; b.lse = (float*)(W + w.lse);
  b.r1 = W + w.r1; b.st1 = (float*)(W + w.st1); b.x1 = W + w.x1;
  b.hact = W + w.hact; b.r2 = W + w.r2; b.st2 = (float*)(W + w.st2);
  if (fp8_pass) { b.x8 = (uint8_t*)(W + w.x8); b.ctx8 = (uint8_t*)(W + w.ctx8); b.x18 = (uint8_t*)(W + w.x18); b.h8 = (uint8_t*)(W + w.h8); }
  return b;
}

// token elimination (nbest_encoder_infer_tokens): after infer_layout, the rows the selection works on - the score and the current mask
// as floats [B][S] f32, the kept indices [B][S] i32, two origin rows [B][S] i32 and two masks [B][S] u8 (each pair: read one, write
// the other; the first mask read is the caller's).  Every shrunken row fits its full-width region.
struct TokenLayout {
  size_t score, maskf, idx, org[2], mask[2], total;
};
static TokenLayout token_layout(const nbest_encoder_desc* d, size_t base) {
  TokenLayout t;
  const size_t n = (size_t)d->B * d->S;
  size_t o = base;
  t.score = take(o, al(4 * n)); t.maskf = take(o, al(4 * n)); t.idx = take(o, al(4 * n));
  t.org[0] = take(o, al(4 * n)); t.org[1] = take(o, al(4 * n)); t.mask[0] = take(o, al(n)); t.mask[1] = take(o, al(n));
  t.total = o;
  return t;
}
// the schedule of nbest_encoder_infer_tokens and where the kept positions go (NULL: nowhere)
struct TokenPrune {
  const int32_t* keep;
  int32_t* token_kept;
};
}  // namespace

extern "C" size_t nbest_encoder_infer_ws_bytes(const nbest_encoder_desc* d) { return d ? infer_layout(sizes(d)).total : 0; }
extern "C" size_t nbest_encoder_infer_tokens_ws_bytes(const nbest_encoder_desc* d) {
  return d ? token_layout(d, infer_layout(sizes(d)).total).total : 0;
}
extern "C" size_t nbest_encoder_infer_fp8_ws_bytes(const nbest_encoder_desc* d) { return d ? infer_layout(sizes(d), true).total : 0; }

// cls_attn != NULL: also the CLS row's attention probabilities of every layer, [L][B][heads][S] fp32, each launched right after the
// layer's QKV projection (last layer: after the CLS-row Q).
// pr != NULL (nbest_encoder_infer_pruned): layer l keeps k = pr->layers_host[l].k heads and reads Wqkv', bqkv' and Wo' out of the compact
// images (head_prune.hip) - every compact tensor fits the buffer of its full-width counterpart, so the workspace is the same.
// f8 (nbest_encoder_infer_fp8 only; no cls_attn, no pr): the descriptor carries the fp8 forward.  Without an activation history
// (fp8_act == 0) the pass is the bf16 one plus the amax records of the GEMM inputs (Fwd::calib); with one, the full-width GEMMs run in
// fp8 on static scales: nothing is recorded.
// tp != NULL (nbest_encoder_infer_tokens only; no cls_attn, no pr, no f8, no head gate): tokens are dropped between the layers by the
// schedule tp->keep (token_prune.hip), and every layer runs on the rows that are left; the workspace grows by token_layout.
static int infer_impl(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                      const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out, float* cls_attn,
                      const nbest_head_prune_images* pr, nbest_stream_t stream, bool f8 = false, const TokenPrune* tp = nullptr) {
  if (f8) {
    NB_CHECK(d, NBEST_ERR_ARG, "encoder_infer_fp8: null descriptor");
    NB_CHECK(d->dtype == NBEST_BF16, NBEST_ERR_DTYPE, "encoder_infer_fp8: needs the bf16 path (dtype %d)", d->dtype);
    NB_CHECK(d->w8 && d->w8_inv_scale, NBEST_ERR_ARG, "encoder_infer_fp8: needs the e4m3 weights and their inverse scales (desc.w8, w8_inv_scale)");
    NB_CHECK(!d->head_gate, NBEST_ERR_ARG, "encoder_infer_fp8: head gates (desc.head_gate) are not supported");
    if (d->fp8_act) NB_CHECK(d->aamax_prev, NBEST_ERR_ARG, "encoder_infer_fp8: fp8_act without an activation history (desc.aamax_prev); calibrate first");
    else NB_CHECK(d->aamax_new, NBEST_ERR_ARG, "encoder_infer_fp8: the calibration pass (fp8_act == 0) needs the slot blocks it records in (desc.aamax_new)");
  }
  RUN(check_desc(d, false));
  NB_CHECK(d->hidden_drop == 0.f && d->attn_drop == 0.f, NBEST_ERR_ARG,
           "encoder_infer: dropout must be 0 (hidden_drop=%g, attn_drop=%g): inference has no dropout", d->hidden_drop, d->attn_drop);
  NB_CHECK(f8 || !d->w8, NBEST_ERR_ARG, "encoder_infer: the fp8 forward (desc.w8) is not supported; pass the bf16 weights without w8");
  NB_CHECK(!d->base_ids && !d->alpha, NBEST_ERR_ARG, "encoder_infer: interpolated embeddings (desc.base_ids / alpha) are not supported; "
                                                     "run nbest_encoder_forward");
  NB_CHECK(!d->emb_delta, NBEST_ERR_ARG, "encoder_infer: perturbed embeddings (desc.emb_delta) are not supported; run nbest_encoder_forward");
  NB_CHECK(wts && prm && ids && pos && key_mask && ws && cls_out, NBEST_ERR_ARG, "encoder_infer: null pointer");
  const Sizes z = sizes(d);
  const InferLayout w = infer_layout(z, f8);
  const TokenLayout tw = token_layout(d, w.total);
  NB_CHECK(ws_bytes >= (tp ? tw.total : w.total), NBEST_ERR_WORKSPACE, "encoder_infer: workspace too small (%zu < %zu)", ws_bytes,
           tp ? tw.total : w.total);
  if (tp) {
    NB_CHECK(!d->head_gate, NBEST_ERR_ARG, "encoder_infer_tokens: head gates (desc.head_gate) are not supported (a head mean under a gate is not defined)");
    for (int l = 0; l + 1 < d->L; ++l) {
      NB_CHECK(tp->keep[l] >= 1, NBEST_ERR_ARG, "encoder_infer_tokens: keep[%d] = %d < 1", l, tp->keep[l]);
      NB_CHECK(l == 0 || tp->keep[l] <= tp->keep[l - 1], NBEST_ERR_ARG, "encoder_infer_tokens: the schedule increases at layer %d (%d after %d)",
               l, tp->keep[l], tp->keep[l - 1]);
    }
  }
  if (pr) {
    NB_CHECK(pr->w && pr->bqkv && pr->layers_host, NBEST_ERR_ARG, "encoder_infer_pruned: null image pointer");
    NB_CHECK(!d->head_gate, NBEST_ERR_ARG, "encoder_infer_pruned: desc.head_gate must be NULL (the gate is folded into the compact Wo')");
    NB_CHECK(((uintptr_t)pr->w & 15) == 0 && ((uintptr_t)pr->w_packed & 15) == 0 && ((uintptr_t)pr->bqkv & 15) == 0, NBEST_ERR_ALIGN,
             "encoder_infer_pruned: the images must be 16-byte aligned");
    for (int l = 0; l < d->L; ++l) {
      const nbest_head_prune_layer& t = pr->layers_host[l];
      NB_CHECK(t.k >= 1 && t.k <= d->heads, NBEST_ERR_ARG, "encoder_infer_pruned: layer %d keeps %d heads (1 .. %d)", l, t.k, d->heads);
      NB_CHECK(d->dtype != NBEST_BF16 || t.k % 2 == 0, NBEST_ERR_SHAPE, "encoder_infer_pruned(bf16): layer %d keeps %d heads - the bf16 "
               "GEMM tiles need an even count (N = 64 k a multiple of 128); carry a head whose gate is 0", l, t.k);
      NB_CHECK(t.dst_wqkv >= 0 && t.dst_wo >= 0 && t.dst_bqkv >= 0 && t.dst_wqkv % 8 == 0 && t.dst_wo % 8 == 0 && t.dst_bqkv % 4 == 0,
               NBEST_ERR_ALIGN, "encoder_infer_pruned: layer %d: image offsets must be non-negative multiples of 16 bytes", l);
    }
  }
  Fwd c = make_fwd(d, wts, prm, z, key_mask, stream);
  const bool fp8_pass = c.g.fp8;   // (false unless f8: the other entry points refuse desc.w8)
  if (fp8_pass) { c.q8 = true; c.arec = false; c.g.amax_new = nullptr; }   // static scales: no producer records
  const Ptrs& P = c.g.W;
  char* W = (char*)ws;
  const int64_t B = d->B;
  const int H = d->H, F = d->F, dt = d->dtype;
  void *cur = W + w.X0, *nxt = W + w.X1;   // the layer's input and output; they change places after every layer
  const LayerBufs b = infer_layer(w, ws, fp8_pass);
  auto probs = [&](int l) { return cls_attn ? cls_attn + (int64_t)l * B * d->heads * d->S : nullptr; };

  RUN(nbest_embed_ln_fwd(ids, seg, pos, P.W(d->off_word), P.W(d->off_type), P.W(d->off_pos), P.P(d->off_emb_ln_g), P.P(d->off_emb_ln_b),
                         cur, (float*)(W + w.emb_stats), z.M, H, d->ln_eps, dt, d->hidden_drop, d->seed, d->drop_stream_base,
                         (hipStream_t)stream));
  // the compact matrices of layer l (pr != NULL); the packed image serves the full-width GEMMs of layers 0 .. L-2 only
  auto pruned = [&](int l) {
    const nbest_head_prune_layer& t = pr->layers_host[l];
    const char *wb = (const char*)pr->w, *pb = (const char*)pr->w_packed;
    return PrunedLayer{t.k, wb + t.dst_wqkv * z.esz, pb ? pb + t.dst_wqkv * z.esz : nullptr, wb + t.dst_wo * z.esz,
                       pb ? pb + t.dst_wo * z.esz : nullptr, pr->bqkv + t.dst_bqkv};
  };
  // Token elimination (tp != NULL): layer l runs on dl, a copy of the descriptor with S = S_l, and on M = B S_l rows; without it S_l = S
  // throughout and dl is the descriptor.  `mask`: the key mask of the S_l tokens; `org`: their original positions (NULL: the identity).
  nbest_encoder_desc dl = *d;
  c.d = &dl;
  const uint8_t* mask = key_mask;
  const int32_t* org = nullptr;
  int side = 0;            // which of tw.org / tw.mask the next selection writes
  bool have_maskf = false;   // tw.maskf holds `mask` as floats (written by the first scored layer, then by every selection)
  for (int l = 0; l + 1 < d->L; ++l) {
    c.g.M = B * dl.S; c.key_mask = mask;
    if (pr) {
      const PrunedLayer pl = pruned(l);
      RUN(layer_forward(c, l, cur, nxt, b, nullptr, nullptr, &pl));
    } else {
      RUN(layer_forward(c, l, cur, nxt, b, b.x8, probs(l)));   // (fp8 pass: the next layer's x8 comes out of this LayerNorm)
    }
    std::swap(cur, nxt);
    if (!tp) continue;
    const int Sl = dl.S, k = std::min((int)tp->keep[l], Sl);
    if (k < Sl) {   // score from the layer's own attention (its qkv and lse are still in the workspace), select, gather into the free X
      hipStream_t st = (hipStream_t)stream;
      float *score = (float*)(W + tw.score), *maskf = (float*)(W + tw.maskf);
      int32_t *idx = (int32_t*)(W + tw.idx), *org_out = (int32_t*)(W + tw.org[side]);
      uint8_t* mask_out = (uint8_t*)(W + tw.mask[side]);
      if (!have_maskf) RUN(nbest_internal_mask_to_f32(mask, maskf, B * Sl, st));
      RUN(nbest_attention_rollout_step(b.qkv, mask, b.lse, maskf, score, 0.f, d->B, Sl, d->heads, 64, dt, stream));
      RUN(nbest_token_select(score, mask, org, k, idx, mask_out, maskf, org_out, d->B, Sl, stream));
      RUN(nbest_rows_compact(cur, idx, nxt, d->B, Sl, k, H, dt, stream));
      std::swap(cur, nxt);
      mask = mask_out; org = org_out; have_maskf = true; side ^= 1;
      dl.S = k;
    }
    if (tp->token_kept)
      RUN(nbest_internal_token_kept_row(org, tp->token_kept + (int64_t)l * B * d->S, d->B, d->S, dl.S, (hipStream_t)stream));
  }
  const int64_t M = B * dl.S, SH = (int64_t)dl.S * H;   // what reaches the last layer
  key_mask = mask;
  // last layer, CLS rows only (weights read unpacked: the packed images are laid out for the full-width GEMMs)
  const int l = d->L - 1;
  const nbest_layer_offsets& o = d->layers_host[l];
  const void* xin = cur;
  void* kv = b.qkv; void* q = b.ctx; void* cctx = b.r1; void* cx1 = b.x1; void* ch = b.hact; void* cr = b.r2;
  // pruned: Wqkv' [3 Hk][H] (Q rows, then K | V rows), bqkv', Wo' [H][Hk] and heads = k; Hk = H otherwise
  const PrunedLayer pl = pr ? pruned(l) : PrunedLayer{d->heads, P.W(o.wqkv), nullptr, P.W(o.wo), nullptr, P.P(o.bqkv)};
  const int heads = pl.k, Hk = 64 * heads;
  nbest_gemm_args g;
  if (fp8_pass) {   // K | V, all rows, in fp8: the e4m3 copy of the layer input against rows H .. 3H of the e4m3 QKV matrix (unpacked)
    if (l == 0) RUN(nbest_internal_cast_bf16_to_fp8(xin, b.x8, M * H, c.AP(0), nullptr, (hipStream_t)stream));
    nbest_gemm_fp8_args g8 = {};
    g8.A = b.x8; g8.B = (const uint8_t*)d->w8 + o.wqkv + (int64_t)H * H; g8.C = kv; g8.bias = P.P(o.bqkv) + H;
    g8.M = M; g8.N = 2 * H; g8.K = H; g8.lda = g8.ldb = H; g8.ldc = 2 * H;
    g8.epilogue = NBEST_EPI_BIAS; g8.out_scale = 1.f; g8.out_scale_dev = d->w8_inv_scale + 4 * l; g8.a_amax = d->aamax_prev + 4 * l;
    RUN(nbest_gemm_fp8(&g8, stream));
  } else {
    g = gemm_nt(dt, xin, (const char*)pl.wqkv + (size_t)Hk * H * z.esz, kv, M, 2 * Hk, H);   // K | V, all rows
    g.epilogue = NBEST_EPI_BIAS; g.bias = pl.bqkv + Hk;
    RUN(nbest_gemm(&g, stream));
    RUN(c.calib(xin, M * H, 4 * l));   // (calibration pass of the fp8 inference: the one fp8 GEMM input of this layer)
  }
  g = gemm_nt(dt, xin, pl.wqkv, q, B, Hk, H);                                             // Q, CLS rows (lda = S H)
  g.lda = SH; g.epilogue = NBEST_EPI_BIAS; g.bias = pl.bqkv;
  RUN(nbest_gemm(&g, stream));
  if (cls_attn) RUN(nbest_internal_attention_cls_probs(q, H, kv, 2 * H, key_mask, probs(l), d->S, d->B, d->S, d->heads, 64, dt, stream));
  RUN(nbest_attention_cls_fwd_internal(q, Hk, kv, 2 * Hk, key_mask, cctx, Hk, d->B, dl.S, heads, 64, dt, stream, 0.f, 0, 0));
  if (d->head_gate) RUN(nbest_head_gate_fwd(cctx, H, cctx, H, d->head_gate + (int64_t)l * d->heads, B, d->heads, 64, dt, stream));
  g = gemm_nt(dt, cctx, pl.wo, cr, B, H, Hk);
  g.epilogue = NBEST_EPI_BIAS_DROP_RES; g.bias = P.P(o.bo); g.R = xin; g.ldr = SH;        // residual: the CLS rows
  RUN(nbest_gemm(&g, stream));
  RUN(nbest_internal_layernorm_fwd8(cr, P.P(o.ln1_g), P.P(o.ln1_b), cx1, nullptr, b.st1, B, H, d->ln_eps, dt, stream, nullptr, nullptr));
  g = gemm_nt(dt, cx1, P.W(o.w1), ch, B, F, H);
  g.epilogue = NBEST_EPI_BIAS_GELU; g.bias = P.P(o.b1); g.ldu = F;
  RUN(nbest_gemm(&g, stream));
  g = gemm_nt(dt, ch, P.W(o.w2), cr, B, H, F);
  g.epilogue = NBEST_EPI_BIAS_DROP_RES; g.bias = P.P(o.b2); g.R = cx1; g.ldr = H;
  RUN(nbest_gemm(&g, stream));
  RUN(nbest_internal_layernorm_fwd8(cr, P.P(o.ln2_g), P.P(o.ln2_b), cls_out, nullptr, b.st2, B, H, d->ln_eps, dt, stream, nullptr, nullptr));
  return NBEST_OK;
}

extern "C" int nbest_encoder_infer_attn(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                                        const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out,
                                        float* cls_attn, nbest_stream_t stream) {
  return infer_impl(d, wts, prm, ids, seg, pos, key_mask, ws, ws_bytes, cls_out, cls_attn, nullptr, stream);
}

extern "C" int nbest_encoder_infer_pruned(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids,
                                          const int64_t* seg, const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes,
                                          void* cls_out, const nbest_head_prune_images* images, nbest_stream_t stream) {
  NB_CHECK(images, NBEST_ERR_ARG, "encoder_infer_pruned: null images");
  return infer_impl(d, wts, prm, ids, seg, pos, key_mask, ws, ws_bytes, cls_out, nullptr, images, stream);
}

extern "C" int nbest_encoder_infer(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                                   const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out,
                                   nbest_stream_t stream) {
  return nbest_encoder_infer_attn(d, wts, prm, ids, seg, pos, key_mask, ws, ws_bytes, cls_out, nullptr, stream);
}

extern "C" int nbest_encoder_infer_tokens(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                                          const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out,
                                          const int32_t* keep_host, int n_keep, int32_t* token_kept, nbest_stream_t stream) {
  NB_CHECK(d, NBEST_ERR_ARG, "encoder_infer_tokens: null descriptor");
  NB_CHECK(n_keep == d->L - 1, NBEST_ERR_ARG, "encoder_infer_tokens: the schedule has %d entries, L - 1 = %d are needed", n_keep, d->L - 1);
  NB_CHECK(keep_host || n_keep == 0, NBEST_ERR_ARG, "encoder_infer_tokens: null schedule");
  const TokenPrune tp = {keep_host, token_kept};
  return infer_impl(d, wts, prm, ids, seg, pos, key_mask, ws, ws_bytes, cls_out, nullptr, nullptr, stream, false, &tp);
}

extern "C" int nbest_encoder_infer_fp8(const nbest_encoder_desc* d, const void* wts, const float* prm, const int64_t* ids, const int64_t* seg,
                                       const int64_t* pos, const uint8_t* key_mask, void* ws, size_t ws_bytes, void* cls_out,
                                       nbest_stream_t stream) {
  return infer_impl(d, wts, prm, ids, seg, pos, key_mask, ws, ws_bytes, cls_out, nullptr, nullptr, stream, true);
}
