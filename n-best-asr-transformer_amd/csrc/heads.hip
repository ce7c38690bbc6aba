// K7 STC heads + losses (forward and analytic backward), K8 CLS-MSE, K10 decode.
//
// Shapes are tiny (B x 171 x 768 for bert-base on DSTC2), so everything is fp32 VALU work in two launches
// (heads_fwd_kernel, heads_bwd_kernel); the point is to replace ~40 tiny launches + 4 host syncs of the reference
// (/root/reference/models/modules/hierarchical_classifier.py:35-60, /root/reference/n_best_asr_bert.py:160-195) and to hand
// dCLS to the encoder backward.
//
// Workspace layout: HeadsWs.  LDS layout of heads_fwd_kernel: HeadsLds.
#include "common.h"

namespace {
enum { kPlain = 0, kKd = 1, kKdT = 2, kRDrop = 3 };   // the soft term of a heads call (heads_fwd_kernel<T, MODE>)

// The workspace of a heads call, as byte offsets.  nbest_heads_ws_bytes is ABI: the reserved region (never written) keeps its size.
struct HeadsWs {
  size_t cls, reserved, dz, sloss, mw, lay_row, bytes;
  HeadsWs(int B, int R, int H) {
    cls = 0;                                                         // float [B][H]: the CLS rows in fp32
    reserved = cls + (size_t)B * H * sizeof(float);                  // float [B][R]
    dz = reserved + (size_t)B * R * sizeof(float);                   // float [B][R]: d(loss)/d(logits)
    sloss = dz + (size_t)B * R * sizeof(float);                      // float [B][4]: per-sample losses
    mw = sloss + (size_t)4 * B * sizeof(float);                      // uint32 [<= R + 1 layers][B][ceil(H / 32)]: dropout mask bits
    lay_row = mw + (size_t)(R + 1) * B * ((H + 31) / 32) * sizeof(uint32_t);   // int32 [R]: classifier layer of a head row
    bytes = lay_row + (size_t)R * sizeof(int32_t);
  }
  template <typename T> static T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }
};

// The dynamic LDS of heads_fwd_kernel, as offsets in 4-byte words: the kernel takes its pointers from it, heads_launch the byte count.
struct HeadsLds {
  int z, lay, mk, lsum, soft, row2, x2, mk2, words;
  __host__ __device__ HeadsLds(int H, int R, int n_lay, int waves, int mode) {
    const int M = n_lay * ((H + 31) >> 5);
    z = H;                                                           // float [R]: the logits, after float [H]: the CLS row
    lay = z + R;                                                     // int32 [R]: classifier layer of a row
    mk = lay + R;                                                    // uint32 [n_lay][W]: the layers' mask words
    lsum = mk + M;                                                   // float [waves][3]: partials of the three hard losses
    soft = lsum + 3 * waves;                                         // float [waves]: partials of the soft term (all but kPlain)
    row2 = soft + (mode != kPlain ? waves : 0);                      // float [R]: the second row of logits (kKdT: the teacher's, kRDrop: the twin's)
    x2 = row2 + (mode == kKdT || mode == kRDrop ? R : 0);            // float [H]: kRDrop, the twin's CLS row
    mk2 = x2 + (mode == kRDrop ? H : 0);                             // uint32 [n_lay][W]: kRDrop, the twin's mask words
    words = mk2 + (mode == kRDrop ? M : 0);
  }
  __host__ __device__ size_t bytes() const { return (size_t)words * 4; }
};

// the classifier layer of head row r: 0 for the top classifier, k for the k-th softmax head (heads lie in increasing top order)
__device__ __forceinline__ int layer_of_row(int r, const int32_t* __restrict__ head_row, int n_top) {
  if (r < n_top) return 0;
  int lay = 0, k = 0;
  for (int t = 0; t < n_top; ++t) {
    const int hr = head_row[t];
    if (hr >= 0) {
      ++k;
      if (hr <= r) lay = k;
    }
  }
  return lay;
}

// The 1 + n_heads dropout masks of a step (one per linear layer of the hierarchical classifier, each over [B][H]) are hashed ONCE
// and kept as bits: mw[(layer * B + b) * W + (h >> 5)], W = ceil(H / 32) words per row.  Every head row of a layer shares its
// layer's mask, so hashing per (row, b, h) in the three kernels below repeated the same 14-instruction decision R / n_layers = 14
// times (34 M hashes per kernel at B = 256); the bits are the same decisions (nb_keep), so nothing changes numerically.
__device__ __forceinline__ void heads_mask_words(const DropCfg& drop, int lay, int b, int B, int H, int W, uint32_t* lds_row,
                                                 uint32_t* __restrict__ glob_row) {
  const int lane = threadIdx.x & 63;
  for (int h0 = (threadIdx.x & ~63); h0 < H; h0 += blockDim.x) {
    const int h = h0 + lane;
    const bool keep = (h < H) && nb_keep(drop, (uint32_t)((lay * B + b) * H + h));
    const uint64_t bal = __ballot(keep);
    if (lane == 0) {
      const int w = h0 >> 5;
      lds_row[w] = (uint32_t)bal;
      if (w + 1 < W) lds_row[w + 1] = (uint32_t)(bal >> 32);
      if (glob_row) {
        glob_row[w] = (uint32_t)bal;
        if (w + 1 < W) glob_row[w + 1] = (uint32_t)(bal >> 32);
      }
    }
  }
}

// the four loss sums over the batch, each in a fixed order (every thread of the block calls it)
__device__ __forceinline__ void loss_sums(const float* __restrict__ sample_loss, int B, float* __restrict__ out) {
  __shared__ float sm[16];
  for (int k = 0; k < 4; ++k) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) s += sample_loss[4 * b + k];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) out[k] = s;
  }
}

__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ sample_loss, int B, float* __restrict__ out) {
  loss_sums(sample_loss, B, out);
}

// a wave's logit of one head row of heads_fwd_kernel, without the bias (mrow: the mask words of the row's layer, read only under dropout)
__device__ __forceinline__ float wave_logit(const float* __restrict__ w, const float* x, const uint32_t* mrow, const DropCfg& drop, int H,
                                            int lane) {
  float s = 0.f;
#pragma unroll 4
  for (int h = lane; h < H; h += 64) {
    float xv = x[h];
    if (drop.thr16) xv = ((mrow[h >> 5] >> (h & 31)) & 1u) ? xv * drop.scale : 0.f;
    s = fmaf(w[h], xv, s);
  }
  return wave_sum(s);
}

// ---- the heads as TWO launches ---------------------------------------------------------------------------------------------------
// heads_fwd_kernel: one block per sample - CLS row and the layers' dropout bits into LDS (laid out by HeadsLds), the R logits (a wave
// per row, wave_logit), then scores / losses / d(loss)/d(logits) with the TOP labels spread over the waves, lanes over a head's columns.
// heads_bwd_kernel: weight gradient and input gradient in one grid (blocks [0, nW): an 8-row x 64-column tile of dWh, waves split the
// batch, the CLS column chunk loaded once per sample for all 8 rows; blocks [nW, nW + nD): 8 samples x 64 columns of dCLS, waves split
// the head rows, the weight element loaded once for all 8 samples); the last block sums the per-sample losses.  Fixed-order sums.
//
// heads_fwd_kernel<T, MODE> is the plain kernel plus one soft term, whose sum goes to sample_loss[4 b + 3].  Every hard statement is
// the plain instantiation's; what a mode adds sits under `if constexpr`.
// kKd, kKdT (distillation): the three hard terms with a teacher's outputs in place of the labels - the targets of the two BCEs, and
// the teacher's distribution over a head's columns where the hard term has the one-hot class; d(logits) = (1 - alpha) d_hard + w d_soft
// (dz is linear in the upstream gradient, so the two are blended per logit).  SoftView yields, per top label and per head column, the
// student's soft scores (pS, sS, fS), the teacher's targets (tt, tb, tf) and w, so the soft statements stand once in each of their
// four places: the single-bottom branch, the accumulate pass, the dz pass, the top-label epilogue.
//   kKd  (nbest_stc_heads_kd): the hard scores against the teacher's fp32 probabilities t_top / t_bott / t_fin; w = alpha.
//   kKdT (nbest_stc_heads_kd_t): the teacher comes as its LOGITS t_logits [B][R], staged in LDS as the second row.  Both rows are
//        softened by 1 / T: p_T = sigmoid(z_t / T), s_T = softmax(z / T), f_T = p_T s_T of the two models; loss = T^2 x the soft loss
//        of those, w = alpha x T (T^2 of the loss x 1 / T of du / dz).  The student's tempered max is max(z) / T.
// Each keeps its reduction tree (kKd: two wave_sum, kKdT: one wave_sum2; they round differently).
// kRDrop (nbest_stc_heads_rdrop): rows b and b + B / 2 of the batch are twins (one utterance under two sets of dropout bits).  The
// block of row b also stages its twin's CLS row and mask words and forms the twin's R logits in the logits loop from the same read of
// the weights, with the twin's arithmetic in its order (the twin's block computes the same bits for them): the second row.  The pair's
// consistency term is the symmetric KL of the model's factorisation, in its logarithm-free form
//   R = sum_t 1/2 (p_t - p'_t)(z_t - z'_t) + (1 / n_heads) sum_k 1/2 sum_j (s_kj - s'_kj)(z_kj - z'_kj)
// (no term on final); each block of a pair writes R / 2 into sample_loss[4 b + 3] and dz = dz_hard + alpha dR/dz(own row).  Another
// formula, so its own statements.  The differences of scores are formed under fp contract(off): equal twins give dR/dz = 0 exactly,
// alpha = 0 the plain kernel's bits.
// The second row's per-head max and exp-sum ride in the student's passes over the columns (independent shuffle chains: latency-bound).
struct KdArgs {
  const float* t_top;   // [B][n_top]        (kKdT: t_logits [B][R])
  const float* t_bott;  // [B][R - n_top]
  const float* t_fin;   // [B][n_bottom]
  float alpha, temperature;   // temperature: kKdT only
};

// a - b that never fuses with a product feeding it (the device default contracts a * b - c into an fma; e * inv - e * inv must be 0)
__device__ __forceinline__ float sub_exact(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__device__ __forceinline__ float bce_term(float p, float y) {
  return -(y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(logf(1.f - p), -100.f));
}

// The distillation term of one sample: filled from the teacher's arrays (kKd) or the two rows of logits in LDS (kKdT); inert otherwise.
template <int MODE>
struct SoftView {
  struct Col { float sS, fS, tb, tf; };   // a head column: the student's soft softmax and final score, the teacher's
  const float *z, *z2;                     // kKdT: the two rows of logits in LDS
  const float *ttop, *tbot, *tfin;         // kKd: the teacher's rows of this sample
  float invT, w;                           // 1 / T (kKdT); the weight of the soft gradient in dz: alpha (kKd), alpha x T (kKdT)
  float pS = 0.f, qT = 0.f;                // per top label: the student's soft top score; kKdT: the teacher's
  __device__ void top(int t, float zt, float pt) {                                         // the soft top scores of label t
    pS = MODE == kKdT ? 1.0f / (1.0f + __expf(-zt * invT)) : pt;
    if constexpr (MODE == kKdT) qT = 1.0f / (1.0f + __expf(-z2[t] * invT));
  }
  __device__ float tt(int t) const { return MODE == kKdT ? qT : ttop[t]; }                 // the target of the top BCE
  __device__ float tf_single(int bi) const { return MODE == kKdT ? qT : tfin[bi]; }        // single bottom: final = top score, of both models
  // column c = hr + j of a head (jb = c - n_top, bi its bottom label): s, f the hard scores; mx, mx2 the rows' maxima, invs, inv2 1 / the tempered sums
  __device__ Col col(int c, int jb, int bi, float s, float f, float mx, float mx2, float invs, float inv2) const {
    if constexpr (MODE != kKdT) return {s, f, tbot[jb], tfin[bi]};
    const float sT = __expf((z[c] - mx) * invT) * invs, tb = __expf((z2[c] - mx2) * invT) * inv2;
    return {sT, pS * sT, tb, qT * tb};
  }
};

constexpr int kFwdThreads = 512;
template <typename T, int MODE>
__global__ __launch_bounds__(kFwdThreads) void heads_fwd_kernel(const void* __restrict__ hidden_, int64_t cls_stride, const float* __restrict__ Wh,
                                                                 const float* __restrict__ bh, const float* __restrict__ labels,
                                                                 const int32_t* __restrict__ bottom_off, const int32_t* __restrict__ bottom_ids,
                                                                 const int32_t* __restrict__ head_row, int n_top, int n_bottom, int R, int H,
                                                                 int n_heads, int n_lay, float* __restrict__ cls_out, float* __restrict__ top,
                                                                 float* __restrict__ bott, float* __restrict__ fin, float* __restrict__ dz,
                                                                 float* __restrict__ sample_loss, uint32_t* __restrict__ mw,
                                                                 int32_t* __restrict__ lay_row, DropCfg drop, KdArgs kd) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // HeadsLds
  constexpr bool KD = MODE == kKd, KDT = MODE == kKdT, RD = MODE == kRDrop, SOFT = KD || KDT, ROW2 = KDT || RD;
  const int b = blockIdx.x, B = gridDim.x, W = (H + 31) >> 5;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const HeadsLds L(H, R, n_lay, nw, MODE);
  float* z = xs + L.z;
  int32_t* lay_s = (int32_t*)(xs + L.lay);
  uint32_t* mk = (uint32_t*)(xs + L.mk);
  float* lsum = xs + L.lsum;
  float* z2 = xs + L.row2;                                  // ROW2: the teacher's (kKdT) or the twin's (kRDrop) row of logits
  float* xt = xs + L.x2;                                    // RD: the twin's CLS row and mask words
  uint32_t* mkt = (uint32_t*)(xs + L.mk2);
  const T* hidden = (const T*)hidden_;
  const T* x = hidden + (int64_t)b * cls_stride;
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    const float v = to_f<T>(x[h]);
    xs[h] = v;
    cls_out[(int64_t)b * H + h] = v;
  }
  if constexpr (KDT)
    for (int r = threadIdx.x; r < R; r += blockDim.x) z2[r] = kd.t_top[(int64_t)b * R + r];
  if constexpr (RD) {
    const int bt = b < (B >> 1) ? b + (B >> 1) : b - (B >> 1);
    const T* x2 = hidden + (int64_t)bt * cls_stride;
    for (int h = threadIdx.x; h < H; h += blockDim.x) xt[h] = to_f<T>(x2[h]);
    if (drop.thr16)
      for (int lay = 0; lay < n_lay; ++lay) heads_mask_words(drop, lay, bt, B, H, W, mkt + lay * W, nullptr);
  }
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const int l = layer_of_row(r, head_row, n_top);
    lay_s[r] = l;
    if (b == 0) lay_row[r] = l;
  }
  if (drop.thr16)
    for (int lay = 0; lay < n_lay; ++lay) heads_mask_words(drop, lay, b, B, H, W, mk + lay * W, mw + ((int64_t)lay * B + b) * W);
  __syncthreads();
  for (int r = wave; r < R; r += nw) {
    const float* w = Wh + (int64_t)r * H;
    const uint32_t* mrow = mk + lay_s[r] * W;
    if constexpr (RD) {                                     // the twin's logit next to the row's own: one read of the weights
      const uint32_t* mrow2 = mkt + lay_s[r] * W;
      float s = 0.f, s2 = 0.f;
#pragma unroll 4
      for (int h = lane; h < H; h += 64) {
        float xv = xs[h], xv2 = xt[h];
        if (drop.thr16) {
          xv = ((mrow[h >> 5] >> (h & 31)) & 1u) ? xv * drop.scale : 0.f;
          xv2 = ((mrow2[h >> 5] >> (h & 31)) & 1u) ? xv2 * drop.scale : 0.f;
        }
        const float wv = w[h];
        s = fmaf(wv, xv, s);
        s2 = fmaf(wv, xv2, s2);
      }
      s = wave_sum(s);
      s2 = wave_sum(s2);
      if (lane == 0) {
        z[r] = s + bh[r];
        z2[r] = s2 + bh[r];
      }
    } else {
      const float s = wave_logit(w, xs, mrow, drop, H, lane);
      if (lane == 0) z[r] = s + bh[r];
    }
  }
  __syncthreads();
  const float* y = labels + (int64_t)b * n_bottom;
  float l_bot = 0.f, l_top = 0.f, l_ce = 0.f;
  float l_soft = 0.f;                                       // every lane's own share of the soft term
  SoftView<MODE> sv{z, z2, KD ? kd.t_top + (int64_t)b * n_top : nullptr, KD ? kd.t_bott + (int64_t)b * (R - n_top) : nullptr,
                    KD ? kd.t_fin + (int64_t)b * n_bottom : nullptr, KDT ? 1.0f / kd.temperature : 1.f,
                    KDT ? kd.alpha * kd.temperature : kd.alpha};
  const float wh = 1.f - kd.alpha;
  for (int t = wave; t < n_top; t += nw) {                  // a wave per top label (lanes parallelise the head columns)
    const int o0 = bottom_off[t], nk = bottom_off[t + 1] - o0, hr = head_row[t];
    const float zt = z[t];
    const float pt = 1.0f / (1.0f + __expf(-zt));
    float dpt = 0.f;  // d(loss)/d(top score)
    float ytop = 0.f;
    float dpt_s = 0.f;  // SOFT: d(soft loss)/d(soft top score)
    if constexpr (SOFT) sv.top(t, zt, pt);
    const float ptw = RD ? 1.0f / (1.0f + __expf(-z2[t])) : 0.f, dzt = RD ? zt - z2[t] : 0.f;   // RD: the twin's top score, z_t - z'_t
    if (hr < 0) {
      const int bi = bottom_ids[o0];                        // single bottom label: final = top score
      const float yy = y[bi];
      ytop = yy;
      if (lane == 0) {
        fin[(int64_t)b * n_bottom + bi] = pt;
        l_bot += -(yy * fmaxf(logf(pt), -100.f) + (1.f - yy) * fmaxf(logf(1.f - pt), -100.f));
      }
      dpt += (pt - yy) / fmaxf(pt * (1.f - pt), 1e-12f);
      if constexpr (SOFT) {
        const float tf = sv.tf_single(bi);
        if (lane == 0) l_soft += bce_term(sv.pS, tf);
        dpt_s += (sv.pS - tf) / fmaxf(sv.pS * (1.f - sv.pS), 1e-12f);
      }
    } else {
      float mx = -INFINITY;                                 // softmax head over nk columns (nk may exceed 64: strided)
      float mx2 = -INFINITY;                                // ROW2: the second row's max, in the same pass
      for (int j = lane; j < nk; j += 64) {
        mx = fmaxf(mx, z[hr + j]);
        if constexpr (ROW2) mx2 = fmaxf(mx2, z2[hr + j]);
      }
      mx = wave_max(mx);
      if constexpr (ROW2) mx2 = wave_max(mx2);
      float se = 0.f;
      float seT = 0.f, se2 = 0.f;                           // KDT: sum of exp((z - max) / T) (max(z / T) = max(z) / T); ROW2: the second row's sum
      for (int j = lane; j < nk; j += 64) {
        se += __expf(z[hr + j] - mx);
        if constexpr (KDT) {
          seT += __expf((z[hr + j] - mx) * sv.invT);
          se2 += __expf((z2[hr + j] - mx2) * sv.invT);
        }
        if constexpr (RD) se2 += __expf(z2[hr + j] - mx2);   // the twin's sum, in the row's own order
      }
      se = wave_sum(se);
      if constexpr (KDT) wave_sum2(seT, se2);
      if constexpr (RD) se2 = wave_sum(se2);
      const float inv = 1.0f / se;
      const float invsT = KDT ? 1.0f / seT : 0.f, inv2 = ROW2 ? 1.0f / se2 : 0.f;
      const float wr = 0.5f / (float)n_heads;               // RD: the weight of a head's term
      int idx = nk - 1;                                     // class index: the active bottom label, else the last column (NONE)
      float ysum = 0.f;
      for (int j = lane; j < nk; j += 64) {
        const float yy = y[bottom_ids[o0 + j]];
        ysum += yy;
        if (yy > 0.5f) idx = min(idx, j);
      }
      ysum = wave_sum(ysum);
      for (int o = 32; o > 0; o >>= 1) idx = min(idx, __shfl_xor(idx, o, 64));
      if (ysum == 0.f) idx = nk - 1;
      ytop = ysum;
      float dot = 0.f, dtop_acc = 0.f, lb = 0.f;
      float dot_s = 0.f, dtop_s = 0.f;
      for (int j = lane; j < nk; j += 64) {                 // the accumulate pass
        const float s = __expf(z[hr + j] - mx) * inv;
        const int bi = bottom_ids[o0 + j];
        const float yy = y[bi];
        const float f = pt * s;
        fin[(int64_t)b * n_bottom + bi] = f;
        bott[(int64_t)b * (R - n_top) + (hr - n_top) + j] = s;
        lb += -(yy * fmaxf(logf(f), -100.f) + (1.f - yy) * fmaxf(logf(1.f - f), -100.f));
        const float gf = (f - yy) / fmaxf(f * (1.f - f), 1e-12f);
        float ds = gf * pt;
        if (j == idx) ds += -1.0f / ((s + 1e-12f) * (float)n_heads);
        dot += ds * s;
        dtop_acc += gf * s;
        if constexpr (SOFT) {
          const auto c = sv.col(hr + j, (hr - n_top) + j, bi, s, f, mx, mx2, invsT, inv2);
          l_soft += bce_term(c.fS, c.tf);
          const float gs = (c.fS - c.tf) / fmaxf(c.fS * (1.f - c.fS), 1e-12f);
          const float dss = gs * sv.pS - c.tb / ((c.sS + 1e-12f) * (float)n_heads);
          dot_s += dss * c.sS;
          dtop_s += gs * c.sS;
        }
        if constexpr (RD) {                                 // 1/2 (s - s')(z - z') and sum_j s_j (z_j - z'_j)
          const float sw = __expf(z2[hr + j] - mx2) * inv2, dzz = z[hr + j] - z2[hr + j];
          l_soft += wr * (sub_exact(s, sw) * dzz);
          dot_s += s * dzz;
        }
      }
      if constexpr (RD) dot_s = wave_sum(dot_s);
      dot = wave_sum(dot);
      dpt += wave_sum(dtop_acc);
      if constexpr (KD) {
        dot_s = wave_sum(dot_s);
        dpt_s += wave_sum(dtop_s);
      }
      if constexpr (KDT) {
        wave_sum2(dot_s, dtop_s);
        dpt_s += dtop_s;
      }
      l_bot += wave_sum(lb) * (lane == 0 ? 1.f : 0.f);
      for (int j = lane; j < nk; j += 64) {                 // the dz pass
        const float s = __expf(z[hr + j] - mx) * inv;
        const int bi = bottom_ids[o0 + j];
        const float yy = y[bi];
        const float f = pt * s;
        const float gf = (f - yy) / fmaxf(f * (1.f - f), 1e-12f);
        float ds = gf * pt;
        if (j == idx) {
          ds += -1.0f / ((s + 1e-12f) * (float)n_heads);
          l_ce += -logf(s + 1e-12f) / (float)n_heads;
        }
        if constexpr (SOFT) {
          const auto c = sv.col(hr + j, (hr - n_top) + j, bi, s, f, mx, mx2, invsT, inv2);
          const float gs = (c.fS - c.tf) / fmaxf(c.fS * (1.f - c.fS), 1e-12f);
          const float dss = gs * sv.pS - c.tb / ((c.sS + 1e-12f) * (float)n_heads);
          l_soft += -c.tb * logf(c.sS + 1e-12f) / (float)n_heads;
          // alpha = 0 gives the plain kernel's bits because the soft term is finite (|gs|, tb / (sS + 1e-12) <= 1e12): 1 * x + 0 * y = x
          dz[(int64_t)b * R + hr + j] = wh * (s * (ds - dot)) + sv.w * (c.sS * (dss - dot_s));
        } else if constexpr (RD) {
          const float sw = __expf(z2[hr + j] - mx2) * inv2, dzz = z[hr + j] - z2[hr + j];
          const float dr = wr * (sub_exact(s, sw) + s * (dzz - dot_s));
          // alpha = 0 gives the plain kernel's bits (dr is finite: x + 0 * y = x), equal twins give dr = 0
          dz[(int64_t)b * R + hr + j] = s * (ds - dot) + kd.alpha * dr;
        } else {
          dz[(int64_t)b * R + hr + j] = s * (ds - dot);
        }
      }
    }
    if (lane == 0) l_top += -(ytop * fmaxf(logf(pt), -100.f) + (1.f - ytop) * fmaxf(logf(1.f - pt), -100.f));   // top BCE against y . B2T
    dpt += (pt - ytop) / fmaxf(pt * (1.f - pt), 1e-12f);
    if constexpr (SOFT) {
      const float tt = sv.tt(t);
      if (lane == 0) l_soft += bce_term(sv.pS, tt);
      dpt_s += (sv.pS - tt) / fmaxf(sv.pS * (1.f - sv.pS), 1e-12f);
    }
    if constexpr (RD)
      if (lane == 0) l_soft += 0.5f * ((pt - ptw) * dzt);
    if (lane == 0) {
      top[(int64_t)b * n_top + t] = pt;
      if constexpr (SOFT) dz[(int64_t)b * R + t] = wh * (dpt * pt * (1.f - pt)) + sv.w * (dpt_s * sv.pS * (1.f - sv.pS));
      else if constexpr (RD) dz[(int64_t)b * R + t] = dpt * pt * (1.f - pt) + kd.alpha * (0.5f * (pt * (1.f - pt) * dzt + (pt - ptw)));
      else dz[(int64_t)b * R + t] = dpt * pt * (1.f - pt);
    }
  }
  l_ce = wave_sum(l_ce);
  if (lane == 0) { lsum[3 * wave] = l_bot; lsum[3 * wave + 1] = l_top; lsum[3 * wave + 2] = l_ce; }
  if constexpr (MODE != kPlain) {
    l_soft = wave_sum(l_soft);
    if (lane == 0) xs[L.soft + wave] = l_soft;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float v = 0.f;
    for (int w = 0; w < nw; ++w) v += lsum[3 * w + threadIdx.x];     // wave order: the same sum on every run
    sample_loss[4 * b + threadIdx.x] = v;
  }
  if (threadIdx.x == 3) {
    float v = 0.f;
    if constexpr (MODE != kPlain)
      for (int w = 0; w < nw; ++w) v += xs[L.soft + w];
    if constexpr (KDT) v *= kd.temperature * kd.temperature;
    if constexpr (RD) v *= 0.5f;                             // each block of a pair carries half of the pair's term
    sample_loss[4 * b + 3] = v;
  }
}

constexpr int kBwdRows = 8;      // head rows (wgrad) / samples (dgrad) per block
__global__ __launch_bounds__(256) void heads_bwd_kernel(const float* __restrict__ cls, const float* __restrict__ dz, const float* __restrict__ Wh,
                                                        int B, int R, int H, float* __restrict__ dWh, float* __restrict__ dbh,
                                                        float* __restrict__ dcls, int accumulate, const uint32_t* __restrict__ mw,
                                                        const int32_t* __restrict__ lay_row, DropCfg drop, const float* __restrict__ sample_loss,
                                                        float* __restrict__ loss_out, int nW) {
  __shared__ float red[4][kBwdRows][64];
  __shared__ float redb[4][kBwdRows];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nh = (H + 63) >> 6, W = (H + 31) >> 5;
  const int bid = blockIdx.x;
  if (bid < nW) {
    // ---- dWh[r][h] = sum_b dz[b][r] * drop_{layer(r)}(cls[b][h]); dbh[r] = sum_b dz[b][r] ----
    const int r0 = (bid / nh) * kBwdRows, h = (bid % nh) * 64 + lane;
    const bool hv = h < H;
    int lay[kBwdRows];
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) lay[j] = lay_row[min(r0 + j, R - 1)];
    float acc[kBwdRows], sb[kBwdRows];
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) acc[j] = sb[j] = 0.f;
    for (int b = wave; b < B; b += 4) {
      const float xv = hv ? cls[(int64_t)b * H + h] : 0.f;
      const float xd = xv * drop.scale;
#pragma unroll
      for (int j = 0; j < kBwdRows; ++j) {
        const float g = (r0 + j < R) ? dz[(int64_t)b * R + r0 + j] : 0.f;
        float xm = xv;
        if (drop.thr16) xm = (hv && ((mw[((int64_t)lay[j] * B + b) * W + (h >> 5)] >> (h & 31)) & 1u)) ? xd : 0.f;
        acc[j] = fmaf(g, xm, acc[j]);
        sb[j] += g;
      }
    }
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) {
      red[wave][j][lane] = acc[j];
      if (lane == 0) redb[wave][j] = sb[j];
    }
    __syncthreads();
    for (int j = wave; j < kBwdRows; j += 4) {
      const int r = r0 + j;
      if (r < R && hv) {
        const float v = (red[0][j][lane] + red[1][j][lane]) + (red[2][j][lane] + red[3][j][lane]);
        float* o = dWh + (int64_t)r * H + h;
        *o = accumulate ? *o + v : v;
      }
      if (r < R && lane == 0 && (bid % nh) == 0) {
        const float v = (redb[0][j] + redb[1][j]) + (redb[2][j] + redb[3][j]);
        dbh[r] = accumulate ? dbh[r] + v : v;
      }
    }
    return;
  }
  const int nD = ((B + kBwdRows - 1) / kBwdRows) * nh;
  if (bid < nW + nD) {
    // ---- dcls[b][h] = sum_r dz[b][r] * Wh[r][h] * dropmask_{layer(r)}(b, h) ----
    const int q = bid - nW, b0 = (q / nh) * kBwdRows, h = (q % nh) * 64 + lane;
    const bool hv = h < H;
    float acc[kBwdRows];
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) acc[j] = 0.f;
    for (int r = wave; r < R; r += 4) {
      const float w = hv ? Wh[(int64_t)r * H + h] : 0.f;
      const float wd = w * drop.scale;
      const int lay = lay_row[r];
#pragma unroll
      for (int j = 0; j < kBwdRows; ++j) {
        const int b = min(b0 + j, B - 1);
        const float g = dz[(int64_t)b * R + r];
        float wm = w;
        if (drop.thr16) wm = (hv && ((mw[((int64_t)lay * B + b) * W + (h >> 5)] >> (h & 31)) & 1u)) ? wd : 0.f;
        acc[j] = fmaf(g, wm, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) red[wave][j][lane] = acc[j];
    __syncthreads();
    for (int j = wave; j < kBwdRows; j += 4) {
      const int b = b0 + j;
      if (b < B && hv) dcls[(int64_t)b * H + h] = (red[0][j][lane] + red[1][j][lane]) + (red[2][j][lane] + red[3][j][lane]);
    }
    return;
  }
  // ---- last block (launched only with loss_out): the four loss sums over the batch (fixed order) ----
  if (loss_out) loss_sums(sample_loss, B, loss_out);
}

// d(logits) from ARBITRARY upstream gradients of the three outputs (the autograd bridge: the reference's loop calls
// total_loss.backward() on whatever it built from top / bottoms / final, /root/reference/n_best_asr_bert.py:255-264):
//   final[b][bi] = top_t (single-bottom top) | top_t * s_j ;  s = softmax(head logits) ;  top = sigmoid(z_t)
// grid B, block 256: a wave per top label, lanes over the head columns (as heads_fwd_kernel).
__global__ __launch_bounds__(256) void heads_vjp_dz_kernel(const float* __restrict__ top, const float* __restrict__ bott,
                                                           const float* __restrict__ dtop, const float* __restrict__ dbott,
                                                           const float* __restrict__ dfin, const int32_t* __restrict__ bottom_off,
                                                           const int32_t* __restrict__ bottom_ids, const int32_t* __restrict__ head_row,
                                                           int n_top, int n_bottom, int R, float* __restrict__ dz) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const float* gf = dfin + (int64_t)b * n_bottom;
  for (int t = wave; t < n_top; t += nw) {
    const int o0 = bottom_off[t], nk = bottom_off[t + 1] - o0, hr = head_row[t];
    const float pt = top[(int64_t)b * n_top + t];
    float dpt = dtop[(int64_t)b * n_top + t];
    if (hr < 0) {
      dpt += gf[bottom_ids[o0]];
    } else {
      const float* sb = bott + (int64_t)b * (R - n_top) + (hr - n_top);
      const float* gb = dbott + (int64_t)b * (R - n_top) + (hr - n_top);
      float dot = 0.f, acc = 0.f;
      for (int j = lane; j < nk; j += 64) {
        const float s = sb[j], g = gf[bottom_ids[o0 + j]];
        const float ds = gb[j] + g * pt;
        dot += ds * s;
        acc += g * s;
      }
      dot = wave_sum(dot);
      dpt += wave_sum(acc);
      for (int j = lane; j < nk; j += 64) {
        const float s = sb[j];
        const float ds = gb[j] + gf[bottom_ids[o0 + j]] * pt;
        dz[(int64_t)b * R + hr + j] = s * (ds - dot);
      }
    }
    if (lane == 0) dz[(int64_t)b * R + t] = dpt * pt * (1.f - pt);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cls_mse_kernel(const T* __restrict__ ha, int64_t sa, const T* __restrict__ ht, int64_t st_,
                                                      float* __restrict__ loss, float* __restrict__ da, float* __restrict__ dt,
                                                      int B, int H, float grad_scale) {
  __shared__ float sm[16];
  const int64_t n = (int64_t)B * H;
  const float c = 2.0f * grad_scale / (float)n;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const int b = (int)(i / H), h = (int)(i - (int64_t)b * H);
    const float d = to_f<T>(ha[b * sa + h]) - to_f<T>(ht[b * st_ + h]);
    s += d * d;
    if (da) da[i] += c * d;
    if (dt) dt[i] = -c * d;
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) loss[0] = s / (float)n;
}

__global__ void decode_kernel(const float* __restrict__ top, const float* __restrict__ bott, const int32_t* __restrict__ bottom_off,
                              const int32_t* __restrict__ bottom_ids, const int32_t* __restrict__ head_row,
                              const uint8_t* __restrict__ none_flag, int n_top, int R, int32_t* __restrict__ pred, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * n_top) return;
  const int b = i / n_top, t = i - b * n_top;
  int out = -1;
  if (top[i] > 0.5f) {
    const int o0 = bottom_off[t], nk = bottom_off[t + 1] - o0, hr = head_row[t];
    if (hr < 0) out = bottom_ids[o0];
    else {
      const float* s = bott + (int64_t)b * (R - n_top) + (hr - n_top);
      int am = 0;
      float best = s[0];
      for (int j = 1; j < nk; ++j)
        if (s[j] > best) { best = s[j]; am = j; }   // first maximum, as numpy argmax
      const int bi = bottom_ids[o0 + am];
      out = none_flag[bi] ? -1 : bi;
    }
  }
  pred[i] = out;
}

// one heads call: the arguments the entry points share, the soft term's mode and its arguments
struct HeadsCall {
  const void* hidden; int64_t cls_stride; const float *Wh, *bh; const nbest_label_space* ls; const float* labels;
  float *top, *bott, *final_scores, *loss_parts, *dcls, *dWh, *dbh;
  int B, H, dtype, need_grad, accumulate; float drop_p; uint64_t seed; uint32_t drop_stream;
  void* ws; size_t ws_bytes; nbest_stream_t stream;
  int mode; KdArgs kd;
};
constexpr decltype(&heads_fwd_kernel<float, kPlain>) kHeadsFwd[2][4] = {   // by [dtype][mode]
    {heads_fwd_kernel<float, kPlain>, heads_fwd_kernel<float, kKd>, heads_fwd_kernel<float, kKdT>, heads_fwd_kernel<float, kRDrop>},
    {heads_fwd_kernel<bf16, kPlain>, heads_fwd_kernel<bf16, kKd>, heads_fwd_kernel<bf16, kKdT>, heads_fwd_kernel<bf16, kRDrop>}};
static_assert(NBEST_F32 == 0 && NBEST_BF16 == 1, "kHeadsFwd is indexed by the dtype code");

// the two launches of nbest_stc_heads / _kd / _kd_t / _rdrop
int heads_launch(const HeadsCall& c) {
  NB_CHECK(c.hidden && c.Wh && c.bh && c.ls && c.labels && c.top && c.bott && c.final_scores && c.loss_parts && c.ws && c.B > 0 && c.H > 0,
           NBEST_ERR_ARG, "stc_heads: null pointer");
  NB_CHECK(!c.need_grad || (c.dcls && c.dWh && c.dbh), NBEST_ERR_ARG, "stc_heads: need_grad without gradient buffers");
  const int B = c.B, H = c.H, R = c.ls->n_rows, n_top = c.ls->n_top, n_bottom = c.ls->n_bottom;
  NB_CHECK(R > n_top && n_top > 0 && n_bottom > 0 && R <= 4096 && H <= 2048, NBEST_ERR_SHAPE, "stc_heads: bad label space");
  const HeadsWs w(B, R, H);
  NB_CHECK(c.ws_bytes >= w.bytes, NBEST_ERR_WORKSPACE, "stc_heads: workspace too small");
  NB_CHECK((int64_t)11 * B * H < ((int64_t)1 << 32), NBEST_ERR_SHAPE, "stc_heads: B*H too large");
  hipStream_t st = (hipStream_t)c.stream;
  float *cls = w.at<float>(c.ws, w.cls), *dz = w.at<float>(c.ws, w.dz), *sloss = w.at<float>(c.ws, w.sloss);
  uint32_t* mw = w.at<uint32_t>(c.ws, w.mw);
  int32_t* lay_row = w.at<int32_t>(c.ws, w.lay_row);
  const DropCfg d = make_drop(c.drop_p, c.seed, c.drop_stream);
  // the CE term averages over the softmax heads: a head's rows are its bottoms, a single-bottom top has none, so n_heads = R - n_bottom
  const int n_heads = R - n_bottom;
  NB_CHECK(n_heads > 0, NBEST_ERR_SHAPE, "stc_heads: label space has no multi-value head");
  const int n_lay = n_heads + 1;
  const size_t smemF = HeadsLds(H, R, n_lay, kFwdThreads / 64, c.mode).bytes();
  NB_CHECK(c.mode != kRDrop || smemF <= (size_t)64 * 1024, NBEST_ERR_SHAPE, "stc_heads_rdrop: %zu bytes of LDS per block exceed 64 KB", smemF);
  NB_CHECK(c.dtype == NBEST_F32 || c.dtype == NBEST_BF16, NBEST_ERR_DTYPE, "stc_heads: bad dtype %d", c.dtype);
  kHeadsFwd[c.dtype][c.mode]<<<B, kFwdThreads, smemF, st>>>(c.hidden, c.cls_stride, c.Wh, c.bh, c.labels, c.ls->bottom_off, c.ls->bottom_ids,
                                                           c.ls->head_row, n_top, n_bottom, R, H, n_heads, n_lay, cls, c.top, c.bott,
                                                           c.final_scores, dz, sloss, mw, lay_row, d, c.kd);
  NB_LAUNCH_CHECK();
  if (c.need_grad) {
    const int nh = (H + 63) / 64;
    const int nW = ((R + kBwdRows - 1) / kBwdRows) * nh, nD = ((B + kBwdRows - 1) / kBwdRows) * nh;
    heads_bwd_kernel<<<nW + nD + 1, 256, 0, st>>>(cls, dz, c.Wh, B, R, H, c.dWh, c.dbh, c.dcls, c.accumulate, mw, lay_row, d, sloss, c.loss_parts, nW);
  } else {
    loss_reduce_kernel<<<1, 256, 0, st>>>(sloss, B, c.loss_parts);
  }
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
}  // namespace

extern "C" size_t nbest_heads_ws_bytes(int B, int R, int H) { return HeadsWs(B, R, H).bytes; }

extern "C" int nbest_stc_heads(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                               const nbest_label_space* ls, const float* labels, float* top, float* bott,
                               float* final_scores, float* loss_parts, float* dcls, float* dWh, float* dbh, int B, int H,
                               int dtype, int need_grad, int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream,
                               void* ws, size_t ws_bytes, nbest_stream_t stream) {
  return heads_launch({hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype, need_grad,
                       accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, kPlain, {}});
}

// Knowledge distillation: nbest_stc_heads with a teacher's probabilities as a second set of targets (kKd).
extern "C" int nbest_stc_heads_kd(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                                  const nbest_label_space* ls, const float* labels, const float* t_top, const float* t_bott,
                                  const float* t_final, float alpha, float* top, float* bott, float* final_scores,
                                  float* loss_parts, float* dcls, float* dWh, float* dbh, int B, int H, int dtype, int need_grad,
                                  int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes,
                                  nbest_stream_t stream) {
  NB_CHECK(alpha >= 0.f && alpha <= 1.f, NBEST_ERR_ARG, "stc_heads_kd: alpha %g outside [0, 1]", (double)alpha);
  NB_CHECK(alpha == 0.f || (t_top && t_bott && t_final), NBEST_ERR_ARG, "stc_heads_kd: null teacher pointer with alpha != 0");
  NB_CHECK((t_top && t_bott && t_final) || !(t_top || t_bott || t_final), NBEST_ERR_ARG,
           "stc_heads_kd: pass all three teacher arrays or none");
  // alpha = 0 without a teacher: nothing soft to compute, the plain kernel (loss_parts[3] = 0)
  return heads_launch({hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype, need_grad,
                       accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, t_top ? kKd : kPlain,
                       {t_top, t_bott, t_final, alpha, 0.f}});
}

// Distillation at a temperature: the teacher's LOGITS as the second set of targets, both models softened by 1 / T (kKdT).
extern "C" int nbest_stc_heads_kd_t(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                                    const nbest_label_space* ls, const float* labels, const float* t_logits, float alpha,
                                    float temperature, float* top, float* bott, float* final_scores, float* loss_parts, float* dcls,
                                    float* dWh, float* dbh, int B, int H, int dtype, int need_grad, int accumulate, float drop_p,
                                    uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(alpha >= 0.f && alpha <= 1.f, NBEST_ERR_ARG, "stc_heads_kd_t: alpha %g outside [0, 1]", (double)alpha);
  NB_CHECK(temperature > 0.f && temperature < INFINITY, NBEST_ERR_ARG, "stc_heads_kd_t: temperature %g must be finite and > 0",
           (double)temperature);
  NB_CHECK(alpha == 0.f || t_logits, NBEST_ERR_ARG, "stc_heads_kd_t: null teacher logits with alpha != 0");
  // alpha = 0 without a teacher: nothing soft to compute, the plain kernel (loss_parts[3] = 0)
  return heads_launch({hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype, need_grad,
                       accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, t_logits ? kKdT : kPlain,
                       {t_logits, nullptr, nullptr, alpha, temperature}});
}

// R-Drop: rows b and b + B2 / 2 are twins; the symmetric KL between their outputs enters the loss with weight alpha (kRDrop).
extern "C" int nbest_stc_heads_rdrop(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                                     const nbest_label_space* ls, const float* labels, float alpha, float* top, float* bott,
                                     float* final_scores, float* loss_parts, float* dcls, float* dWh, float* dbh, int B2, int H,
                                     int dtype, int need_grad, int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream,
                                     void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(alpha >= 0.f && alpha < INFINITY, NBEST_ERR_ARG, "stc_heads_rdrop: alpha %g must be finite and >= 0", (double)alpha);
  NB_CHECK(B2 > 0 && (B2 & 1) == 0, NBEST_ERR_SHAPE, "stc_heads_rdrop: B2 = %d must be even (rows b and b + B2 / 2 are twins)", B2);
  return heads_launch({hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B2, H, dtype, need_grad,
                       accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, kRDrop, {nullptr, nullptr, nullptr, alpha, 0.f}});
}

namespace {
// The logits stage of heads_fwd_kernel on its own, dropout off: wave_logit's arithmetic in its order, + bh[r] - the numbers its scores
// are made from.  The loop stays its own: through wave_logit itself this call measured 0.3 us (1.5 %) slower.
constexpr int kLogitsThreads = 512;
template <typename T>
__global__ __launch_bounds__(kLogitsThreads) void heads_logits_kernel(const T* __restrict__ hidden, int64_t cls_stride,
                                                                       const float* __restrict__ Wh, const float* __restrict__ bh, int R,
                                                                       int H, float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [H]
  const int b = blockIdx.x;
  const T* x = hidden + (int64_t)b * cls_stride;
  for (int h = threadIdx.x; h < H; h += blockDim.x) xs[h] = to_f<T>(x[h]);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  __syncthreads();
  for (int r = wave; r < R; r += nw) {
    const float* w = Wh + (int64_t)r * H;
    float s = 0.f;
#pragma unroll 4
    for (int h = lane; h < H; h += 64) s = fmaf(w[h], xs[h], s);
    s = wave_sum(s);
    if (lane == 0) logits[(int64_t)b * R + r] = s + bh[r];
  }
}
}  // namespace

extern "C" int nbest_stc_heads_logits(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                                      const nbest_label_space* ls, float* logits, int B, int H, int dtype, nbest_stream_t stream) {
  NB_CHECK(hidden && Wh && bh && ls && logits && B > 0 && H > 0, NBEST_ERR_ARG, "stc_heads_logits: null pointer");
  NB_CHECK(dtype == NBEST_F32 || dtype == NBEST_BF16, NBEST_ERR_DTYPE, "stc_heads_logits: bad dtype %d", dtype);
  const int R = ls->n_rows, n_top = ls->n_top;
  NB_CHECK(R > n_top && n_top > 0 && R <= 4096 && H <= 2048, NBEST_ERR_SHAPE, "stc_heads_logits: bad label space");
  hipStream_t st = (hipStream_t)stream;
  const size_t smem = (size_t)H * sizeof(float);
  if (dtype == NBEST_F32)
    heads_logits_kernel<float><<<B, kLogitsThreads, smem, st>>>((const float*)hidden, cls_stride, Wh, bh, R, H, logits);
  else
    heads_logits_kernel<bf16><<<B, kLogitsThreads, smem, st>>>((const bf16*)hidden, cls_stride, Wh, bh, R, H, logits);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

// Backward of the heads for arbitrary upstream gradients (autograd bridge; hipabi.stc_heads_vjp): `ws` is the workspace a
// nbest_stc_heads call with the same (hidden, Wh, dropout seed) just used - it still holds the fp32 CLS rows, the layers' dropout bits
// and the row -> layer table.  dcls [B][H] is overwritten; dWh / dbh are overwritten unless accumulate.
extern "C" int nbest_stc_heads_vjp(const float* Wh, const nbest_label_space* ls, const float* top, const float* bott, const float* dtop,
                                   const float* dbott, const float* dfin, float* dcls, float* dWh, float* dbh, int B, int H, int accumulate,
                                   float drop_p, uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(Wh && ls && top && bott && dtop && dbott && dfin && dcls && dWh && dbh && ws && B > 0 && H > 0, NBEST_ERR_ARG, "stc_heads_vjp: null pointer");
  const int R = ls->n_rows, n_top = ls->n_top, n_bottom = ls->n_bottom;
  const HeadsWs w(B, R, H);
  NB_CHECK(ws_bytes >= w.bytes, NBEST_ERR_WORKSPACE, "stc_heads_vjp: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float *cls = w.at<float>(ws, w.cls), *dz = w.at<float>(ws, w.dz);
  uint32_t* mw = w.at<uint32_t>(ws, w.mw);
  int32_t* lay_row = w.at<int32_t>(ws, w.lay_row);
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  heads_vjp_dz_kernel<<<B, 256, 0, st>>>(top, bott, dtop, dbott, dfin, ls->bottom_off, ls->bottom_ids, ls->head_row, n_top, n_bottom, R, dz);
  NB_LAUNCH_CHECK();
  const int nh = (H + 63) / 64;
  const int nW = ((R + kBwdRows - 1) / kBwdRows) * nh, nD = ((B + kBwdRows - 1) / kBwdRows) * nh;
  heads_bwd_kernel<<<nW + nD, 256, 0, st>>>(cls, dz, Wh, B, R, H, dWh, dbh, dcls, accumulate, mw, lay_row, d, nullptr, nullptr, nW);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_cls_mse(const void* hidden_a, int64_t stride_a, const void* hidden_t, int64_t stride_t, float* loss,
                             float* da, float* dt, int B, int H, int dtype, float grad_scale, nbest_stream_t stream) {
  NB_CHECK(hidden_a && hidden_t && loss && B > 0 && H > 0, NBEST_ERR_ARG, "cls_mse: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == NBEST_F32)
    cls_mse_kernel<float><<<1, 256, 0, st>>>((const float*)hidden_a, stride_a, (const float*)hidden_t, stride_t, loss, da, dt, B, H, grad_scale);
  else if (dtype == NBEST_BF16)
    cls_mse_kernel<bf16><<<1, 256, 0, st>>>((const bf16*)hidden_a, stride_a, (const bf16*)hidden_t, stride_t, loss, da, dt, B, H, grad_scale);
  else NB_CHECK(false, NBEST_ERR_DTYPE, "cls_mse: bad dtype %d", dtype);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

namespace {
__global__ void stamp_kernel(int32_t* flag, int32_t value) {
  __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace

extern "C" int nbest_stream_stamp(int32_t* flag, int32_t value, nbest_stream_t stream) {
  NB_CHECK(flag, NBEST_ERR_ARG, "stream_stamp: null pointer");
  stamp_kernel<<<1, 1, 0, (hipStream_t)stream>>>(flag, value);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}

extern "C" int nbest_stc_decode(const float* top, const float* bott, const nbest_label_space* ls, const uint8_t* none_flag,
                                int32_t* pred, int B, nbest_stream_t stream) {
  NB_CHECK(top && bott && ls && none_flag && pred && B > 0, NBEST_ERR_ARG, "stc_decode: null pointer");
  const int n = B * ls->n_top;
  decode_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(top, bott, ls->bottom_off, ls->bottom_ids, ls->head_row,
                                                                 none_flag, ls->n_top, ls->n_rows, pred, B);
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
