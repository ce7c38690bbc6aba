// K7 STC heads + losses (forward and analytic backward), K8 CLS-MSE, K10 decode.
//
// Shapes are tiny (B x 171 x 768 for bert-base on DSTC2), so everything is fp32 VALU work in two launches
// (heads_fwd_kernel, heads_bwd_kernel); the point is to replace ~40 tiny launches + 4 host syncs of the reference
// (/root/reference/models/modules/hierarchical_classifier.py:35-60, /root/reference/n_best_asr_bert.py:160-195) and to hand
// dCLS to the encoder backward.
//
// Workspace layout (floats): cls[B][H] | logits[B][R] | dz[B][R] | sample_loss[B][4]
#include "common.h"

namespace {

__device__ __forceinline__ int layer_of_row(int r, const int32_t* __restrict__ head_row, int n_top, int* lay_cache) {
  (void)lay_cache;
  if (r < n_top) return 0;
  // heads are laid out in increasing top order: find the top t with head_row[t] <= r < next head's start
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

__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ sample_loss, int B, float* __restrict__ out) {
  __shared__ float sm[16];
  for (int k = 0; k < 4; ++k) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) s += sample_loss[4 * b + k];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) out[k] = s;
  }
}

// ---- round 4: the heads as TWO launches (147 us in four launches for a 256 x 768 x 171 problem) ------------------
// heads_fwd_kernel: one block per sample does what heads_logits_kernel + heads_scores_kernel did - CLS row and the layers' dropout bits
// into LDS, the 171 logits (a wave per row), then scores / losses / d(loss)/d(logits) with the TOP labels spread over the waves (the
// old scores kernel walked the 30 tops one after the other in a single wave: 37 us of dependent exp / log / shuffle latency).
// heads_bwd_kernel: weight gradient and input gradient in one grid (blocks [0, nW): an 8-row x 64-column tile of dWh, waves split the
// batch, the CLS column chunk loaded once per sample for all 8 rows; blocks [nW, nW + nD): 8 samples x 64 columns of dCLS, waves split
// the head rows, the weight element loaded once for all 8 samples); the last block sums the per-sample losses.  Fixed-order sums.
//
// KD (nbest_stc_heads_kd, knowledge distillation): the same kernel with a second set of targets - a teacher's fp32 probabilities
// t_top / t_bott / t_fin in the layout of top / bott / final.  The soft loss is the three terms with the teacher's outputs in
// place of the labels: the targets of the two BCEs, and the teacher's distribution over a head's columns where the hard term has
// the one-hot class.  Its sum goes to sample_loss[4 b + 3]; d(logits) = (1 - alpha) d_hard + alpha d_soft (dz is linear in the
// upstream gradient, so the two are blended per logit).  Every hard statement is the plain instantiation's; the soft ones sit
// under `if constexpr (KD)`, so the plain instantiation computes what it always did.
//
// KD_T (nbest_stc_heads_kd_t, distillation at a temperature): the teacher comes as its LOGITS t_logits [B][R]; its row is staged in LDS
// next to the student's.  Both rows are softened by 1 / T and the soft statements of KD run on the tempered scores p_T = sigmoid(z_t / T),
// s_T = softmax(z / T), f_T = p_T s_T of the two models; loss = T^2 x that, d(logits) = T x that (T^2 of the loss x 1 / T of du / dz).
// The teacher's per-head max and the two tempered sums ride in the student's passes over the columns (independent shuffle chains:
// the kernel is latency-bound); the student's tempered max is max(z) / T.  Hard statements, scores and dropout bits as plain.
//
// RDROP (nbest_stc_heads_rdrop, R-Drop): rows b and b + B / 2 of the batch are twins (one utterance under two sets of dropout bits).  The
// block of row b also stages its twin's CLS row and the twin's mask words of the n_lay layers, and forms the twin's R logits in the logits
// loop with its own arithmetic in its own order (the twin's block computes the same bits for them); they sit where KD_T keeps the
// teacher's row.  The pair's consistency term is the symmetric KL of the model's factorisation, in its logarithm-free form
//   R = sum_t 1/2 (p_t - p'_t)(z_t - z'_t) + (1 / n_heads) sum_k 1/2 sum_j (s_kj - s'_kj)(z_kj - z'_kj)
// (no term on final); each block of a pair writes R / 2 into sample_loss[4 b + 3] and dz = dz_hard + alpha dR/dz(own row).  The twin's max and
// exp-sum ride in the row's own passes, as KD_T's teacher.  The differences of scores are formed under fp contract(off): equal twins give
// dR/dz = 0 exactly, alpha = 0 the plain kernel's bits.
enum { kPlain = 0, kKd = 1, kKdT = 2, kRDrop = 3 };
struct KdArgs {
  const float* t_top;   // [B][n_top]        (kKdT: t_logits [B][R])
  const float* t_bott;  // [B][R - n_top]
  const float* t_fin;   // [B][n_bottom]
  float alpha;
  float temperature;    // kKdT only
};

// a - b that never fuses with a product feeding it (the device default contracts a * b - c into an fma; e * inv - e * inv must be 0)
__device__ __forceinline__ float sub_exact(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__device__ __forceinline__ float bce_term(float p, float y) {
  return -(y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(logf(1.f - p), -100.f));
}

constexpr int kFwdThreads = 512;
template <typename T, int MODE>
__global__ __launch_bounds__(kFwdThreads) void heads_fwd_kernel(const T* __restrict__ hidden, int64_t cls_stride, const float* __restrict__ Wh,
                                                                 const float* __restrict__ bh, const float* __restrict__ labels,
                                                                 const int32_t* __restrict__ bottom_off, const int32_t* __restrict__ bottom_ids,
                                                                 const int32_t* __restrict__ head_row, int n_top, int n_bottom, int R, int H,
                                                                 int n_heads, int n_lay, float* __restrict__ cls_out, float* __restrict__ top,
                                                                 float* __restrict__ bott, float* __restrict__ fin, float* __restrict__ dz,
                                                                 float* __restrict__ sample_loss, uint32_t* __restrict__ mw,
                                                                 int32_t* __restrict__ lay_row, DropCfg drop, KdArgs kd) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [H] | logits [R] | layer of row [R] | mask words [n_lay][W] | loss partials [waves][3] (KD: | soft [waves]) (KD_T: | teacher logits [R]) (RDROP: | twin logits [R] | twin CLS [H] | twin mask words [n_lay][W])
  constexpr bool KD = MODE == kKd, KDT = MODE == kKdT, RD = MODE == kRDrop;
  const int b = blockIdx.x, B = gridDim.x, W = (H + 31) >> 5;
  float* zs = xs + H;
  int32_t* lay_s = (int32_t*)(zs + R);
  uint32_t* mk = (uint32_t*)(lay_s + R);
  float* lsum = (float*)(mk + n_lay * W);
  const T* x = hidden + (int64_t)b * cls_stride;
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    const float v = to_f<T>(x[h]);
    xs[h] = v;
    cls_out[(int64_t)b * H + h] = v;
  }
  float* tzs = lsum + 4 * (blockDim.x >> 6);               // KD_T: the teacher's row of logits
  if constexpr (KDT)
    for (int r = threadIdx.x; r < R; r += blockDim.x) tzs[r] = kd.t_top[(int64_t)b * R + r];
  float* xt = tzs + R;                                      // RDROP: the twin's CLS row and mask words
  uint32_t* mkt = (uint32_t*)(xt + H);
  if constexpr (RD) {
    const int bt = b < (B >> 1) ? b + (B >> 1) : b - (B >> 1);
    const T* x2 = hidden + (int64_t)bt * cls_stride;
    for (int h = threadIdx.x; h < H; h += blockDim.x) xt[h] = to_f<T>(x2[h]);
    if (drop.thr16)
      for (int lay = 0; lay < n_lay; ++lay) heads_mask_words(drop, lay, bt, B, H, W, mkt + lay * W, nullptr);
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const int l = layer_of_row(r, head_row, n_top, nullptr);
    lay_s[r] = l;
    if (b == 0) lay_row[r] = l;
  }
  if (drop.thr16)
    for (int lay = 0; lay < n_lay; ++lay) heads_mask_words(drop, lay, b, B, H, W, mk + lay * W, mw + ((int64_t)lay * B + b) * W);
  __syncthreads();
  for (int r = wave; r < R; r += nw) {
    const float* w = Wh + (int64_t)r * H;
    const uint32_t* mrow = mk + lay_s[r] * W;
    float s = 0.f;
    if constexpr (RD) {                                     // the twin's logit next to the row's own: one read of the weights
      const uint32_t* mrow2 = mkt + lay_s[r] * W;
      float s2 = 0.f;
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
        zs[r] = s + bh[r];
        tzs[r] = s2 + bh[r];
      }
      continue;
    }
#pragma unroll 4
    for (int h = lane; h < H; h += 64) {
      float xv = xs[h];
      if (drop.thr16) xv = ((mrow[h >> 5] >> (h & 31)) & 1u) ? xv * drop.scale : 0.f;
      s = fmaf(w[h], xv, s);
    }
    s = wave_sum(s);
    if (lane == 0) zs[r] = s + bh[r];
  }
  __syncthreads();
  const float* z = zs;
  const float* y = labels + (int64_t)b * n_bottom;
  float l_bot = 0.f, l_top = 0.f, l_ce = 0.f;
  float l_soft = 0.f;                                       // KD: every lane's own share of the three soft terms
  const float* tfin = KD ? kd.t_fin + (int64_t)b * n_bottom : nullptr;
  const float* tbot = KD ? kd.t_bott + (int64_t)b * (R - n_top) : nullptr;
  const float wh = 1.f - kd.alpha, wsft = kd.alpha;
  const float invT = KDT ? 1.0f / kd.temperature : 1.f;     // KD_T: u = z / T of both models
  const float wsT = KDT ? kd.alpha * kd.temperature : 0.f;  // KD_T: alpha x T, the weight of d(soft / T^2) / du in dz
  for (int t = wave; t < n_top; t += nw) {                  // a wave per top label (lanes parallelise the head columns)
    const int o0 = bottom_off[t], nk = bottom_off[t + 1] - o0, hr = head_row[t];
    const float zt = z[t];
    const float pt = 1.0f / (1.0f + __expf(-zt));
    float dpt = 0.f;  // d(loss)/d(top score)
    float ytop = 0.f;
    float dpt_s = 0.f;  // KD: d(soft loss)/d(top score)
    float ptT = 0.f, qT = 0.f;                              // KD_T: the tempered top scores of the student and the teacher
    if constexpr (KDT) {
      ptT = 1.0f / (1.0f + __expf(-zt * invT));
      qT = 1.0f / (1.0f + __expf(-tzs[t] * invT));
    }
    float ptw = 0.f, dzt = 0.f;                             // RDROP: the twin's top score, z_t - z'_t
    if constexpr (RD) {
      ptw = 1.0f / (1.0f + __expf(-tzs[t]));
      dzt = zt - tzs[t];
    }
    if (hr < 0) {
      const int bi = bottom_ids[o0];                        // single bottom label: final = top score
      const float yy = y[bi];
      ytop = yy;
      if (lane == 0) {
        fin[(int64_t)b * n_bottom + bi] = pt;
        l_bot += -(yy * fmaxf(logf(pt), -100.f) + (1.f - yy) * fmaxf(logf(1.f - pt), -100.f));
      }
      dpt += (pt - yy) / fmaxf(pt * (1.f - pt), 1e-12f);
      if constexpr (KD) {
        const float tf = tfin[bi];
        if (lane == 0) l_soft += bce_term(pt, tf);
        dpt_s += (pt - tf) / fmaxf(pt * (1.f - pt), 1e-12f);
      }
      if constexpr (KDT) {                                  // final = top score, of both models
        if (lane == 0) l_soft += bce_term(ptT, qT);
        dpt_s += (ptT - qT) / fmaxf(ptT * (1.f - ptT), 1e-12f);
      }
    } else {
      float mx = -INFINITY;                                 // softmax head over nk columns (nk may exceed 64: strided)
      float tmx = -INFINITY;                                // KD_T: the teacher's max, in the same pass
      for (int j = lane; j < nk; j += 64) {
        mx = fmaxf(mx, z[hr + j]);
        if constexpr (KDT || RD) tmx = fmaxf(tmx, tzs[hr + j]);
      }
      mx = wave_max(mx);
      if constexpr (KDT || RD) tmx = wave_max(tmx);
      float se = 0.f;
      float seT = 0.f, teT = 0.f;                           // KD_T: sums of exp((z - max) / T), student and teacher (max(z / T) = max(z) / T)
      for (int j = lane; j < nk; j += 64) {
        se += __expf(z[hr + j] - mx);
        if constexpr (KDT) {
          seT += __expf((z[hr + j] - mx) * invT);
          teT += __expf((tzs[hr + j] - tmx) * invT);
        }
        if constexpr (RD) teT += __expf(tzs[hr + j] - tmx);  // RDROP: the twin's sum, in the row's own order
      }
      se = wave_sum(se);
      if constexpr (KDT) wave_sum2(seT, teT);
      if constexpr (RD) teT = wave_sum(teT);
      const float inv = 1.0f / se;
      const float invsT = KDT ? 1.0f / seT : 0.f, invtT = (KDT || RD) ? 1.0f / teT : 0.f;
      const float wr = 0.5f / (float)n_heads;               // RDROP: the weight of a head's term
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
      for (int j = lane; j < nk; j += 64) {
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
        if constexpr (KD) {
          const float tf = tfin[bi], tb = tbot[(hr - n_top) + j];
          l_soft += bce_term(f, tf);
          const float gs = (f - tf) / fmaxf(f * (1.f - f), 1e-12f);
          const float dss = gs * pt - tb / ((s + 1e-12f) * (float)n_heads);
          dot_s += dss * s;
          dtop_s += gs * s;
        }
        if constexpr (KDT) {                                // the KD statements on the tempered scores
          const float sT = __expf((z[hr + j] - mx) * invT) * invsT, tb = __expf((tzs[hr + j] - tmx) * invT) * invtT;
          const float fT = ptT * sT, tf = qT * tb;
          l_soft += bce_term(fT, tf);
          const float gs = (fT - tf) / fmaxf(fT * (1.f - fT), 1e-12f);
          const float dss = gs * ptT - tb / ((sT + 1e-12f) * (float)n_heads);
          dot_s += dss * sT;
          dtop_s += gs * sT;
        }
        if constexpr (RD) {                                 // 1/2 (s - s')(z - z') and sum_j s_j (z_j - z'_j)
          const float sw = __expf(tzs[hr + j] - tmx) * invtT, dzz = z[hr + j] - tzs[hr + j];
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
      for (int j = lane; j < nk; j += 64) {
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
        if constexpr (KD) {
          const float tf = tfin[bi], tb = tbot[(hr - n_top) + j];
          const float gs = (f - tf) / fmaxf(f * (1.f - f), 1e-12f);
          const float dss = gs * pt - tb / ((s + 1e-12f) * (float)n_heads);
          l_soft += -tb * logf(s + 1e-12f) / (float)n_heads;
          // alpha = 0 gives the plain kernel's bits because the soft term is finite (|gs|, tb / (s + 1e-12) <= 1e12): 1 * x + 0 * y = x
          dz[(int64_t)b * R + hr + j] = wh * (s * (ds - dot)) + wsft * (s * (dss - dot_s));
        } else if constexpr (KDT) {
          const float sT = __expf((z[hr + j] - mx) * invT) * invsT, tb = __expf((tzs[hr + j] - tmx) * invT) * invtT;
          const float fT = ptT * sT, tf = qT * tb;
          const float gs = (fT - tf) / fmaxf(fT * (1.f - fT), 1e-12f);
          const float dss = gs * ptT - tb / ((sT + 1e-12f) * (float)n_heads);
          l_soft += -tb * logf(sT + 1e-12f) / (float)n_heads;
          // alpha = 0 gives the plain kernel's bits: the soft term is finite, as in KD
          dz[(int64_t)b * R + hr + j] = wh * (s * (ds - dot)) + wsT * (sT * (dss - dot_s));
        } else if constexpr (RD) {
          const float sw = __expf(tzs[hr + j] - tmx) * invtT, dzz = z[hr + j] - tzs[hr + j];
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
    if constexpr (KD) {
      const float tt = kd.t_top[(int64_t)b * n_top + t];
      if (lane == 0) l_soft += bce_term(pt, tt);
      dpt_s += (pt - tt) / fmaxf(pt * (1.f - pt), 1e-12f);
    }
    if constexpr (KDT) {
      if (lane == 0) l_soft += bce_term(ptT, qT);
      dpt_s += (ptT - qT) / fmaxf(ptT * (1.f - ptT), 1e-12f);
    }
    if constexpr (RD)
      if (lane == 0) l_soft += 0.5f * ((pt - ptw) * dzt);
    if (lane == 0) {
      top[(int64_t)b * n_top + t] = pt;
      if constexpr (KD) dz[(int64_t)b * R + t] = wh * (dpt * pt * (1.f - pt)) + wsft * (dpt_s * pt * (1.f - pt));
      else if constexpr (KDT) dz[(int64_t)b * R + t] = wh * (dpt * pt * (1.f - pt)) + wsT * (dpt_s * ptT * (1.f - ptT));
      else if constexpr (RD) dz[(int64_t)b * R + t] = dpt * pt * (1.f - pt) + kd.alpha * (0.5f * (pt * (1.f - pt) * dzt + (pt - ptw)));
      else dz[(int64_t)b * R + t] = dpt * pt * (1.f - pt);
    }
  }
  l_ce = wave_sum(l_ce);
  if (lane == 0) { lsum[3 * wave] = l_bot; lsum[3 * wave + 1] = l_top; lsum[3 * wave + 2] = l_ce; }
  if constexpr (KD || KDT || RD) {
    l_soft = wave_sum(l_soft);
    if (lane == 0) lsum[3 * nw + wave] = l_soft;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float v = 0.f;
    for (int w = 0; w < nw; ++w) v += lsum[3 * w + threadIdx.x];     // wave order: the same sum on every run
    sample_loss[4 * b + threadIdx.x] = v;
  }
  if (threadIdx.x == 3) {
    float v = 0.f;
    if constexpr (KD || KDT || RD)
      for (int w = 0; w < nw; ++w) v += lsum[3 * nw + w];
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
  if (!loss_out) return;
  __shared__ float sm[16];
  for (int k = 0; k < 4; ++k) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) s += sample_loss[4 * b + k];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) loss_out[k] = s;
  }
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

}  // namespace

extern "C" size_t nbest_heads_ws_bytes(int B, int R, int H) {
  // cls | logits | dz | per-sample losses | dropout mask bits of at most R + 1 classifier layers
  return ((size_t)B * H + (size_t)2 * B * R + (size_t)4 * B) * sizeof(float) + (size_t)(R + 1) * B * ((H + 31) / 32) * sizeof(uint32_t) + (size_t)R * sizeof(int32_t);
}

namespace {
// the two launches of nbest_stc_heads / nbest_stc_heads_kd / nbest_stc_heads_kd_t (kd: the teacher's arrays and alpha, or nullptr for
// the plain kernel; kd->temperature > 0 selects the logits form, whose t_top is t_logits [B][R]; rdrop: kd carries alpha alone and rows
// b / b + B / 2 are twins)
int heads_launch(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh, const nbest_label_space* ls,
                 const float* labels, float* top, float* bott, float* final_scores, float* loss_parts, float* dcls, float* dWh,
                 float* dbh, int B, int H, int dtype, int need_grad, int accumulate, float drop_p, uint64_t seed,
                 uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream, const KdArgs* kd, bool rdrop = false) {
  NB_CHECK(hidden && Wh && bh && ls && labels && top && bott && final_scores && loss_parts && ws && B > 0 && H > 0,
           NBEST_ERR_ARG, "stc_heads: null pointer");
  NB_CHECK(!need_grad || (dcls && dWh && dbh), NBEST_ERR_ARG, "stc_heads: need_grad without gradient buffers");
  const int R = ls->n_rows, n_top = ls->n_top, n_bottom = ls->n_bottom;
  NB_CHECK(R > n_top && n_top > 0 && n_bottom > 0 && R <= 4096 && H <= 2048, NBEST_ERR_SHAPE, "stc_heads: bad label space");
  NB_CHECK(ws_bytes >= nbest_heads_ws_bytes(B, R, H), NBEST_ERR_WORKSPACE, "stc_heads: workspace too small");
  NB_CHECK((int64_t)11 * B * H < ((int64_t)1 << 32), NBEST_ERR_SHAPE, "stc_heads: B*H too large");
  hipStream_t st = (hipStream_t)stream;
  float* cls = (float*)ws;
  float* logits = cls + (size_t)B * H;
  float* dz = logits + (size_t)B * R;
  float* sloss = dz + (size_t)B * R;
  uint32_t* mw = (uint32_t*)(sloss + (size_t)4 * B);
  int32_t* lay_row = (int32_t*)(mw + (size_t)(R + 1) * B * ((H + 31) / 32));
  const DropCfg d = make_drop(drop_p, seed, drop_stream);
  // number of softmax heads = R - n_top rows split over heads; the CE term averages over heads: count on host is not
  // available (device arrays), so it is passed implicitly: n_heads = #tops with head_row >= 0, computed by the caller
  // into ls->n_bottom? -> no: derive it from sizes: sum over multi tops (nk) = R - n_top and singles = n_top - n_heads,
  // n_bottom = (R - n_top) + (n_top - n_heads)  =>  n_heads = R - n_bottom.
  const int n_heads = R - n_bottom;
  NB_CHECK(n_heads > 0, NBEST_ERR_SHAPE, "stc_heads: label space has no multi-value head");
  const int n_lay = n_heads + 1;
  const int mode = !kd ? kPlain : rdrop ? kRDrop : kd->temperature > 0.f ? kKdT : kKd;
  // kKdT: the soft partials as kKd, then the teacher's row of R logits (heads_fwd_kernel finds it at lsum + 4 floats per wave)
  const size_t smemF = ((size_t)H + 2 * (size_t)R) * sizeof(float) + (size_t)n_lay * ((H + 31) / 32) * sizeof(uint32_t) + (size_t)(kd ? 4 : 3) * (kFwdThreads / 64) * sizeof(float) +
                       (mode == kKdT ? (size_t)R * sizeof(float) : 0) +
                       // kRDrop: the twin's logits where kKdT keeps the teacher's, then the twin's CLS row and its mask words
                       (mode == kRDrop ? ((size_t)R + H) * sizeof(float) + (size_t)n_lay * ((H + 31) / 32) * sizeof(uint32_t) : 0);
  NB_CHECK(mode != kRDrop || smemF <= (size_t)64 * 1024, NBEST_ERR_SHAPE, "stc_heads_rdrop: %zu bytes of LDS per block exceed 64 KB", smemF);
  const KdArgs ka = kd ? *kd : KdArgs{nullptr, nullptr, nullptr, 0.f, 0.f};
#define NB_HEADS_FWD(TT, KD)                                                                                                          \
  heads_fwd_kernel<TT, KD><<<B, kFwdThreads, smemF, st>>>((const TT*)hidden, cls_stride, Wh, bh, labels, ls->bottom_off, ls->bottom_ids,  \
                                                          ls->head_row, n_top, n_bottom, R, H, n_heads, n_lay, cls, top, bott,            \
                                                          final_scores, dz, sloss, mw, lay_row, d, ka)
  if (dtype == NBEST_F32) {
    if (mode == kRDrop) NB_HEADS_FWD(float, kRDrop); else if (mode == kKdT) NB_HEADS_FWD(float, kKdT); else if (mode == kKd) NB_HEADS_FWD(float, kKd); else NB_HEADS_FWD(float, kPlain);
  } else if (dtype == NBEST_BF16) {
    if (mode == kRDrop) NB_HEADS_FWD(bf16, kRDrop); else if (mode == kKdT) NB_HEADS_FWD(bf16, kKdT); else if (mode == kKd) NB_HEADS_FWD(bf16, kKd); else NB_HEADS_FWD(bf16, kPlain);
  }
  else NB_CHECK(false, NBEST_ERR_DTYPE, "stc_heads: bad dtype %d", dtype);
#undef NB_HEADS_FWD
  NB_LAUNCH_CHECK();
  (void)logits;
  if (need_grad) {
    const int nh = (H + 63) / 64;
    const int nW = ((R + kBwdRows - 1) / kBwdRows) * nh, nD = ((B + kBwdRows - 1) / kBwdRows) * nh;
    heads_bwd_kernel<<<nW + nD + 1, 256, 0, st>>>(cls, dz, Wh, B, R, H, dWh, dbh, dcls, accumulate, mw, lay_row, d, sloss, loss_parts, nW);
  } else {
    loss_reduce_kernel<<<1, 256, 0, st>>>(sloss, B, loss_parts);
  }
  NB_LAUNCH_CHECK();
  return NBEST_OK;
}
}  // namespace

extern "C" int nbest_stc_heads(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                               const nbest_label_space* ls, const float* labels, float* top, float* bott,
                               float* final_scores, float* loss_parts, float* dcls, float* dWh, float* dbh, int B, int H,
                               int dtype, int need_grad, int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream,
                               void* ws, size_t ws_bytes, nbest_stream_t stream) {
  return heads_launch(hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype,
                      need_grad, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, nullptr);
}

// Knowledge distillation: nbest_stc_heads with a teacher's probabilities as a second set of targets (heads_fwd_kernel<T, true>).
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
  if (!t_top)       // alpha = 0 without a teacher: nothing soft to compute, the plain kernel (loss_parts[3] = 0)
    return heads_launch(hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype,
                        need_grad, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, nullptr);
  const KdArgs kd{t_top, t_bott, t_final, alpha, 0.f};
  return heads_launch(hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype,
                      need_grad, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, &kd);
}

// Distillation at a temperature: the teacher's LOGITS as the second set of targets, both models softened by 1 / T (heads_fwd_kernel<T, kKdT>).
extern "C" int nbest_stc_heads_kd_t(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                                    const nbest_label_space* ls, const float* labels, const float* t_logits, float alpha,
                                    float temperature, float* top, float* bott, float* final_scores, float* loss_parts, float* dcls,
                                    float* dWh, float* dbh, int B, int H, int dtype, int need_grad, int accumulate, float drop_p,
                                    uint64_t seed, uint32_t drop_stream, void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(alpha >= 0.f && alpha <= 1.f, NBEST_ERR_ARG, "stc_heads_kd_t: alpha %g outside [0, 1]", (double)alpha);
  NB_CHECK(temperature > 0.f && temperature < INFINITY, NBEST_ERR_ARG, "stc_heads_kd_t: temperature %g must be finite and > 0",
           (double)temperature);
  NB_CHECK(alpha == 0.f || t_logits, NBEST_ERR_ARG, "stc_heads_kd_t: null teacher logits with alpha != 0");
  if (!t_logits)    // alpha = 0 without a teacher: nothing soft to compute, the plain kernel (loss_parts[3] = 0)
    return heads_launch(hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype,
                        need_grad, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, nullptr);
  const KdArgs kd{t_logits, nullptr, nullptr, alpha, temperature};
  return heads_launch(hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B, H, dtype,
                      need_grad, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, &kd);
}

// R-Drop: rows b and b + B2 / 2 are twins; the symmetric KL between their outputs enters the loss with weight alpha (heads_fwd_kernel<T, kRDrop>).
extern "C" int nbest_stc_heads_rdrop(const void* hidden, int64_t cls_stride, const float* Wh, const float* bh,
                                     const nbest_label_space* ls, const float* labels, float alpha, float* top, float* bott,
                                     float* final_scores, float* loss_parts, float* dcls, float* dWh, float* dbh, int B2, int H,
                                     int dtype, int need_grad, int accumulate, float drop_p, uint64_t seed, uint32_t drop_stream,
                                     void* ws, size_t ws_bytes, nbest_stream_t stream) {
  NB_CHECK(alpha >= 0.f && alpha < INFINITY, NBEST_ERR_ARG, "stc_heads_rdrop: alpha %g must be finite and >= 0", (double)alpha);
  NB_CHECK(B2 > 0 && (B2 & 1) == 0, NBEST_ERR_SHAPE, "stc_heads_rdrop: B2 = %d must be even (rows b and b + B2 / 2 are twins)", B2);
  const KdArgs kd{nullptr, nullptr, nullptr, alpha, 0.f};
  return heads_launch(hidden, cls_stride, Wh, bh, ls, labels, top, bott, final_scores, loss_parts, dcls, dWh, dbh, B2, H, dtype,
                      need_grad, accumulate, drop_p, seed, drop_stream, ws, ws_bytes, stream, &kd, true);
}

namespace {
// The logits stage of heads_fwd_kernel on its own, dropout off: one block per sample, the CLS row in LDS, a wave per head row, lanes
// strided over h, fmaf, wave_sum, + bh[r] - the same arithmetic in the same order, so these are the numbers its scores are made from.
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
  NB_CHECK(ws_bytes >= nbest_heads_ws_bytes(B, R, H), NBEST_ERR_WORKSPACE, "stc_heads_vjp: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* cls = (float*)ws;
  float* dz = cls + (size_t)B * H + (size_t)B * R;
  float* sloss = dz + (size_t)B * R;
  uint32_t* mw = (uint32_t*)(sloss + (size_t)4 * B);
  int32_t* lay_row = (int32_t*)(mw + (size_t)(R + 1) * B * ((H + 31) / 32));
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
