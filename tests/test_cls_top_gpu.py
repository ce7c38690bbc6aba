"""GPU: the top encoder layer on the CLS rows only (nbest_encoder_desc.cls_top, NBestSTCModel.cls_top) against the full-width
top layer - same seed, same inputs, same dropout decisions - plus its composition with gradient accumulation, a backward in chunks,
frozen matrices, the weight-gradient modes and the transcript pass, run-to-run bit equality, and the passes that keep the
full-width layer.

Bars.  fp32: the two paths compute the same sums over the same operands in another order, so scores agree to 1e-5 absolute and
every gradient tensor to 1e-4 of its norm; a wrong dropout keep index would show as an O(1) difference.  "Tensor" is the library's:
the Q | K | V biases of a layer are ONE [3H] gradient tensor (bqkv), compared as one - the key third of it is mathematically zero
(softmax does not see a key bias), pure rounding noise with no norm of its own to be relative to.  asr_cls: 1e-5 of the largest
CLS entry (sums of <= 3072 products in another order: sqrt(3072) x 2^-24 = 3e-6 of the operands' scale).  Loss parts: every term
is 1-Lipschitz in one score, so B x (top + bottom scores) x 1e-5.
bf16: no tolerance is invented.  The flag-on path is held to the floor-based bars of tests/test_model_gpu.py on its golden
cases; flag on against flag off is logged (cls_top_parity.log, beside the model parity log of tests/test_model_gpu.py)."""
import os

import pytest
import torch

from test_infer_gpu import _batch, _model
from test_model_gpu import LOG as MODEL_LOG

pytestmark = pytest.mark.gpu
LOG = os.path.join(os.path.dirname(MODEL_LOG), "cls_top_parity.log")
LAY = "bert_encoder.encoder.layer.%d."
S_VALUES = [5, 77, 114, 128, 129, 256]      # either side of the attention dispatch boundaries (32-key blocks, 128, 256)


def _log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")
    print(msg)


_MODELS = {}


def _shared_model(labels, family, dtype, L=2):
    """one model per (family, dtype, L) for the whole module: a run sets the dropout rates, the flag and the step counter"""
    key = (family, dtype, L)
    if key not in _MODELS:
        m, cfg, _ = _model(labels, family, L=L, dtype=dtype)
        m.train()
        _MODELS[key] = (m, cfg)
    return _MODELS[key]


def _grads(m):
    """name -> fp32 clone of every gradient tensor; the Q | K | V biases of a layer as the one [3H] tensor the library forms"""
    out, qkv = {}, {}
    for n, p in m.named_parameters():
        if p.grad is None or "pooler" in n:
            continue
        g = p.grad.detach().float().clone()
        if ".attention.self." in n and n.endswith(".bias"):
            qkv.setdefault(n.split(".attention.self.")[0], {})[n.split(".")[-2]] = g
        else:
            out[n] = g
    for pre, d in qkv.items():
        out[pre + ".attention.self.qkv.bias"] = torch.cat([d["query"], d["key"], d["value"]])
    return out


def _run(m, b, on, drop, seg=True, add_l2=False, **kw):
    m.cfg.hidden_dropout_prob = m.cfg.attention_probs_dropout_prob = drop
    m.cls_top = on
    m.step_counter = 0
    out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if seg else None, trans_input_ids=b["tids"] if add_l2 else None,
                             trans_seg_ids=b["tseg"] if add_l2 else None, add_l2_loss=add_l2, **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.detach().float().clone()) for k, v in out.items()}


def _compare(tag, o1, g1, o0, g0, f32):
    """flag on (o1, g1) against flag off (o0, g0): logged; asserted at the fp32 bars"""
    n_scores = sum(o0[k].numel() for k in ("top", "final", "bott"))
    sc = max((o1[k] - o0[k]).abs().max().item() for k in ("top", "final", "bott"))
    cl = (o1["asr_cls"] - o0["asr_cls"]).abs().max().item()
    cls_scale = o0["asr_cls"].abs().max().item()
    lo = (o1["loss_parts"] - o0["loss_parts"]).abs().max().item()
    assert g1.keys() == g0.keys()
    rel = sorted(((g1[n] - g0[n]).norm().item() / max(g0[n].norm().item(), 1e-30), n) for n in g0)
    _log("%s: scores %.2e  asr_cls %.2e (scale %.1f)  loss parts %.2e  gradients: worst %.2e (%s), median %.2e" % (
        tag, sc, cl, cls_scale, lo, rel[-1][0], rel[-1][1][-48:], rel[len(rel) // 2][0]))
    for o in (o1, o0):
        assert all(torch.isfinite(v).all() for v in o.values() if v is not None)
    if not f32:
        return
    assert sc <= 1e-5, (tag, "scores", sc)
    assert cl <= 1e-5 * max(cls_scale, 1.0), (tag, "asr_cls", cl)
    assert lo <= 1e-5 * n_scores, (tag, "loss parts", lo)
    if o0.get("trans_cls") is not None:
        assert (o1["trans_cls"] - o0["trans_cls"]).abs().max().item() <= 1e-5 * max(o0["trans_cls"].abs().max().item(), 1.0)
    bad = [(r, n) for r, n in rel if r > 1e-4]
    assert not bad, (tag, bad[-4:])


def _on_off(tag, m, b, drop, f32, **kw):
    o1 = _run(m, b, True, drop, **kw)
    g1 = _grads(m)
    o0 = _run(m, b, False, drop, **kw)
    g0 = _grads(m)
    _compare(tag, o1, g1, o0, g0, f32)
    return g1, g0


# ---- 1. same decisions, same result ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_flag_on_equals_flag_off(dtype, drop, S, labels):
    """bert, 2 layers, B = 3 (odd S) or 4: scores, loss parts, asr_cls and every gradient tensor.  With dropout on, the fp32 leg is
    the check of the index rule: attention keeps of query 0, hidden-dropout keeps of rows b S"""
    m, cfg = _shared_model(labels, "bert", dtype)
    B = 3 if S % 2 else 4
    b = _batch(cfg, labels, B, S)
    f32 = dtype == torch.float32
    _on_off("on/off %s drop %.1f B %d S %3d" % ("f32 " if f32 else "bf16", drop, B, S), m, b, drop, f32)


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2"])
def test_bf16_flag_on_meets_the_golden_bars(name, labels, monkeypatch):
    """bf16 has no on/off tolerance of its own: the flag-on step is held to the floor-based bars of test_model_gpu.py against the
    reference's committed outputs, on its 2-layer golden cases - and the passes of that step did run the CLS-rows layer"""
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    import test_model_gpu as tm
    seen = []
    enc = NBestSTCModel._encode

    def spy(self, *a, **kw):
        rec = enc(self, *a, **kw)
        seen.append(rec.cls_top)
        return rec
    monkeypatch.setattr(NBestSTCModel, "_encode", spy)
    tm.test_step_matches_reference_outputs(name, torch.bfloat16, labels)
    assert seen and all(seen), seen


# ---- 2. masks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["bert", "xlm-roberta"])
@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_masks(dtype, drop, family, labels):
    """ragged lengths with trailing pads, and a row that is [CLS] followed by pads only.  bert: its only unmasked key is CLS;
    xlm-roberta (mask = ids > 0 for every family, CLS id 0, pad id 1): CLS itself is the one masked key.  Both position families"""
    m, cfg = _shared_model(labels, family, dtype)
    f32 = dtype == torch.float32
    for B, S in ((3, 37), (4, 128)):
        b = _batch(cfg, labels, B, S)
        b["ids"][1, 1:] = cfg.pad_token_id
        b["seg"][1, :] = 0
        b["ids"][2, S - S // 3:] = cfg.pad_token_id          # trailing pads, whatever length the ragged batch drew
        b["seg"][2, S - S // 3:] = 0
        n_keys = int((b["ids"][1] > 0).sum())
        assert n_keys == (1 if family == "bert" else S - 1)
        _on_off("masks %s %s drop %.1f B %d S %3d" % (family, "f32 " if f32 else "bf16", drop, B, S), m, b, drop, f32, seg=family == "bert")


# ---- 3. composition ----------------------------------------------------------------------------------------------------------------
def test_accumulate_over_two_micro_batches(labels):
    m, cfg = _shared_model(labels, "bert", torch.float32)
    b1, b2 = _batch(cfg, labels, 3, 77, seed=3), _batch(cfg, labels, 3, 77, seed=4)
    res = []
    for on in (True, False):
        _run(m, b1, on, 0.1)
        o = _run(m, b2, on, 0.1, accumulate=True)
        res.append((o, _grads(m)))
    _compare("accumulate f32", res[0][0], res[0][1], res[1][0], res[1][1], True)
    # and the second call did add: the sum differs from the second micro-batch alone
    _run(m, b2, True, 0.1)
    alone = _grads(m)
    w = LAY % 1 + "output.dense.weight"
    assert (res[0][1][w] - alone[w]).norm().item() > 1e-2 * alone[w].norm().item()


def test_backward_in_chunks_top_chunk_is_the_top_layer(labels):
    m, cfg = _shared_model(labels, "bert", torch.float32)
    b = _batch(cfg, labels, 4, 114)
    done = []
    g1, _ = _on_off("chunks f32", m, b, 0.1, True, chunks=[(0, 1), (1, 2)], on_chunk_done=lambda lo, hi: done.append((lo, hi)))
    assert done == [(1, 2), (0, 1)] * 2
    # chunked equals whole, flag on: the same launches in the same order
    _run(m, b, True, 0.1)
    whole = _grads(m)
    assert all(torch.equal(whole[n], g1[n]) for n in whole)


@pytest.mark.parametrize("which", ["attention.output.dense.weight", "output.dense.weight"])
def test_frozen_top_matrix(which, labels):
    """Wo or W2 of the top layer frozen through requires_grad: no gradient for it, every other tensor as with the full-width layer"""
    m, cfg = _shared_model(labels, "bert", torch.float32)
    b = _batch(cfg, labels, 3, 77)
    p = dict(m.named_parameters())[LAY % 1 + which]
    p.requires_grad_(False)
    try:
        g1, g0 = _on_off("frozen %s f32" % which, m, b, 0.1, True)
        assert LAY % 1 + which not in g1 and p.grad is None
        assert LAY % 1 + which.replace("weight", "bias") in g1
    finally:
        p.requires_grad_(True)
        m.zero_grad()
        _run(m, b, True, 0.0)          # the plan sees every tensor trainable again


def _check_event_pairs(m, b, B, S, L, on):
    """desc.wgrad_events: a backward records nbest_encoder_wgrad_launches_per_layer x L pairs, the first ones of the array, each
    end after its begin - with the flag as without"""
    import ctypes as C
    from nbest_amd import hipabi as hb
    n_ev = 8 * L
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
    for e in evs:
        e.record()
    torch.cuda.synchronize()
    mark = torch.cuda.Event(enable_timing=True)
    arr = (C.c_void_p * n_ev)(*[e.cuda_event for e in evs])
    desc = m._pass(B, S, 0).desc
    per_layer = hb.lib().nbest_encoder_wgrad_launches_per_layer(C.byref(desc))
    desc.wgrad_events, desc.wgrad_events_n = C.cast(arr, C.POINTER(C.c_void_p)), n_ev
    try:
        mark.record()
        _run(m, b, on, 0.1)
    finally:
        desc.wgrad_events, desc.wgrad_events_n = None, 0
    fresh = [mark.elapsed_time(e) >= 0.0 for e in evs]
    assert fresh == [True] * (2 * per_layer * L) + [False] * (n_ev - 2 * per_layer * L), (on, per_layer, fresh)
    assert all(evs[2 * i].elapsed_time(evs[2 * i + 1]) >= 0.0 for i in range(per_layer * L))
    assert sum(evs[2 * i].elapsed_time(evs[2 * i + 1]) for i in range(per_layer * L)) > 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wgrad_group_modes(dtype, labels):
    """4 layers of bert-base width, B S = 512, wgrad_group NEVER / ALWAYS / WINDOW.  fp32 (every mode resolves to the split-K
    launches there): flag on against flag off at the fp32 bars.  bf16, where the grouped launch and the windows exist: flag on
    against flag off is logged per mode, and what is asserted needs no bf16 tolerance - with the flag on, the modes see bit-equal
    operands, so the top layer's attention-out / FFN gradients (the same plain launches in every mode) are bit-equal across the
    modes and every other tensor differs from mode NEVER by the fp32 summation order over K only: 1e-4 of its norm"""
    from nbest_amd import hipabi as hb
    f32 = dtype == torch.float32
    res = {}
    for mode in (hb.WGRAD_GROUP_NEVER, hb.WGRAD_GROUP_ALWAYS, hb.WGRAD_GROUP_WINDOW):
        m, cfg, _ = _model(labels, "bert", L=4, dtype=dtype)
        m.train()
        m.wgrad_group = mode
        b = _batch(cfg, labels, 4, 128)
        if not f32:
            d = m._desc(4, 128, 0).desc
            assert hb.encoder_wgrad_plan(d, 0, 4)["mode"] == mode
        res[mode] = _on_off("wgrad_group %d %s" % (mode, "f32 " if f32 else "bf16"), m, b, 0.1, f32)[0]
        for on in (True, False):
            _check_event_pairs(m, b, 4, 128, 4, on)
    if f32:
        return
    never = res[hb.WGRAD_GROUP_NEVER]
    small = [LAY % 3 + w for w in ("attention.output.dense.weight", "intermediate.dense.weight", "output.dense.weight")]
    for mode in (hb.WGRAD_GROUP_ALWAYS, hb.WGRAD_GROUP_WINDOW):
        for n, g in res[mode].items():
            if n in small or not n.endswith("weight") or "encoder.layer" not in n:
                assert torch.equal(g, never[n]), (mode, n)
            else:
                r = (g - never[n]).norm().item() / never[n].norm().item()
                assert r <= 1e-4, (mode, n, r)


def test_transcript_pass(labels):
    """--add_l2_loss: both encoder passes run the CLS-rows layer, the transcript pass (S_t = 16) first in the backward"""
    for family in ("bert", "xlm-roberta"):
        m, cfg = _shared_model(labels, family, torch.float32)
        b = _batch(cfg, labels, 4, 129)
        _on_off("add_l2_loss %s f32" % family, m, b, 0.1, True, seg=family == "bert", add_l2=True)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_are_bit_equal(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    arenas = []
    for _ in range(2):
        m, cfg, _ = _model(labels, "bert", L=2, dtype=dtype)
        m.train()
        assert m.cls_top
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        b = _batch(cfg, labels, 4, 77)
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        g = m.arena.g.clone()
        opt.step()
        torch.cuda.synchronize()
        arenas.append((g, m.arena.p.clone()))
    assert torch.equal(arenas[0][0], arenas[1][0]) and torch.equal(arenas[0][1], arenas[1][1])
    assert torch.isfinite(arenas[0][0]).all() and arenas[0][0].abs().max().item() > 0


# ---- 5. fallbacks ----------------------------------------------------------------------------------------------------------------------
def _flags_of(monkeypatch):
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    seen = []
    enc = NBestSTCModel._encode

    def spy(self, *a, **kw):
        rec = enc(self, *a, **kw)
        seen.append(rec.cls_top)
        return rec
    monkeypatch.setattr(NBestSTCModel, "_encode", spy)
    return seen


def test_fp8w_keeps_the_full_width_layer(labels, monkeypatch):
    seen = _flags_of(monkeypatch)
    res = []
    for on in (True, False):
        m, cfg, _ = _model(labels, "bert", L=2, dtype=torch.bfloat16, fp8=True)
        m.train()
        m.cls_top = on
        b = _batch(cfg, labels, 4, 77)
        for _ in range(2):               # calibration pass, then the fp8 pass
            out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
        torch.cuda.synchronize()
        res.append((out, m.arena.g.clone()))
    assert seen and not any(seen)
    assert torch.equal(res[0][1], res[1][1]) and all(torch.equal(res[0][0][k], res[1][0][k]) for k in ("top", "final", "bott", "asr_cls"))


def test_eval_head_mask_attribute_and_attention_maps_are_todays(labels, monkeypatch):
    """eval passes (also under a head mask), attribute() and return_attns give the bits they give with the flag switched off: the
    model routes them to the full-width layer.  return_attns in training mode under no_grad too, whose maps come from the stash"""
    seen = _flags_of(monkeypatch)
    m, cfg = _shared_model(labels, "bert", torch.float32)
    b = _batch(cfg, labels, 3, 37)
    mask = torch.ones(2, cfg.num_attention_heads)
    mask[1, 3] = 0.0
    mask[0, 5] = 0.5
    res = []
    for on in (True, False):
        m.cls_top = on
        m.eval()
        r = {}
        r["eval"] = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)["final"].clone()
        top, _, fin, attns, cls, _ = m(None, b["ids"], seg_ids=b["seg"], return_attns=True)
        r["fin"], r["attn_top"], r["cls"] = fin.clone(), attns[-1].clone(), cls.clone()
        r["attr"] = m.attribute(b["ids"], seg_ids=b["seg"], steps=4)["attr"].clone()
        m.set_head_mask(mask)
        r["masked"] = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)["final"].clone()
        m.set_head_mask(None)
        m.train()
        m.cfg.hidden_dropout_prob = m.cfg.attention_probs_dropout_prob = 0.0
        m.step_counter = 0
        with torch.no_grad():
            r["train_attn"] = m(None, b["ids"], seg_ids=b["seg"], return_attns=True)[3][-1].clone()
        torch.cuda.synchronize()
        res.append(r)
    assert not any(seen), seen
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    assert torch.allclose(res[0]["attn_top"].sum(-1), torch.ones_like(res[0]["attn_top"].sum(-1)), atol=1e-5)


def test_stale_stash_is_refused_across_settings(labels):
    """a backward on a stash that a forward with the other setting has overwritten is caught by the generation check"""
    m, cfg = _shared_model(labels, "bert", torch.float32)
    m.cfg.hidden_dropout_prob = m.cfg.attention_probs_dropout_prob = 0.0
    b = _batch(cfg, labels, 3, 37)
    for first in (True, False):
        m.zero_grad()
        m.cls_top = first
        top, _, fin, _, _ = m(None, b["ids"], seg_ids=b["seg"])
        m.cls_top = not first
        m(None, b["ids"], seg_ids=b["seg"])
        with pytest.raises(RuntimeError, match="another forward ran"):
            fin.sum().backward()
    m.cls_top = True
