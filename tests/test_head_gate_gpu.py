"""GPU: head gates and head importance - nbest_head_gate_fwd / _bwd against fp64 torch, the all-ones mask against no mask (bit for
bit), masked scores and NBestSTCModel.head_gate_grad against the fp64 oracle (tests/test_head_gate_cpu.py), predict against the eval
forward under a mask, a pruned head against zeroed Wo columns, the training state head_gate_grad must leave alone, the descriptor
refusals and --head_mask / --head_importance end to end."""
import ctypes as C
import json
import os
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_attrib_cpu import oracle_model
from test_head_gate_cpu import case_tensors, mixed_mask, oracle_gated
from test_infer_gpu import _batch, _model, _same_state, _state
from test_model_gpu import _cmp, _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rnd(*shape, dtype=torch.float32, s=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * s).to(dtype).to(DEV)


def _gate(heads, seed):
    """a gate with the special values 1, 0 and 0.5 and random floats (negative ones too)"""
    g = _rnd(heads, s=1.5, seed=seed)
    g[0], g[1], g[2] = 1.0, 0.0, 0.5
    return g


def _scaled_ok(got, ref64, dtype):
    """T(gate * float(x)) against the fp64 product: fp32 - the fp32 product of two fp32 numbers is the correctly rounded exact
    product, which fp64 holds exactly: bit-equal; bf16 - rounded twice (fp32, then bf16): within one bf16 ulp, 2^-8 relative"""
    if dtype == torch.float32:
        return torch.equal(got.double(), ref64.float().double())
    return bool(((got.double() - ref64).abs() <= 2.0 ** -8 * ref64.abs()).all())


# ---- 1. the kernels against fp64 torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("heads", [12, 16])
@pytest.mark.parametrize("M", [1, 5, 130])
def test_head_gate_fwd(M, heads, dtype):
    from nbest_amd import hipabi as hb
    H = heads * 64
    x = _rnd(M, H, dtype=dtype, seed=M + heads)
    gate = _gate(heads, 1)
    ref = x.double().view(M, heads, 64) * gate.double()[None, :, None]
    out = hb.head_gate_fwd(x, gate, heads)
    assert _scaled_ok(out.view(M, heads, 64), ref, dtype), "out of place"
    assert torch.equal(out.view(M, heads, 64)[:, 0], x.view(M, heads, 64)[:, 0]), "a gate of 1 must leave the bits as they are"
    assert torch.all(out.view(M, heads, 64)[:, 1] == 0), "a gate of 0 must give exact zeros"
    # ld_out > H: rows of a wider buffer, whose other columns stay untouched
    wide = torch.full((M, H + 64), 7.0, dtype=dtype, device=DEV)
    hb.head_gate_fwd(x, gate, heads, out=wide[:, :H])
    assert torch.equal(wide[:, :H], out) and torch.all(wide[:, H:] == 7.0)
    # ld_in > H, and in place
    src = torch.full((M, H + 128), 3.0, dtype=dtype, device=DEV)
    src[:, :H] = x
    hb.head_gate_fwd(src[:, :H], gate, heads, out=src[:, :H])
    assert torch.equal(src[:, :H], out) and torch.all(src[:, H:] == 3.0)
    y = x.clone()
    hb.head_gate_fwd(y, gate, heads, out=y)
    assert torch.equal(y, out), "in place differs from out of place"
    ones = torch.ones(heads, device=DEV)
    assert torch.equal(hb.head_gate_fwd(x, ones, heads), x)
    assert torch.all(hb.head_gate_fwd(x, torch.zeros(heads, device=DEV), heads) == 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("heads", [12, 16])
@pytest.mark.parametrize("S", [1, 37, 128, 300])
def test_head_gate_bwd(S, heads, dtype):
    from nbest_amd import hipabi as hb
    B, H = 3, heads * 64
    ctx = _rnd(B * S, H, dtype=dtype, seed=S)
    dctx0 = _rnd(B * S, H, dtype=dtype, s=0.3, seed=S + 1)
    gate = _gate(heads, 2)
    # fp64 sum of the same (fp32 / bf16) inputs: the kernel accumulates in fp32 in both dtypes
    ref = (ctx.double() * dctx0.double()).view(B, S, heads, 64).sum(dim=(1, 3))
    d1, d2 = dctx0.clone(), dctx0.clone()
    g1 = hb.head_gate_bwd(ctx, d1, gate, B, S, heads)
    g2 = hb.head_gate_bwd(ctx, d2, gate, B, S, heads)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2) and torch.equal(d1, d2), "two runs differ"
    err, scale = (g1.double() - ref).abs().max().item(), ref.abs().max().item()
    print("head_gate_bwd S=%d heads=%d %s: |dgate - ref| %.3e, max|ref| %.3e (ratio %.2e)" % (S, heads, dtype, err, scale, err / scale))
    assert err <= 1e-5 * scale, "dgate vs fp64: %.3e > 1e-5 x %.3e" % (err, scale)
    sref = dctx0.double().view(B, S, heads, 64) * gate.double()[None, None, :, None]
    assert _scaled_ok(d1.view(B, S, heads, 64), sref, dtype), "dctx <- gate * dctx"
    assert torch.equal(d1.view(B, S, heads, 64)[:, :, 0], dctx0.view(B, S, heads, 64)[:, :, 0])
    # all-ones gate: dctx untouched, dgate as before (it does not depend on the gate)
    d3 = dctx0.clone()
    g3 = hb.head_gate_bwd(ctx, d3, torch.ones(heads, device=DEV), B, S, heads)
    assert torch.equal(d3, dctx0), "a gate of 1 must leave dctx bit-identical"
    assert torch.equal(g3, g1)
    # dgate == NULL: scale only
    d4 = dctx0.clone()
    assert hb.head_gate_bwd(None, d4, gate, B, S, heads, want_dgate=False) is None
    assert torch.equal(d4, d1)
    torch.cuda.synchronize()


# ---- 2. an all-ones mask is the model without a mask, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_ones_mask_is_identity(dtype, labels):
    m, cfg, _ = _model(labels, dtype=dtype)
    m.eval()
    b = _batch(cfg, labels, 4, 48)
    tg = [(0, 1), (2, 4), (3, 0)]

    def run():
        ev = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)
        ev = {k: v.clone() for k, v in ev.items() if v is not None}
        pr = m.predict(b["ids"], seg_ids=b["seg"])
        pa = m.predict(b["ids"], seg_ids=b["seg"], return_attns=True)
        at = m.attribute(b["ids"], seg_ids=b["seg"], targets=tg, steps=4)
        torch.cuda.synchronize()
        return ev, pr, pa, at

    assert m.head_mask is None
    ref = run()
    m.set_head_mask(torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads))
    assert m.head_mask is not None and m.head_mask.device.type == "cuda" and "head_mask" not in "".join(m.state_dict().keys())
    got = run()
    m.set_head_mask(None)
    for name, r, g in zip(("forward_backward(need_grad=False)", "predict", "predict(return_attns)", "attribute"), ref, got):
        assert r.keys() == g.keys()
        for k in r:
            assert torch.equal(r[k], g[k]), "%s: %s differs under an all-ones mask" % (name, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_ones_gate_backward_is_identity(dtype, labels):
    """the dhidden of a no_param_grad backward with head_gate (all ones) and head_gate_grad set equals the one without"""
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, dtype=dtype)
    m.eval()
    b = _batch(cfg, labels, 4, 48)
    rec = m._encode(0, b["ids"], b["seg"], train=False)
    B, S, H, L, heads = 4, 48, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
    d = rec.ps.desc
    m._set_weights(d, "backward")
    ids, seg, pos, mask = rec.inputs
    act, ws = m._stash[0][:rec.ps.act_bytes], m._ws
    dcls = _rnd(B, H, seed=5)
    ones = torch.ones(L, heads, device=DEV)
    grad = torch.full((L, B, heads), float("nan"), device=DEV)

    def run(gated):
        dh = hb.cls_grad_scatter(dcls, B, S, H, dtype)
        d.no_param_grad = 1
        d.head_gate, d.head_gate_grad = (ones.data_ptr(), grad.data_ptr()) if gated else (None, None)
        rc = hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(m.arena.weights), hb.ptr(m.arena.w16t), hb.ptr(m.arena.p), None,
                                             hb.ptr(ids), hb.ptr(seg), hb.ptr(pos), hb.ptr(mask), hb.ptr(act), act.numel(), hb.ptr(dh),
                                             hb.ptr(ws), ws.numel(), 0, 0, L, 0, hb.stream_ptr())
        d.no_param_grad = 0
        d.head_gate = d.head_gate_grad = None
        assert rc == 0, hb.last_error()
        return dh

    ref, got = run(False), run(True)
    torch.cuda.synchronize()
    assert torch.equal(ref, got), "dhidden differs under all-ones gates"
    assert bool(torch.isfinite(grad).all()) and grad.abs().max().item() > 0


# ---- 3. against the fp64 oracle ---------------------------------------------------------------------------------------------------
def _hip_model(meta, labels, dtype):
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    _, ocfg, cfg, sd, batch = oracle_model(meta, labels)
    m = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=dtype, dropout=0.0, seed=1)
    m.load_reference_state(sd)
    m.eval()
    return m, cfg, batch


def _hip_masked(m, meta, batch, mask):
    """final scores of the eval forward and of predict, and head_gate_grad, under ``mask``"""
    ids, seg, y = (None if t is None else t.to(DEV) for t in case_tensors(meta, batch))
    m.set_head_mask(mask)
    ev = m.forward_backward(ids, y, seg_ids=seg, need_grad=False)["final"].double().cpu()
    pr = m.predict(ids, seg_ids=seg)["final"].double().cpu()
    hg = m.head_gate_grad(ids, y, seg_ids=seg)
    torch.cuda.synchronize()
    return ev, pr, hg["grad"].double().cpu(), hg["loss_parts"].double().cpu()


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2"])
def test_masked_scores_and_gate_grad_match_oracle_fp32(name, labels):
    """fp32, a mask with zeros, a 0.5 and ones in both layers: final scores within 1e-4 absolute (the bar of
    test_predict_matches_reference_outputs), head_gate_grad per utterance within 1e-3 relative (the bar of the fp32 IG test);
    the gradient of a head gated 0 is part of the norm like every other"""
    meta, _ = load_case(name)
    om, ocfg, cfg, _, batch = oracle_model(meta, labels)
    m, _, _ = _hip_model(meta, labels, torch.float32)
    ids, seg, y = case_tensors(meta, batch)
    mask = mixed_mask(ocfg.num_hidden_layers, ocfg.num_attention_heads)
    _, _, fin_ref, total_ref, g_ref = oracle_gated(om, ocfg, labels, ids, seg, y, mask)
    ev, pr, g, loss = _hip_masked(m, meta, batch, mask)
    for tag, fin in (("eval forward", ev), ("predict", pr)):
        err = (fin - fin_ref).abs().max().item()
        print("fp32 %s %s: |final - ref| %.3e" % (name, tag, err))
        assert err <= 1e-4, "%s %s: |final - ref| = %.3e > 1e-4" % (name, tag, err)
    assert abs(loss[:3].sum().item() - total_ref.item()) <= 1e-4 * abs(total_ref.item())
    assert g.shape == g_ref.shape
    for b in range(ids.shape[0]):
        rel = (g[:, b] - g_ref[:, b]).norm().item() / g_ref[:, b].norm().item()
        print("fp32 %s utterance %d: |g - g_ref| / |g_ref| = %.3e" % (name, b, rel))
        assert rel <= 1e-3, "%s utterance %d: |g - g_ref| / |g_ref| = %.3e > 1e-3" % (name, b, rel)
    pruned = (mask == 0)
    assert g[:, 0][pruned].abs().max().item() > 0, "pruned heads have a gradient"
    # the mask matters: the un-masked scores differ from the masked reference by more than the bar
    m.set_head_mask(None)
    plain = m.predict(*(None if t is None else t.to(DEV) for t in (ids, seg)))["final"].double().cpu()
    assert (plain - fin_ref).abs().max().item() > 1e-3


def _bf16_leg_gated(om, ocfg, labels, ids, seg, y, mask):
    """the bf16-storage leg (oracle/bf16sim.py's rounding points: bs.encode without fp8) with the head gate: ctx is stored in bf16,
    then multiplied by the fp32 gate and stored in bf16 again (nbest_head_gate_fwd); on the way back the gradient w.r.t. the gated
    copy and the one w.r.t. ctx are rounded (the dgrad GEMM's bf16 output, nbest_head_gate_bwd's in-place store), the gate gradient
    is their fp32 product sum.  Returns (final, grad [L, B, heads]) in fp64."""
    import math
    import torch.nn.functional as F
    from oracle import bf16sim as bs, stc
    from oracle.encoder import position_ids_for
    enc = om.bert_encoder
    E = enc.embeddings
    B, S = ids.shape
    H, nh, L = ocfg.hidden_size, ocfg.num_attention_heads, ocfg.num_hidden_layers
    d = H // nh
    g = mask.float()[:, None, :].expand(L, B, nh).clone().requires_grad_(True)
    km = ids > 0
    s0 = torch.zeros_like(ids) if (seg is None or ocfg.family == "xlm-roberta") else seg
    pos = position_ids_for(ocfg, ids)
    # (rounding commutes with the gather: only the rows the batch reads are rounded, not a 250 002-row table per draw)
    e = (bs.rw(E.word_embeddings.weight[ids]) + F.embedding(s0, bs.rw(E.token_type_embeddings.weight))
         + F.embedding(pos, bs.rw(E.position_embeddings.weight)))
    x = bs.ract(bs._ln(e, E.LayerNorm))
    split = lambda t: t.view(B, S, nh, d).transpose(1, 2)
    for l, lyr in enumerate(enc.encoder.layer):
        sa, ao = lyr.attention.self, lyr.attention.output
        q, k, v = (bs.ract(F.linear(x, bs.rw(mm.weight), mm.bias)) for mm in (sa.query, sa.key, sa.value))
        ctx = bs.ract(bs._AttnCore.apply(split(q), split(k), split(v), km, 1.0 / math.sqrt(d)).transpose(1, 2).reshape(B, S, H))
        ctx = bs.ract(ctx * g[l].repeat_interleave(d, dim=-1)[:, None, :])
        r1 = bs.ract(F.linear(ctx, bs.rw(ao.dense.weight), ao.dense.bias) + x)
        x1 = bs.ract(bs._ln(r1, ao.LayerNorm))
        hact = bs._GeluStore.apply(F.linear(x1, bs.rw(lyr.intermediate.dense.weight), lyr.intermediate.dense.bias), True)
        r2 = bs.ract(F.linear(hact, bs.rw(lyr.output.dense.weight), lyr.output.dense.bias) + x1)
        x = bs.ract(bs._ln(r2, lyr.output.LayerNorm))
    top, bottoms, final = om.clf(x[:, 0, :])
    b2t = stc.bottom2top_matrix(labels.top2bottom)
    _, total, _ = stc.total_loss(top, bottoms, final, y.float(), labels.top2bottom, b2t)
    grad, = torch.autograd.grad(total, g)
    return final.detach().double(), grad.detach().double()


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2"])
def test_masked_scores_and_gate_grad_match_oracle_bf16(name, labels):
    """bf16 against the fp64 oracle under the same mask: the bar is 2 x the floor of a bf16-storage leg - the maximum over five draws
    (the weights as they are and four copies jittered by 2^-12 relative, as test_attrib_gpu draws them; of the word table only the
    rows the batch reads are jittered - the noise is independent per element and no other row is read) - per case for the final
    scores (max |final - ref|), per utterance for the gate gradient (||g - g_ref|| / ||g_ref||).  Worst HIP / floor ratios seen
    on an MI355X: DESIGN.md section 4 (head gates)."""
    meta, _ = load_case(name)
    om64, ocfg, cfg, _, batch = oracle_model(meta, labels)
    om32 = oracle_model(meta, labels, dtype=torch.float32)[0]
    m, _, _ = _hip_model(meta, labels, torch.bfloat16)
    ids, seg, y = case_tensors(meta, batch)
    B = ids.shape[0]
    mask = mixed_mask(ocfg.num_hidden_layers, ocfg.num_attention_heads)
    _, _, fin_ref, _, g_ref = oracle_gated(om64, ocfg, labels, ids, seg, y, mask)
    fin_floor, g_floor = 0.0, torch.zeros(B, dtype=torch.float64)
    word = om32.bert_encoder.embeddings.word_embeddings.weight
    rows = torch.unique(ids)
    params = list(om32.parameters())
    saved = [(p[rows] if p is word else p).detach().clone() for p in params]
    for draw in range(5):
        if draw:
            gj = torch.Generator().manual_seed(1000003 * meta["seed"] + draw)
            with torch.no_grad():
                for p, q in zip(params, saved):
                    jit = q * (1.0 + 2.0 ** -12 * (2.0 * torch.rand(q.shape, generator=gj) - 1.0))
                    if p is word:
                        p[rows] = jit
                    else:
                        p.copy_(jit)
        fin_leg, g_leg = _bf16_leg_gated(om32, ocfg, labels, ids, seg, y, mask)
        fin_floor = max(fin_floor, (fin_leg - fin_ref).abs().max().item())
        for b in range(B):
            g_floor[b] = max(g_floor[b].item(), (g_leg[:, b] - g_ref[:, b]).norm().item() / g_ref[:, b].norm().item())
    ev, pr, g, _ = _hip_masked(m, meta, batch, mask)
    e_ev, e_pr = (ev - fin_ref).abs().max().item(), (pr - fin_ref).abs().max().item()
    rels = [(g[:, b] - g_ref[:, b]).norm().item() / g_ref[:, b].norm().item() for b in range(B)]
    worst = max(r / g_floor[b].item() for b, r in enumerate(rels))
    msg = "bf16 head gates %s: HIP / floor: final (eval forward) %.2f, final (predict) %.2f, gate grad %.2f (worst utterance); floors %.2e / %.2e" % (
        name, e_ev / fin_floor, e_pr / fin_floor, worst, fin_floor, g_floor.max().item())
    print(msg)
    _log(msg)
    assert e_ev <= 2.0 * fin_floor, "%s eval forward: |final - ref| %.3e > 2 x floor %.3e" % (name, e_ev, fin_floor)
    assert e_pr <= 2.0 * fin_floor, "%s predict: |final - ref| %.3e > 2 x floor %.3e" % (name, e_pr, fin_floor)
    for b, r in enumerate(rels):
        assert r <= 2.0 * g_floor[b].item(), "%s utterance %d: |g - g_ref| / |g_ref| = %.3e > 2 x floor %.3e" % (name, b, r, g_floor[b].item())


# ---- 4. consistency -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(3, 40), (4, 48)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_masked_predict_agrees_with_masked_eval_forward(B, S, dtype, labels):
    """tolerances of test_infer_gpu.test_predict_agrees_with_eval_forward"""
    m, cfg, _ = _model(labels, "bert", dtype=dtype)
    b = _batch(cfg, labels, B, S)
    m.eval()
    m.set_head_mask(mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads))
    ev = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)
    pr = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    tag = "masked agree B=%d S=%d %s " % (B, S, "f32" if f32 else "bf16")
    _cmp(tag + "cls", pr["cls"], ev["asr_cls"].float().cpu(), rtol=1e-5 if f32 else 2.0 ** -7)
    _cmp(tag + "final", pr["final"], ev["final"].cpu(), atol=1e-6 if f32 else 2e-3)
    if f32:
        assert torch.equal(pr["pred"], m.decode(ev["top"], ev["bott"]))
    m.set_head_mask(None)
    plain = m.predict(b["ids"], seg_ids=b["seg"])
    assert not torch.equal(plain["cls"], pr["cls"]), "the mask changed nothing"


def test_pruned_head_equals_zeroed_wo_columns(labels):
    """gate 0 on head h of layer l against a model whose attention-output columns of that head are zero: <= 1e-6 relative on the
    CLS rows (fp32; both paths add exact zeros for the head, in the same places of the same sums)"""
    from nbest_amd.model import NBestSTCModel
    m, cfg, sd = _model(labels, dtype=torch.float32)
    b = _batch(cfg, labels, 4, 48)
    L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
    pruned = [(0, 3), (1, 0), (1, 11)]
    mask = torch.ones(L, heads)
    sd2 = {k: v.copy() for k, v in sd.items()}
    for l, h in pruned:
        mask[l, h] = 0.0
        sd2["bert_encoder.encoder.layer.%d.attention.output.dense.weight" % l][:, h * 64:(h + 1) * 64] = 0.0
    m2 = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=torch.float32, dropout=0.3, seed=7)
    m2.load_reference_state(sd2)
    m.eval()
    m2.eval()
    m.set_head_mask(mask)
    for tag, f in (("eval forward", lambda mm: mm.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)["asr_cls"].float().clone()),
                   ("predict", lambda mm: mm.predict(b["ids"], seg_ids=b["seg"])["cls"].float())):
        got, ref = f(m), f(m2)
        torch.cuda.synchronize()
        rel = (got - ref).abs().max().item() / ref.abs().max().item()
        print("pruned heads vs zeroed Wo columns, %s: rel %.3e, bit-identical %s" % (tag, rel, torch.equal(got, ref)))
        assert rel <= 1e-6, "%s: %.3e" % (tag, rel)


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_head_gate_grad_leaves_training_state_alone(mode, labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, dtype=torch.float32 if mode == "f32" else torch.bfloat16)
    m.train()
    b = _batch(cfg, labels, 4, 48)
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    for _ in range(2):
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        opt.step()
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    torch.cuda.synchronize()
    before = _state(m)
    out = m.head_gate_grad(b["ids"], b["labels"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    assert out["grad"].shape == (cfg.num_hidden_layers, 4, cfg.num_attention_heads) and bool(torch.isfinite(out["grad"]).all())
    after = _state(m)
    after["stash"].pop("headgrad", None)
    _same_state(before, after)
    assert m.head_mask is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_after_head_gate_grad_is_unchanged(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_hg in (False, True):
        m, cfg, _ = _model(labels, dtype=dtype)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_hg:
            m.head_gate_grad(b["ids"], b["labels"], seg_ids=b["seg"])
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after head_gate_grad() differs"


def test_training_under_a_mask_raises(labels):
    m, cfg, _ = _model(labels, dtype=torch.float32)
    m.train()
    b = _batch(cfg, labels, 4, 48)
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    g0, step0 = m.arena.g.clone(), m.step_counter
    m.set_head_mask(torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads))
    with pytest.raises(RuntimeError, match="head mask"):
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    with pytest.raises(RuntimeError, match="head mask"):
        m(None, b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    assert torch.equal(m.arena.g, g0) and m.step_counter == step0, "a refused call must leave the gradients alone"
    with pytest.raises(ValueError):
        m.set_head_mask(torch.ones(cfg.num_attention_heads, cfg.num_hidden_layers))
    m.set_head_mask(None)
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    torch.cuda.synchronize()


def test_fp8w_model_under_a_mask(labels):
    """the stash forward of an fp8w model refuses a mask (before anything is enqueued); its predict runs the bf16 copy and equals
    the bf16 model's masked predict"""
    m8, cfg, _ = _model(labels, dtype=torch.bfloat16, fp8=True)
    mb, _, _ = _model(labels, dtype=torch.bfloat16)
    b = _batch(cfg, labels, 4, 48)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    m8.eval()
    m8.set_head_mask(mask)
    mb.set_head_mask(mask)
    with pytest.raises(RuntimeError, match="head_gate"):
        m8.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)
    o8, ob = m8.predict(b["ids"], seg_ids=b["seg"]), mb.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    for k in ("cls", "final", "pred"):
        assert torch.equal(o8[k], ob[k]), k


# ---- 6. descriptor refusals ---------------------------------------------------------------------------------------------------------
def test_descriptor_refusals(labels):
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, dtype=torch.bfloat16)
    m.eval()
    b = _batch(cfg, labels, 2, 16)
    rec = m._encode(0, b["ids"], b["seg"], train=False)
    torch.cuda.synchronize()
    B, S, H, L, heads = 2, 16, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
    d = rec.ps.desc
    m._set_weights(d, "backward")
    ids, seg, pos, mask = rec.inputs
    act, ws = m._stash[0][:rec.ps.act_bytes], m._ws
    gate = torch.ones(L, heads, device=DEV)
    grad = torch.zeros(L, B, heads, device=DEV)
    dh = torch.zeros(B * S, H, dtype=torch.bfloat16, device=DEV)
    out = C.c_void_p()
    fwd = lambda: hb.lib().nbest_encoder_forward(C.byref(d), hb.ptr(m.arena.weights), hb.ptr(m.arena.p), hb.ptr(ids), hb.ptr(seg), hb.ptr(pos),
                                                 hb.ptr(mask), hb.ptr(act), act.numel(), hb.ptr(ws), ws.numel(), C.byref(out), hb.stream_ptr())
    bwd = lambda: hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(m.arena.weights), hb.ptr(m.arena.w16t), hb.ptr(m.arena.p),
                                                  hb.ptr(m.arena.g), hb.ptr(ids), hb.ptr(seg), hb.ptr(pos), hb.ptr(mask), hb.ptr(act),
                                                  act.numel(), hb.ptr(dh), hb.ptr(ws), ws.numel(), 0, 0, L, 0, hb.stream_ptr())
    g0, act0 = m.arena.g.clone(), act.clone()

    def refused(call, what):
        rc = call()
        err = hb.last_error()
        assert rc != 0 and "head_gate" in err, "%s: rc %d, %r" % (what, rc, err)

    # 1. head_gate with the fp8 forward
    w8, inv = torch.zeros(16, dtype=torch.uint8, device=DEV), torch.ones(4 * L, device=DEV)
    d.head_gate = gate.data_ptr()
    d.w8, d.w8_inv_scale = w8.data_ptr(), inv.data_ptr()
    refused(fwd, "w8 forward")
    d.no_param_grad = 1
    refused(bwd, "w8 backward")
    d.no_param_grad = 0
    d.w8 = d.w8_inv_scale = None
    # 2. head_gate with first_trainable > 0
    d.first_trainable = 1
    refused(fwd, "first_trainable forward")
    d.first_trainable = 0
    # 3. a backward with head_gate but without no_param_grad
    refused(bwd, "backward without no_param_grad")
    # 4. head_gate_grad without head_gate
    d.head_gate, d.head_gate_grad = None, grad.data_ptr()
    d.no_param_grad = 1
    refused(bwd, "head_gate_grad without head_gate")
    refused(fwd, "head_gate_grad without head_gate (forward)")
    d.no_param_grad = 0
    d.head_gate_grad = None
    torch.cuda.synchronize()
    assert torch.equal(m.arena.g, g0) and torch.equal(act, act0) and torch.all(grad == 0), "a refused call enqueued something"
    ws_inf = torch.empty(hb.lib().nbest_encoder_infer_ws_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    cls = torch.empty(B, H, dtype=torch.bfloat16, device=DEV)
    d.head_gate_grad = grad.data_ptr()
    with pytest.raises(RuntimeError, match="head_gate"):
        hb.encoder_infer(d, m.arena.weights, m.arena.p, ids, seg, pos, mask, ws_inf, cls)
    d.head_gate_grad = None


# ---- 7. --head_importance / --head_mask end to end -------------------------------------------------------------------------------
def test_cli_head_importance_and_head_mask(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    # trained as test_attrib_gpu.test_cli_predict_attribution: the model must predict labels for a pruned mask to be able to matter
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--lr", "1e-3", "--bert_lr", "1e-4", "--batchSize", "16", "--max_epoch", "4", "--experiment", exp,
              "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", "f32",
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "3", "--resume"]
    assert cli.main(common) == 0
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    n_in = len(open(src).read().strip("\n").split("\n"))
    imp_path = str(tmp_path / "imp.json")
    assert cli.main(common + ["--head_importance", imp_path, "--prune_heads", "3"]) == 0
    res = json.load(open(imp_path))
    L, heads = 2, 12
    assert res["utterances"] == n_in
    for key in ("importance", "normalized", "head_mask", "pruned_mask"):
        assert len(res[key]) == L and all(len(r) == heads for r in res[key]), key
    flat = [x for r in res["importance"] for x in r]
    assert all(x == x and 0.0 <= x < float("inf") for x in flat) and max(flat) > 0.0
    for r in res["normalized"]:
        assert abs(sum(x * x for x in r) - 1.0) <= 1e-9
    assert res["head_mask"] == [[1.0] * heads] * L
    pruned = res["pruned_mask"]
    assert sum(1 for r in pruned for x in r if x == 0.0) == 3 and all(x in (0.0, 1.0) for r in pruned for x in r)
    lowest = sorted((x, i) for i, x in enumerate(flat))[:3]
    assert sorted(i for _, i in lowest) == sorted(l * heads + h for l in range(L) for h in range(heads) if pruned[l][h] == 0.0)
    ones_path, pruned_path = str(tmp_path / "ones.json"), str(tmp_path / "pruned.json")
    json.dump([[1.0] * heads] * L, open(ones_path, "w"))
    json.dump(pruned, open(pruned_path, "w"))
    plain, ones_out, pruned_out = (str(tmp_path / n) for n in ("a.pred", "b.pred", "c.pred"))
    assert cli.main(common + ["--predict", src, "--predict_output", plain]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", ones_out, "--head_mask", ones_path]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", pruned_out, "--head_mask", pruned_path]) == 0
    assert open(ones_out, "rb").read() == open(plain, "rb").read(), ".pred differs under an all-ones --head_mask"
    assert len(open(pruned_out).read().split("\n")[:-1]) == n_in
    # the importance at the pruned mask: the file names the mask in force
    imp2 = str(tmp_path / "imp2.json")
    assert cli.main(common + ["--head_importance", imp2, "--head_mask", pruned_path]) == 0
    res2 = json.load(open(imp2))
    assert res2["head_mask"] == pruned and "pruned_mask" not in res2
    bad = str(tmp_path / "bad.json")
    json.dump([[1.0] * heads] * 3, open(bad, "w"))
    with pytest.raises(SystemExit, match="head_mask"):
        cli.main(common + ["--predict", src, "--predict_output", plain, "--head_mask", bad])
