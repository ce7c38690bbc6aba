"""GPU: integrated-gradients attribution - the interpolated embedding forward, the no_param_grad backward, nbest_embed_attrib against
fp64 torch, NBestSTCModel.attribute against the fp64 oracle IG (tests/test_attrib_cpu.py), chunking, the training state it must leave
alone and --predict_attribution end to end."""
import ctypes as C
import json
import os
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_attrib_cpu import default_baseline, oracle_ig, oracle_model
from test_infer_gpu import _batch, _model, _same_state, _state

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rnd(*shape, dtype=torch.float32, s=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * s).to(dtype).to(DEV)


def _tables(H, V=50, P=80, dtype=torch.float32, seed=0):
    return (_rnd(V, H, dtype=dtype, seed=seed), _rnd(2, H, dtype=dtype, s=0.5, seed=seed + 1), _rnd(P, H, dtype=dtype, s=0.5, seed=seed + 2),
            1.0 + _rnd(H, s=0.1, seed=seed + 3), _rnd(H, s=0.1, seed=seed + 4))


def _ids(family, B, S, pad, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 50, (B, S), generator=g)
    lens = [1 + (S - 1) * (b + 1) // B for b in range(B)]         # row 0 the shortest
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    ids[:, 0] = 0 if family == "xlm-roberta" else 2
    return ids.to(DEV)


def _pos(family, ids, pad):
    if family == "xlm-roberta":
        nonpad = ids.ne(pad).long()
        return (torch.cumsum(nonpad, dim=1) * nonpad + pad).contiguous()
    B, S = ids.shape
    return torch.arange(S, device=DEV).unsqueeze(0).expand(B, S).contiguous()


# ---- 1. interpolated embedding forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["bert", "xlm-roberta"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [768, 1024, 200])
def test_interp_forward(family, dtype, H):
    from nbest_amd import hipabi as hb
    pad = 1 if family == "xlm-roberta" else 0
    B, S = 6, 37
    word, tt, pt, gam, bet = _tables(H, dtype=dtype)
    ids = _ids(family, B, S, pad)
    base = default_baseline(ids, pad)
    seg = (torch.arange(S, device=DEV) > S // 2).long().unsqueeze(0).expand(B, S).contiguous() if family == "bert" else None
    pos = _pos(family, ids, pad)
    alpha = torch.tensor([1.0, 0.0, 0.25, 0.5, 1.0 / 3.0, 0.9], device=DEV)
    out, st = hb.embed_ln_fwd_interp(ids, base, alpha, seg, pos, word, tt, pt, gam, bet, 1e-12)
    o1, s1 = hb.embed_ln_fwd(ids, seg, pos, word, tt, pt, gam, bet, 1e-12)
    o0, s0 = hb.embed_ln_fwd(base, seg, pos, word, tt, pt, gam, bet, 1e-12)
    torch.cuda.synchronize()
    r = lambda t, b: t.view(B, S, -1)[b]
    assert torch.equal(r(out, 0), r(o1, 0)) and torch.equal(r(st, 0), r(s1, 0)), "alpha = 1 row differs from nbest_embed_ln_fwd"
    assert torch.equal(r(out, 1), r(o0, 1)) and torch.equal(r(st, 1), r(s0, 1)), "alpha = 0 row differs from nbest_embed_ln_fwd on x'"
    # intermediate alpha against fp64
    W, T, Pt = word.double(), tt.double(), pt.double()
    a = alpha.double()[:, None, None]
    E = ((1 - a) * W[base] + a * W[ids]) + (T[seg] if seg is not None else T[0]) + Pt[pos]
    mu, var = E.mean(-1, keepdim=True), E.var(-1, unbiased=False, keepdim=True)
    ref = (E - mu) / torch.sqrt(var + 1e-12) * gam.double() + bet.double()
    tol = 2e-5 if dtype == torch.float32 else 2.0 ** -7
    err = (out.view(B, S, H).double() - ref).abs().max().item()
    assert err <= tol * ref.abs().max().item(), "interpolated forward vs fp64: %.3e" % err


# ---- 2. no_param_grad backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_param_grad_backward(dtype, labels):
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, dtype=dtype)
    m.eval()
    b = _batch(cfg, labels, 4, 48)
    rec = m._encode(0, b["ids"], b["seg"], train=False)
    B, S, H, L = 4, 48, cfg.hidden_size, cfg.num_hidden_layers
    d = rec.ps.desc
    m._set_weights(d, "backward")
    ids, seg, pos, mask = rec.inputs
    act, ws = m._stash[0][:rec.ps.act_bytes], m._ws
    dcls = _rnd(B, H, seed=5)

    def run(npg, grad, with_emb=0, ft=0, nig=0):
        dh = hb.cls_grad_scatter(dcls, B, S, H, dtype)
        d.no_param_grad, d.first_trainable, d.no_input_grad = npg, ft, nig
        d.word_perm = hb.word_perm(ids).data_ptr() if with_emb else None
        rc = hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(m.arena.weights), hb.ptr(m.arena.w16t), hb.ptr(m.arena.p), hb.ptr(grad),
                                             hb.ptr(ids), hb.ptr(seg), hb.ptr(pos), hb.ptr(mask), hb.ptr(act), act.numel(), hb.ptr(dh),
                                             hb.ptr(ws), ws.numel(), 0, 0, L, with_emb, hb.stream_ptr())
        d.no_param_grad = d.first_trainable = d.no_input_grad = 0
        return rc, dh

    g = torch.zeros_like(m.arena.g)
    rc, ref = run(0, g)
    assert rc == 0
    g_before = m.arena.g.clone()
    rc, got = run(1, None)
    torch.cuda.synchronize()
    assert rc == 0, hb.last_error()
    assert torch.equal(got, ref), "no_param_grad dhidden differs from the ordinary backward's"
    assert torch.equal(m.arena.g, g_before)
    for kw in (dict(with_emb=1), dict(ft=1), dict(nig=1)):
        rc, _ = run(1, None, **kw)
        assert rc != 0 and "no_param_grad" in hb.last_error(), kw
    if dtype == torch.bfloat16:                                   # the fp8 forward (w8): refused before anything is enqueued
        w8, inv = torch.zeros(16, dtype=torch.uint8, device=DEV), torch.ones(4 * L, device=DEV)
        d.w8, d.w8_inv_scale = w8.data_ptr(), inv.data_ptr()
        rc, _ = run(1, None)
        d.w8 = d.w8_inv_scale = None
        assert rc != 0 and "no_param_grad" in hb.last_error()


@pytest.mark.parametrize("with_attn", [False, True])
def test_encoder_infer_refuses_interpolated_embeddings(with_attn, labels):
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, dtype=torch.bfloat16)
    b = _batch(cfg, labels, 3, 40)
    m.predict(b["ids"], seg_ids=b["seg"])                       # sizes the inference workspace
    B, S = b["ids"].shape
    d = m._desc(B, S, "infer").desc
    ids, seg, pos, mask = m._inputs(b["ids"], b["seg"])
    base, alpha = torch.zeros_like(ids), torch.ones(B, device=DEV)
    cls = torch.empty(B, cfg.hidden_size, dtype=torch.bfloat16, device=DEV)
    attn = torch.empty(cfg.num_hidden_layers, B, cfg.num_attention_heads, S, device=DEV) if with_attn else None
    for fields in ((base, alpha), (base, None), (None, alpha)):
        d.base_ids, d.alpha = (None if t is None else t.data_ptr() for t in fields)
        with pytest.raises(RuntimeError, match="base_ids"):
            hb.encoder_infer(d, m.arena.weights, m.arena.p, ids, seg, pos, mask, m._infer_ws, cls, attn)
    d.base_ids = d.alpha = None


# ---- 3. nbest_embed_attrib -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["bert", "xlm-roberta"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [768, 200])
def test_embed_attrib(family, dtype, H):
    from nbest_amd import hipabi as hb
    pad = 1 if family == "xlm-roberta" else 0
    P, m, S = 3, 5, 29
    word, tt, pt, gam, bet = _tables(H, dtype=dtype, seed=9)
    x = _ids(family, P, S, pad, seed=4)
    base = default_baseline(x, pad)
    base[1, 3] = x[1, 3]                                          # x' = x inside a row: exactly 0
    ids, bids = x.repeat_interleave(m, 0).contiguous(), base.repeat_interleave(m, 0).contiguous()
    seg = (torch.arange(S, device=DEV) % 3 == 0).long().unsqueeze(0).expand(P * m, S).contiguous() if family == "bert" else None
    pos = _pos(family, ids, pad)
    alpha = ((torch.arange(m, device=DEV, dtype=torch.float64) + 0.5) / m).repeat(P).float()
    dh = _rnd(P * m * S, H, dtype=dtype, s=0.3, seed=11)
    A = hb.embed_attrib(ids, bids, alpha, seg, pos, word, tt, pt, gam, dh, P, m, S, 1e-12)
    A2 = hb.embed_attrib(ids, bids, alpha, seg, pos, word, tt, pt, gam, dh, P, m, S, 1e-12)
    torch.cuda.synchronize()
    assert torch.equal(A, A2), "two runs differ"
    W, T, Pt, G = word.double(), tt.double(), pt.double(), gam.double()
    a = alpha.double()[:, None, None]
    E = ((1 - a) * W[bids] + a * W[ids]) + (T[seg] if seg is not None else T[0]) + Pt[pos]
    E.requires_grad_(True)
    mu, var = E.mean(-1, keepdim=True), E.var(-1, unbiased=False, keepdim=True)
    y = (E - mu) / torch.sqrt(var + 1e-12) * G
    gE, = torch.autograd.grad((y * dh.double().view(P * m, S, H)).sum(), E)
    ref = (gE * (W[ids] - W[bids])).sum(-1).view(P, m, S).mean(1)
    zero = (x == base)
    assert torch.all(A[zero] == 0), "pads / x' = x tokens must be exactly 0"
    err = (A.double() - ref).abs().max().item()
    tol = 1e-5 if dtype == torch.float32 else 2e-3
    assert err <= tol * ref.abs().max().item(), "embed_attrib vs fp64: %.3e (max %.3e)" % (err, ref.abs().max().item())


# ---- 4. attribute against the fp64 oracle IG -------------------------------------------------------------------------------------
def _hip_model(meta, labels, dtype):
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    _, ocfg, cfg, sd, batch = oracle_model(meta, labels)
    m = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=dtype, dropout=0.0, seed=1)
    m.load_reference_state(sd)
    m.eval()
    return m, cfg, batch


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2", "bert_L12"])
def test_attribute_matches_oracle_fp32(name, labels):
    meta, _ = load_case(name)
    om, ocfg, cfg, _, batch = oracle_model(meta, labels)
    m, _, _ = _hip_model(meta, labels, torch.float32)
    ids = torch.from_numpy(batch["ids"])
    seg = torch.from_numpy(batch["seg"]) if meta["seg"] else None
    steps = 8
    pr = m.predict(ids.to(DEV), None if seg is None else seg.to(DEV))
    dec = [(b, c) for b, row in enumerate(pr["pred"].cpu().tolist()) for c in row if c >= 0]
    g = torch.Generator().manual_seed(1)
    tg = dec + [(b, int(torch.randint(0, labels.n_bottom, (1,), generator=g))) for b in range(ids.shape[0])]
    out = m.attribute(ids.to(DEV), None if seg is None else seg.to(DEV), targets=tg, steps=steps)
    torch.cuda.synchronize()
    base = default_baseline(ids, cfg.pad_token_id)
    A, sc, bs = oracle_ig(om, ocfg, ids, seg, base, tg, steps)
    got = out["attr"].double().cpu()
    for i, (b, c) in enumerate(tg):
        rel = (got[i] - A[i]).norm().item() / max(A[i].norm().item(), 1e-30)
        assert rel <= 1e-3, "%s pair (%d, %d): |A - A_ref| / |A_ref| = %.3e" % (name, b, c, rel)
        assert (got[i] - A[i]).abs().max().item() <= 1e-4 * A[i].abs().max().item() + 1e-9
        gap, gap_ref = got[i].sum().item() - (out["score"][i] - out["baseline_score"][i]).item(), A[i].sum().item() - (sc[i] - bs[i]).item()
        assert abs(gap - gap_ref) <= 1e-3 * max(abs((sc[i] - bs[i]).item()), 1e-6) + 1e-5, (gap, gap_ref)
    fin = pr["final"].cpu()
    for i, (b, c) in enumerate(tg):
        assert abs(out["score"][i].item() - fin[b, c].item()) <= 1e-6 + 1e-5 * abs(fin[b, c].item())


# ---- 4b. bf16: against the fp64 oracle, bar = 2 x the floor of a bf16-storage IG leg --------------------------------------------
def _segments(row, cfg):
    """token spans of a synthetic n-best row ([CLS] | sys .. [SEP] | hyp .. [SEP] | ...): a separator closes its segment"""
    out, lo = [(0, 1)], 1
    for t in range(1, len(row)):
        if int(row[t]) == cfg.sep_token_id:
            out.append((lo, t + 1))
            lo = t + 1
    return out


def _bf16_leg_ig(om, ocfg, ids, seg, base, targets, steps):
    """IG of the bf16-storage leg (oracle/bf16sim.py's rounding points), starting from the interpolated embedding: tables rounded to
    bf16, the lerp and the embedding LayerNorm in fp32, X0 and every stored activation (and its gradient) rounded as bf16sim.encode
    rounds them, heads in fp32; the gradient reaching the LayerNorm is the rounded one, as the HIP backward stores dhidden in bf16"""
    import math
    import torch.nn.functional as F
    from oracle import bf16sim as bs
    from oracle.encoder import position_ids_for
    enc = om.bert_encoder
    emb = enc.embeddings
    s0 = torch.zeros_like(ids) if (seg is None or ocfg.family == "xlm-roberta") else seg
    pos = position_ids_for(ocfg, ids)
    W = bs._r(emb.word_embeddings.weight.detach())
    T = bs._r(emb.token_type_embeddings.weight.detach())[s0]
    Pp = bs._r(emb.position_embeddings.weight.detach())[pos]
    a = ((torch.arange(steps, dtype=torch.float64) + 0.5) / steps).float()[:, None, None]
    H, nh = ocfg.hidden_size, ocfg.num_attention_heads
    d = H // nh
    out = []
    for b, c in targets:
        wx, wb = W[ids[b]], W[base[b]]
        E = (((1 - a) * wb + a * wx) + T[b]) + Pp[b]
        E.requires_grad_(True)
        km = ids[b].expand(steps, -1) > 0
        x = bs.ract(bs._ln(E, emb.LayerNorm))
        n, S = x.shape[0], x.shape[1]
        split = lambda t: t.view(n, S, nh, d).transpose(1, 2)
        for lyr in enc.encoder.layer:
            sa, ao = lyr.attention.self, lyr.attention.output
            q, k, v = (bs.ract(F.linear(x, bs.rw(mm.weight), mm.bias)) for mm in (sa.query, sa.key, sa.value))
            ctx = bs.ract(bs._AttnCore.apply(split(q), split(k), split(v), km, 1.0 / math.sqrt(d)).transpose(1, 2).reshape(n, S, H))
            r1 = bs.ract(F.linear(ctx, bs.rw(ao.dense.weight), ao.dense.bias) + x)
            x1 = bs.ract(bs._ln(r1, ao.LayerNorm))
            hact = bs._GeluStore.apply(F.linear(x1, bs.rw(lyr.intermediate.dense.weight), lyr.intermediate.dense.bias), True)
            r2 = bs.ract(F.linear(hact, bs.rw(lyr.output.dense.weight), lyr.output.dense.bias) + x1)
            x = bs.ract(bs._ln(r2, lyr.output.LayerNorm))
        f = om.clf(x[:, 0, :])[2][:, c]
        g, = torch.autograd.grad(f.sum(), E)
        out.append((g * (wx - wb)).sum(-1).mean(0).double())
    return torch.stack(out)


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2", "bert_L12"])
def test_attribute_matches_oracle_bf16(name, labels):
    """bf16 attribute() against the fp64 oracle IG: per pair ||A - A_ref|| / ||A_ref||, and every segment mass, within 2 x the floor of a
    bf16-storage IG leg - the maximum over five draws (the weights as they are, and four copies jittered by 2^-12 relative, as
    make_golden.py draws the bf16 floors)"""
    meta, _ = load_case(name)
    om64, ocfg, cfg, _, batch = oracle_model(meta, labels)
    om32 = oracle_model(meta, labels, dtype=torch.float32)[0]
    m, _, _ = _hip_model(meta, labels, torch.bfloat16)
    ids = torch.from_numpy(batch["ids"])
    seg = torch.from_numpy(batch["seg"]) if meta["seg"] else None
    steps = 8
    pr = m.predict(ids.to(DEV), None if seg is None else seg.to(DEV))
    dec = [(b, c) for b, row in enumerate(pr["pred"].cpu().tolist()) for c in row if c >= 0]
    g = torch.Generator().manual_seed(2)
    tg = dec + [(b, int(torch.randint(0, labels.n_bottom, (1,), generator=g))) for b in range(ids.shape[0])]
    out = m.attribute(ids.to(DEV), None if seg is None else seg.to(DEV), targets=tg, steps=steps)
    torch.cuda.synchronize()
    base = default_baseline(ids, cfg.pad_token_id)
    A_ref = oracle_ig(om64, ocfg, ids, seg, base, tg, steps)[0]
    segs = [_segments(ids[b], cfg) for b, _ in tg]
    mass = lambda A, i: torch.tensor([float(A[i][lo:hi].sum()) for lo, hi in segs[i]], dtype=torch.float64)
    rel_floor = torch.zeros(len(tg), dtype=torch.float64)
    mass_floor = torch.zeros(len(tg), dtype=torch.float64)
    params = list(om32.parameters())
    saved = [p.detach().clone() for p in params]
    for draw in range(5):
        if draw:
            gj = torch.Generator().manual_seed(1000003 * meta["seed"] + draw)
            with torch.no_grad():
                for p, q in zip(params, saved):
                    p.copy_(q * (1.0 + 2.0 ** -12 * (2.0 * torch.rand(q.shape, generator=gj) - 1.0)))
        A_leg = _bf16_leg_ig(om32, ocfg, ids, seg, base, tg, steps)
        for i in range(len(tg)):
            rel = (A_leg[i] - A_ref[i]).norm().item() / max(A_ref[i].norm().item(), 1e-30)
            rel_floor[i] = max(rel_floor[i].item(), rel)
            mass_floor[i] = max(mass_floor[i].item(), (mass(A_leg, i) - mass(A_ref, i)).abs().max().item())
    with torch.no_grad():
        for p, q in zip(params, saved):
            p.copy_(q)
    got = out["attr"].double().cpu()
    worst_rel = worst_mass = 0.0
    for i, (b, c) in enumerate(tg):
        rel = (got[i] - A_ref[i]).norm().item() / max(A_ref[i].norm().item(), 1e-30)
        dm = (mass(got, i) - mass(A_ref, i)).abs().max().item()
        worst_rel = max(worst_rel, rel / max(rel_floor[i].item(), 1e-30))
        worst_mass = max(worst_mass, dm / max(mass_floor[i].item(), 1e-30))
        assert rel <= 2.0 * rel_floor[i].item(), "%s pair (%d, %d): |A - A_ref| / |A_ref| = %.3e > 2 x floor %.3e" % (
            name, b, c, rel, rel_floor[i].item())
        assert dm <= 2.0 * mass_floor[i].item(), "%s pair (%d, %d): segment mass error %.3e > 2 x floor %.3e" % (
            name, b, c, dm, mass_floor[i].item())
    fin = pr["final"].cpu()
    sdiff = max(abs(out["score"][i].item() - fin[b, c].item()) for i, (b, c) in enumerate(tg))
    print("bf16 %s: %d pairs, HIP / floor: attr %.2f, mass %.2f (worst); |score - predict final| %.2e"
          % (name, len(tg), worst_rel, worst_mass, sdiff))
    assert sdiff <= 2e-3, "score differs from predict's final by %.3e" % sdiff


# ---- 5. chunking, state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attribute_chunking(dtype, labels):
    meta, _ = load_case("bert_L2")
    m, cfg, batch = _hip_model(meta, labels, dtype)
    ids, seg = torch.from_numpy(batch["ids"]).to(DEV), torch.from_numpy(batch["seg"]).to(DEV)
    tg = [(b, c) for b in range(ids.shape[0]) for c in (0, 3, 7)]
    steps = 6
    a = m.attribute(ids, seg, targets=tg, steps=steps)
    b = m.attribute(ids, seg, targets=tg, steps=steps, max_rows=steps + 2)
    torch.cuda.synchronize()
    for k in ("attr", "score", "baseline_score"):
        d = (a[k] - b[k]).abs().max().item()
        assert d <= 1e-6 * max(a[k].abs().max().item(), 1e-30), "%s differs between chunkings: %.3e" % (k, d)
    print("chunking %s: attr bit-identical %s, score bit-identical %s, baseline_score bit-identical %s"
          % (dtype, torch.equal(a["attr"], b["attr"]), torch.equal(a["score"], b["score"]), torch.equal(a["baseline_score"], b["baseline_score"])))


def test_attribute_steps_beyond_max_rows(labels):
    """a pair's m + 2 rows larger than max_rows run as one call of their own (any steps >= 1; --attribution_steps has no upper
    limit): m = 300 with the default max_rows = 256 is complete to the Riemann error and agrees with an explicit max_rows"""
    meta, _ = load_case("bert_L2")
    m, cfg, batch = _hip_model(meta, labels, torch.float32)
    ids, seg = torch.from_numpy(batch["ids"]).to(DEV), torch.from_numpy(batch["seg"]).to(DEV)
    tg = [(0, 3), (1, 7), (1, 2)]
    a = m.attribute(ids, seg, targets=tg, steps=300)
    b = m.attribute(ids, seg, targets=tg, steps=300, max_rows=2000)
    torch.cuda.synchronize()
    for k in ("attr", "score", "baseline_score"):
        assert (a[k] - b[k]).abs().max().item() <= 1e-6 * max(b[k].abs().max().item(), 1e-30), k
    for i in range(len(tg)):
        dF = (a["score"][i] - a["baseline_score"][i]).item()
        assert abs(a["attr"][i].sum().item() - dF) <= 1e-3 * abs(dF) + 1e-5, (tg[i], a["attr"][i].sum().item(), dF)


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8w"])
def test_attribute_leaves_training_state_alone(mode, labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, dtype=torch.float32 if mode == "f32" else torch.bfloat16, fp8=mode == "fp8w")
    m.train()
    b = _batch(cfg, labels, 4, 48)
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    for _ in range(2):
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        opt.step()
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    torch.cuda.synchronize()
    before = _state(m)
    m.attribute(b["ids"], seg_ids=b["seg"], targets=[(0, 1), (2, 4)], steps=4)
    torch.cuda.synchronize()
    after = _state(m)
    after["stash"].pop("attrib", None)
    _same_state(before, after)


def test_attribute_between_bridge_forward_and_backward(labels):
    outs = []
    for with_attr in (False, True):
        m, cfg, _ = _model(labels, dtype=torch.float32)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        m.zero_grad()
        top, bottoms, fin, asr_cls, _ = m(None, b["ids"], seg_ids=b["seg"])
        if with_attr:
            m.attribute(b["ids"], seg_ids=b["seg"], targets=[(1, 2)], steps=3)
        (fin.sum() + 0.5 * top.sum() + 0.1 * asr_cls.sum()).backward()
        torch.cuda.synchronize()
        outs.append(m.arena.g.clone())
    assert torch.equal(outs[0], outs[1]), "gradients differ when attribute() runs between forward() and backward()"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_after_attribute_is_unchanged(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_attr in (False, True):
        m, cfg, _ = _model(labels, dtype=dtype)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_attr:
            m.attribute(b["ids"], seg_ids=b["seg"], targets=[(0, 0), (3, 5)], steps=4)
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after attribute() differs"


# ---- 6. --predict_attribution end to end ----------------------------------------------------------------------------------------------
def test_cli_predict_attribution(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    # a few epochs at a high learning rate: the model must predict labels for the records to hold anything
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--lr", "1e-3", "--bert_lr", "1e-4", "--batchSize", "16", "--max_epoch", "4", "--experiment", exp,
              "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", "f32",
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "3", "--resume"]
    assert cli.main(common) == 0
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    plain, with_attr, attr = str(tmp_path / "a.pred"), str(tmp_path / "b.pred"), str(tmp_path / "b.ig.jsonl")
    both, attn2, attr2 = str(tmp_path / "c.pred"), str(tmp_path / "c.attn.jsonl"), str(tmp_path / "c.ig.jsonl")
    assert cli.main(common + ["--predict", src, "--predict_output", plain]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", with_attr, "--predict_attribution", attr, "--attribution_steps", "32"]) == 0
    # 256 steps: one pair's rows exceed the default max_rows (256) - the run must still go through
    assert cli.main(common + ["--predict", src, "--predict_output", both, "--predict_attention", attn2, "--predict_attribution", attr2,
                              "--attribution_steps", "256"]) == 0
    ref = open(plain, "rb").read()
    assert open(with_attr, "rb").read() == ref and open(both, "rb").read() == ref, ".pred differs with --predict_attribution"
    preds = [l.split("\t<=>\t")[1] for l in open(plain).read().split("\n")[:-1]]
    n_in = len(open(src).read().strip("\n").split("\n"))
    attn = [json.loads(l) for l in open(attn2).read().strip("\n").split("\n")]
    assert len(preds) == n_in
    for path, steps, tol in ((attr, 32, 2e-2), (attr2, 256, 2e-3)):
        recs = [json.loads(l) for l in open(path).read().strip("\n").split("\n")]
        assert [r["line"] for r in recs] == list(range(1, n_in + 1))
        n_labels = 0
        for r, a, p in zip(recs, attn, preds):
            assert r["segments"] == a["segments"] and r["tokens"] == a["tokens"] and r["steps"] == steps
            assert [l["label"] for l in r["labels"]] == ([x for x in p.split(";")] if p else [])
            for l in r["labels"]:
                n_labels += 1
                assert len(l["token_attr"]) == sum(r["tokens"]) and len(l["mass"]) == len(r["segments"])
                dF = l["score"] - l["baseline_score"]
                assert abs(sum(l["mass"]) - dF) <= tol * abs(dF) + 2e-4, (steps, r["line"], l["label"], sum(l["mass"]), dF)
        assert n_labels > 0, "no utterance has a predicted label: the test checks nothing"
