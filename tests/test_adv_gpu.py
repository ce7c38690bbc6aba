"""GPU: FGM adversarial training on the word embeddings.  The three new entry points (nbest_embed_ln_fwd_adv, nbest_embed_ln_bwd_adv,
nbest_embed_adv_delta) against torch, their zero-delta / repeat / accumulate identities, forward_backward(adv=) on whole models against
the fp64 restatement of tests/test_adv_cpu.py (fp32 at the gradient bars of tests/test_rdrop_gpu.py, bf16 against the floor of a
bf16-storage leg), the epsilon = 0 identity under dropout, the untouched path without the argument, the refusals, train_step and the
command line."""
import ctypes as C
import os
import re
import shutil

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_case, case_inputs
from test_adv_cpu import fgm_reference
from test_kernels_gpu import close, rnd, tol_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
B_, S_, V_ = 5, 37, 400
LENS = [1, 37, 20, 9, 30]           # ragged right padding, row 0 the shortest: [CLS] and nothing but padding after it
NAMES = ("dword", "dtype", "dpos", "dgamma", "dbeta")


def _hb():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi
    return hipabi


def _emb_problem(H, dtype, roberta):
    """B 5, S 37 (more than one block of 4 rows, S odd), ragged; BERT: pad id 0, arange positions, two token types; RoBERTa: pad id 1,
    pad-offset positions, no segments.  Returns a dict; ``mask`` is the key mask (non-padding tokens)."""
    pad = 1 if roberta else 0
    g = torch.Generator().manual_seed(17 + H)
    ids = torch.randint(4, V_, (B_, S_), generator=g)
    ids[:, 0] = 2
    ids[:, 5::7] = 3                                              # [SEP]-like: a run of equal ids across chunks of the sorted order
    for b, n in enumerate(LENS):
        ids[b, n:] = pad
    ids = ids.to(DEV)
    if roberta:
        nonpad = ids.ne(pad).long()
        pos = (torch.cumsum(nonpad, dim=1) * nonpad + pad).contiguous()
        seg, n_types, pos_pad = None, 1, pad
    else:
        pos = torch.arange(S_)[None, :].expand(B_, S_).contiguous().to(DEV)
        seg = (torch.arange(S_)[None, :] > 11).long().expand(B_, S_).contiguous().to(DEV)
        n_types, pos_pad = 2, -1
    p = dict(ids=ids, seg=seg, pos=pos, pad=pad, pos_pad=pos_pad, mask=ids.ne(pad).to(torch.uint8).contiguous(),
             word=rnd(V_, H, dtype=dtype, s=0.5, seed=71), tt=rnd(n_types, H, dtype=dtype, s=0.5, seed=72),
             pt=rnd(S_ + 2, H, dtype=dtype, s=0.5, seed=73), gam=1 + 0.1 * rnd(H, seed=74), bet=0.1 * rnd(H, seed=75),
             delta=rnd(B_ * S_, H, s=0.05, seed=76), dout=rnd(B_ * S_, H, dtype=dtype, seed=77), eps=1e-5 if roberta else 1e-12)
    return p


def _esum(p, wr, tr, pr, delta=None):
    """the embedding sum in torch fp32 from float copies of the stored tables (the word row plus delta first, as the kernels add)"""
    w = F.embedding(p["ids"], wr, padding_idx=p["pad"])
    if delta is not None:
        w = w + delta.view(B_, S_, -1)
    t = tr[p["seg"]] if p["seg"] is not None else tr[0]
    return w + t + F.embedding(p["pos"], pr, padding_idx=p["pos_pad"] if p["pos_pad"] >= 0 else None)


KERNEL_CASES = [(H, dtype, roberta) for H in (768, 1024, 320) for dtype in (torch.float32, torch.bfloat16) for roberta in (False, True)]
KERNEL_IDS = ["H%d-%s-%s" % (H, str(d)[6:], "roberta" if r else "bert") for H, d, r in KERNEL_CASES]


@pytest.mark.parametrize("H,dtype,roberta", KERNEL_CASES, ids=KERNEL_IDS)
def test_embed_fwd_bwd_with_delta(H, dtype, roberta):
    """forward: against layer_norm(word[ids] + delta + type + pos) from the same stored tables at tol_of(dtype); a zero delta gives
    the plain forward's output and stats bit for bit (dropout off and on).  backward: against torch autograd at 5 tol_of(dtype);
    a zero delta gives the plain backward's five outputs bit for bit; two runs give the same bits; accumulation gives one + one"""
    hb = _hb()
    p = _emb_problem(H, dtype, roberta)
    a = (p["ids"], p["seg"], p["pos"], p["word"], p["tt"], p["pt"], p["gam"])
    fwd = lambda delta=None, **kw: hb.embed_ln_fwd(*a, p["bet"], p["eps"], delta=delta, **kw)
    out, stats = fwd(p["delta"])
    wr, tr, pr = (t.float().clone().requires_grad_(True) for t in (p["word"], p["tt"], p["pt"]))
    gr, br = p["gam"].clone().requires_grad_(True), p["bet"].clone().requires_grad_(True)
    ref = F.layer_norm(_esum(p, wr, tr, pr, p["delta"]), (H,), gr, br, p["eps"]).reshape(B_ * S_, H)
    tol = tol_of(dtype)
    close("embed_fwd_adv", out, ref, tol)
    zero = torch.zeros_like(p["delta"])
    plain, pstats = fwd()
    out0, stats0 = fwd(zero)
    assert not torch.equal(out, plain)
    assert torch.equal(out0, plain) and torch.equal(stats0, pstats), "a zero delta changes the forward's bits"
    kw = dict(drop_p=0.1, seed=11, drop_stream=3)
    dz, dp = fwd(zero, **kw), fwd(**kw)
    assert torch.equal(dz[0], dp[0]) and torch.equal(dz[1], dp[1]) and not torch.equal(dp[0], plain)
    # backward
    ref.backward(p["dout"].float())
    bwd = lambda st, delta=None, **kw: hb.embed_ln_bwd(*a, st, p["dout"], B_, S_, word_pad_id=p["pad"], pos_pad_id=p["pos_pad"], delta=delta, **kw)
    got = bwd(stats, p["delta"])
    for n, x, want in zip(NAMES, got, (wr.grad, tr.grad, pr.grad, gr.grad, br.grad)):
        close("embed_bwd_adv %s" % n, x, want, 5 * tol)
    assert got[0][p["pad"]].abs().max().item() == 0.0
    for n, x, y in zip(NAMES, got, bwd(stats, p["delta"])):
        assert torch.equal(x, y), "embed_bwd_adv %s is not bit-reproducible" % n
    for n, x, y in zip(NAMES, bwd(pstats, zero), bwd(pstats)):
        assert torch.equal(x, y), "a zero delta changes the bits of embed_bwd %s" % n
    acc = bwd(stats, p["delta"], accumulate_into=tuple(t.clone() for t in got))
    for n, x, one in zip(NAMES, acc, got):
        assert torch.equal(x, one + one), "accumulate: %s != 2 x the single pass" % n


@pytest.mark.parametrize("H,dtype,roberta", KERNEL_CASES, ids=KERNEL_IDS)
def test_embed_adv_delta(H, dtype, roberta):
    """dropout 0: g = delta norm / epsilon against torch.autograd.grad w.r.t. the embedding sum at 5 tol_of(dtype), norm at the same
    relative bar, | ||delta_b|| - epsilon | <= 1e-5 epsilon, padding rows exactly 0, an utterance whose dout is zero gets a zero delta
    and norm 0 without NaN, two runs give the same bits.  dropout 0.1: the call equals the dropout-0 call on a dout masked with the
    forward's keep bits (read off the forward's zeros) - fp32: masked and scaled by the kernel's fp32 scale, bit for bit; bf16 (where
    the scaled dout has no bf16 representation): masked only, g being linear in dout the scale cancels in delta and multiplies norm,
    both to 1e-5 (fp32 arithmetic, one multiplication moved)"""
    hb = _hb()
    p = _emb_problem(H, dtype, roberta)
    epsilon = 1.5
    dout = p["dout"].clone()
    dout.view(B_, S_, H)[2] = 0                                      # an utterance without gradient
    a = (p["ids"], p["seg"], p["pos"], p["mask"], p["word"], p["tt"], p["pt"], p["gam"])
    run = lambda d, **kw: hb.embed_adv_delta(*a, d, B_, S_, p["eps"], epsilon, **kw)
    delta, norm = run(dout)
    d2, n2 = run(dout)
    torch.cuda.synchronize()
    assert torch.equal(delta, d2) and torch.equal(norm, n2), "embed_adv_delta is not bit-reproducible"
    assert bool(torch.isfinite(delta).all()) and bool(torch.isfinite(norm).all())
    E = _esum(p, p["word"].float(), p["tt"].float(), p["pt"].float()).requires_grad_(True)
    y = F.layer_norm(E, (H,), p["gam"], p["bet"], p["eps"])
    g_ref, = torch.autograd.grad(y, E, dout.float().view(B_, S_, H))
    keep = p["mask"].bool().view(B_, S_, 1)
    g_ref = g_ref * keep
    n_ref = g_ref.flatten(1).norm(dim=1)
    tol = 5 * tol_of(dtype)
    dv = delta.view(B_, S_, H)
    close("embed_adv_delta g", dv * (norm / epsilon).view(B_, 1, 1), g_ref, tol)
    live = [b for b in range(B_) if b != 2]
    assert ((norm[live] - n_ref[live]).abs() <= tol * n_ref[live]).all(), (norm, n_ref)
    assert ((dv[live].double().flatten(1).norm(dim=1) - epsilon).abs() <= 1e-5 * epsilon).all()
    assert dv.masked_select(~keep.expand(B_, S_, H)).abs().max().item() == 0.0, "a padding row is perturbed"
    assert dv[2].abs().max().item() == 0.0 and norm[2].item() == 0.0
    # epsilon 0: zeros, the norm unchanged
    z, nz = hb.embed_adv_delta(*a, dout, B_, S_, p["eps"], 0.0)
    assert z.abs().max().item() == 0.0 and torch.equal(nz, norm)
    # dropout 0.1
    kw = dict(drop_p=0.1, seed=29, drop_stream=1000)
    clean, _ = hb.embed_ln_fwd(p["ids"], p["seg"], p["pos"], p["word"], p["tt"], p["pt"], p["gam"], p["bet"], p["eps"])
    dropped, _ = hb.embed_ln_fwd(p["ids"], p["seg"], p["pos"], p["word"], p["tt"], p["pt"], p["gam"], p["bet"], p["eps"], **kw)
    assert bool((clean != 0).all()), "the forward's output has a zero of its own"
    bits = dropped != 0
    frac = 1.0 - bits.float().mean().item()
    assert 0.07 < frac < 0.13, frac
    dd, dn = run(dout, **kw)
    if dtype == torch.float32:
        scale = (torch.tensor(65536.0) / torch.tensor(65536.0 - 6554.0)).item()       # common.h make_drop: thr = lrint(0.1 x 65536)
        md, mn = run(torch.where(bits, dout * torch.tensor(scale, device=DEV), torch.zeros_like(dout)))
        assert torch.equal(dd, md) and torch.equal(dn, mn), "dropout: not the dropout-0 call on the masked, scaled dout"
    else:
        md, mn = run(torch.where(bits, dout, torch.zeros_like(dout)))
        assert (dd - md).abs().max().item() <= 1e-5 * md.abs().max().item()
        assert ((dn - mn * (65536.0 / 58982.0)).abs() <= 1e-5 * dn).all()
    assert not torch.equal(dd, delta)


# ---- whole model ---------------------------------------------------------------------------------------------------------------------
def _step(m, b, meta, **kw):
    return m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                              trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"], **kw)


def _reference(meta, labels, epsilon):
    from test_model_gpu import _oracle_for
    cfg, sd, batch = case_inputs(meta, labels)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    return om, t, fgm_reference(om, t, epsilon, labels.top2bottom, seg=meta["seg"], add_l2=meta["add_l2"])


_REF = {}


def _shared_reference(name, labels, epsilon=1.0):
    """the fp64 reference of a case, computed once and shared by the fp32 and the bf16 test (nobody modifies it)"""
    if name not in _REF:
        meta, _ = load_case(name)
        _REF[name] = (meta,) + _reference(meta, labels, epsilon)
    return _REF[name]


@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_whole_model_fp32_matches_the_fgm_reference(name, labels):
    """fp32, dropout 0, epsilon 1: the arena gradients of forward_backward(adv=) against fgm_reference at the bars of
    tests/test_rdrop_gpu.py::test_whole_model_fp32_matches_the_oracle_under_autograd (noise-to-signal 2e-3 per tensor, the STC heads as
    one fused matrix, key bias skipped); both losses 1e-4 relative, adv_norm 1e-3 relative; the perturbed loss is the larger one; two
    runs give the same bits"""
    from test_model_gpu import _build
    meta, om, t, ref = _shared_reference(name, labels)
    m, b = _build(meta, labels, torch.float32)
    runs = []
    for _ in range(2):
        out = _step(m, b, meta, adv=dict(epsilon=1.0))
        torch.cuda.synchronize()
        runs.append(m.arena.g.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "the FGM step is not bit-reproducible"
    lp, alp = out["loss_parts"].double().cpu(), out["adv_loss_parts"].double().cpu()
    hard, adv, mse = ref["loss_parts"][:3].sum().item(), ref["adv_loss_parts"].sum().item(), ref["loss_parts"][3].item()
    print("forward_backward(adv=) %s fp32: hard loss %.6f vs %.6f, perturbed %.6f vs %.6f, mse %.6f vs %.6f" % (
        name, lp[:3].sum(), hard, alp[:3].sum(), adv, lp[3], mse))
    assert abs(lp[:3].sum().item() - hard) <= 1e-4 * hard and abs(alp[:3].sum().item() - adv) <= 1e-4 * adv
    assert abs(lp[3].item() - mse) <= 1e-4 * mse and alp[3].item() == 0.0
    assert alp[:3].sum().item() > lp[:3].sum().item()
    norm = out["adv_norm"].double().cpu()
    assert norm.shape == ref["norm"].shape and ((norm - ref["norm"]).abs() <= 1e-3 * ref["norm"]).all(), (norm, ref["norm"])
    named, ref_g = dict(m.named_parameters()), ref["grads"]
    fused = lambda n: n.startswith("clf.") and (n.endswith(".weight") or n.endswith(".bias"))
    worst = (0.0, "")
    for kind in (".weight", ".bias"):
        names = [n for n in ref_g if fused(n) and n.endswith(kind)]
        num = sum((named[n].grad.double().cpu() - ref_g[n]).pow(2).sum().item() for n in names) ** 0.5
        den = sum(ref_g[n].pow(2).sum().item() for n in names) ** 0.5
        worst = max(worst, (num / den, "clf fused " + kind))
        assert num <= 2e-3 * den, (kind, num / den)
    for n, g_ref in ref_g.items():
        if n.endswith("attention.self.key.bias") or fused(n):          # (softmax is invariant to a key bias: both sides are noise)
            continue
        ns = ((named[n].grad.double().cpu() - g_ref).norm() / g_ref.norm().clamp_min(1e-30)).item()
        worst = max(worst, (ns, n))
        assert ns <= 2e-3, (n, ns)
    print("forward_backward(adv=) %s fp32: worst gradient noise-to-signal %.3e (%s), bar 2e-3" % ((name,) + worst))
    # not the clean gradient doubled: the second pass ran somewhere else
    n = "bert_encoder.embeddings.word_embeddings.weight"
    assert (ref_g[n] - 2 * ref["clean_grads"][n]).norm().item() > 1e-2 * ref_g[n].norm().item()


def _bf16_leg_delta(om, batch, meta, labels, epsilon):
    """delta of the bf16-storage leg (oracle/bf16sim.py's rounding points) starting from the embedding sum, as
    tests/test_attrib_gpu.py::_bf16_leg_ig with the step's loss in place of the score: tables rounded to bf16, the sum and the embedding
    LayerNorm in fp32, X0 and every stored activation (and its gradient) rounded as bf16sim.encode rounds them, heads and losses in
    fp32; the transcript pass (its CLS rows enter the MSE) runs bf16sim.encode.  Returns delta [B, S, H] fp64."""
    import math
    from oracle import bf16sim as bs, stc
    from oracle.encoder import position_ids_for
    enc, ocfg = om.bert_encoder, om.bert_encoder.cfg
    emb = enc.embeddings
    ids = batch["ids"]
    xl = ocfg.family == "xlm-roberta"
    seg = None if (xl or not meta["seg"]) else batch["seg"]
    s0 = torch.zeros_like(ids) if seg is None else seg
    pos = position_ids_for(ocfg, ids)
    E = (bs._r(emb.word_embeddings.weight.detach())[ids] + bs._r(emb.token_type_embeddings.weight.detach())[s0]) + \
        bs._r(emb.position_embeddings.weight.detach())[pos]
    E.requires_grad_(True)
    km = ids > 0
    H, nh = ocfg.hidden_size, ocfg.num_attention_heads
    d = H // nh
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
    asr, tr = x[:, 0, :], None
    if meta["add_l2"]:
        with torch.no_grad():
            tr = bs.encode(enc, batch["tids"], None if xl else batch["tseg"])
    top, bottoms, final = om.clf(asr)
    _, total, _ = stc.total_loss(top, bottoms, final, batch["labels"].float(), labels.top2bottom, stc.bottom2top_matrix(labels.top2bottom),
                                 asr, tr, meta["add_l2"])
    g, = torch.autograd.grad(total, E)
    g = g.double() * (ids > 0).unsqueeze(-1)
    return g * (epsilon / g.flatten(1).norm(dim=1)).view(-1, 1, 1)


@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_whole_model_bf16_within_the_storage_floor(name, labels):
    """bf16, dropout 0, epsilon 1: per utterance ||delta - delta_ref|| / epsilon against the fp64 reference, within 2 x the floor of a
    bf16-storage leg that starts from the embedding sum - the maximum over five draws (the weights as they are and four copies
    jittered by 2^-12 relative, as tests/test_attrib_gpu.py draws its floors).  Also | ||delta_b|| - epsilon | <= 1e-5 epsilon and the
    perturbed loss above the clean one."""
    from test_model_gpu import _build, _oracle_for
    meta, om64, t, ref = _shared_reference(name, labels)
    eps = 1.0
    cfg, sd, _ = case_inputs(meta, labels)
    om32 = _oracle_for(cfg, sd, labels)
    B = t["ids"].shape[0]
    dref = ref["delta"]
    floor = torch.zeros(B, dtype=torch.float64)
    params = list(om32.parameters())
    saved = [p.detach().clone() for p in params]
    for draw in range(5):
        if draw:
            gj = torch.Generator().manual_seed(1000003 * meta["seed"] + draw)
            with torch.no_grad():
                for p, q in zip(params, saved):
                    p.copy_(q * (1.0 + 2.0 ** -12 * (2.0 * torch.rand(q.shape, generator=gj) - 1.0)))
        leg = _bf16_leg_delta(om32, t, meta, labels, eps)
        floor = torch.maximum(floor, (leg - dref).flatten(1).norm(dim=1) / eps)
    m, b = _build(meta, labels, torch.bfloat16)
    out = _step(m, b, meta, adv=dict(epsilon=eps))
    torch.cuda.synchronize()
    S, H = t["ids"].shape[1], cfg.hidden_size
    delta = m._adv_delta[:B * S * H].view(B, S, H).double().cpu()
    err = (delta - dref).flatten(1).norm(dim=1) / eps
    ratio = (err / floor.clamp_min(1e-30)).max().item()
    print("forward_backward(adv=) %s bf16: ||delta - delta_ref|| / epsilon %s, floor %s, worst HIP / floor %.2f (bar 2)" % (
        name, ["%.3e" % v for v in err.tolist()], ["%.3e" % v for v in floor.tolist()], ratio))
    assert (err <= 2.0 * floor).all(), (err, floor)
    assert ((delta.flatten(1).norm(dim=1) - eps).abs() <= 1e-5 * eps).all()
    assert out["adv_loss_parts"][:3].sum().item() > out["loss_parts"][:3].sum().item()


def test_epsilon_zero_under_dropout_doubles_the_gradient(labels):
    """bf16, B 6, dropout 0.3 / 0.1, epsilon 0: the second pass runs under the same masks on a zero delta, so adv_loss_parts[:3] has
    the bits of loss_parts[:3], and every tensor of arena.g is within 1e-5 of its norm of twice the plain step's gradient (only the
    fp32 order of accumulating a second, equal contribution differs)"""
    from test_optim_adam_gpu import _batch, _model
    a, twin = _model(labels, torch.bfloat16, dropout=0.3), _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(a, labels, B=6)
    out = a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], adv=dict(epsilon=0.0))
    tout = twin.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    assert torch.equal(out["adv_loss_parts"][:3], out["loss_parts"][:3]) and out["adv_loss_parts"][3].item() == 0.0
    assert torch.equal(out["loss_parts"], tout["loss_parts"]) and torch.equal(out["top"], tout["top"])
    assert bool((out["adv_norm"] > 0).all())
    worst = (0.0, "")
    for (n, p), (_, q) in zip(a.named_parameters(), twin.named_parameters()):
        if p.grad is None:
            continue
        two = 2.0 * q.grad.double()
        r = ((p.grad.double() - two).norm() / two.norm().clamp_min(1e-300)).item()
        worst = max(worst, (r, n))
        assert r <= 1e-5, (n, r)
    print("epsilon 0 under dropout: worst |g - 2 g_plain| / |2 g_plain| = %.2e (%s)" % worst)
    assert a.step_counter == twin.step_counter == 1


def test_without_adv_nothing_changes(labels):
    """after a call with ``adv``, a plain forward_backward on that model and on a twin that never saw the argument give the same
    bits (arena.g, scores, loss_parts, step_counter), with and without the transcript pass; no descriptor keeps a delta pointer"""
    from test_optim_adam_gpu import _batch, _model
    a, twin = _model(labels, torch.bfloat16, dropout=0.3), _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(a, labels, B=6)
    kw = dict(seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    out = a.forward_backward(b["ids"], b["labels"], adv=dict(epsilon=1.0), **kw)
    tout = twin.forward_backward(b["ids"], b["labels"], **kw)
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(out[k], tout[k]), k                       # the clean pass's, MSE in slot 3
    assert out["adv_loss_parts"].shape == (4,) and out["adv_norm"].shape == (6,) and "adv_norm" not in tout
    assert not torch.equal(a.arena.g, twin.arena.g)
    assert all(ps.desc.emb_delta is None for ps in a._passes.values())
    for kwargs in (dict(seg_ids=b["seg"]), kw):
        o1, o2 = a.forward_backward(b["ids"], b["labels"], **kwargs), twin.forward_backward(b["ids"], b["labels"], **kwargs)
        torch.cuda.synchronize()
        assert torch.equal(a.arena.g.view(torch.int32), twin.arena.g.view(torch.int32))
        for k in ("top", "bott", "final", "loss_parts"):
            assert torch.equal(o1[k], o2[k]), k
        assert "adv_loss_parts" not in o1
    assert a.step_counter == twin.step_counter == 3


def test_refusals(labels):
    """an fp8 model, a head mask, frozen embeddings or lower layers (RuntimeError); need_grad=False, distill=, rdrop=, a negative or NaN
    epsilon (ValueError naming adv): step_counter and arena.g untouched.  The library refuses emb_delta with w8, base_ids and
    first_trainable > 0, and the inference entry points refuse it, before any pointer is looked at"""
    from test_optim_adam_gpu import _batch, _model
    adv = dict(epsilon=1.0)
    m = _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(m, labels, B=6)
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    g0, steps = m.arena.g.clone(), m.step_counter
    call = lambda mm=m, **kw: mm.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], **kw)
    distill = dict(logits=torch.zeros(6, m.dls.n_rows, device=DEV), alpha=0.5, temperature=2.0)
    for kw in (dict(adv=adv, need_grad=False), dict(adv=adv, distill=distill), dict(adv=adv, rdrop=dict(alpha=1.0)),
               dict(adv=dict(epsilon=-1.0)), dict(adv=dict(epsilon=float("nan")))):
        with pytest.raises(ValueError, match="adv"):
            call(**kw)
    m.set_head_mask(torch.ones(m.cfg.num_hidden_layers, m.cfg.num_attention_heads))
    with pytest.raises(RuntimeError, match="head mask"):
        call(adv=adv)
    m.set_head_mask(None)
    emb = [p for n, p in m.named_parameters() if n.startswith("bert_encoder.embeddings.")]
    for p in emb:
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="adv"):
        call(adv=adv)
    for p in emb + [p for n, p in m.named_parameters() if n.startswith("bert_encoder.encoder.layer.0.")]:
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="adv"):
        call(adv=adv)
    torch.cuda.synchronize()
    assert m.step_counter == steps and torch.equal(m.arena.g, g0)
    f8 = _model(labels, torch.bfloat16, fp8=True)
    g8 = f8.arena.g.clone()
    with pytest.raises(RuntimeError, match="adv"):
        call(f8, adv=adv)
    assert f8.step_counter == 0 and torch.equal(f8.arena.g, g8)
    # the library
    from test_wgrad_window_cpu import _lib, _desc, BERT
    hb, lib = _lib()
    lay = (hb.LayerOffsets * 4)()
    null, fake = C.c_void_p(), 1 << 20
    for field, word in ((dict(w8=fake, w8_inv_scale=fake), "fp8"), (dict(base_ids=fake, alpha=fake), "base_ids"), (dict(first_trainable=1), "first_trainable")):
        d = _desc(hb, 4, 3, 16, **BERT)
        d.layers_host = lay
        d.emb_delta = fake
        for k, v in field.items():
            setattr(d, k, v)
        calls = {
            "forward": lambda: lib.nbest_encoder_forward(C.byref(d), null, null, null, null, null, null, null, 0, null, 0, None, null),
            "backward": lambda: lib.nbest_encoder_backward(C.byref(d), null, null, null, null, null, null, null, null, null, 0, null, null, 0,
                                                           0, d.first_trainable, d.L, 0, null),
        }
        for what, fn in calls.items():
            rc = fn()
            msg = hb.last_error()
            assert rc < 0 and "emb_delta" in msg and word in msg, (what, rc, msg)
    d = _desc(hb, 4, 3, 16, **BERT)
    d.layers_host = lay
    d.emb_delta = fake
    d.hidden_drop = d.attn_drop = 0.0
    assert lib.nbest_encoder_infer(C.byref(d), null, null, null, null, null, null, null, 0, null, null) < 0 and "emb_delta" in hb.last_error()
    assert lib.nbest_encoder_infer_attn(C.byref(d), null, null, null, null, null, null, null, 0, null, null, null) < 0
    assert "emb_delta" in hb.last_error()


def test_train_step_with_adv(labels):
    """a 1-layer bf16 model, B 8, S 32, dropout 0.3 / 0.1, epsilon 1, 20 steps on one batch: the clean and the perturbed loss both
    fall and the optimizer stepped once per call"""
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import train_step
    from test_optim_adam_gpu import BERT_LR, LR, _batch, _model
    m = _model(labels, torch.bfloat16, layers=1, seed=34, dropout=0.3)
    opt = HipBertAdam(m, lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=40)
    b = _batch(m, labels, B=8, S=32)
    clean, adv = [], []
    for _ in range(21):
        out = train_step(m, opt, b, adv_epsilon=1.0)
        clean.append(out["loss_parts"].clone())
        adv.append(out["adv_loss_parts"].clone())
    torch.cuda.synchronize()
    clean = torch.stack(clean).double().cpu()[:, :3].sum(dim=1).tolist()
    adv = torch.stack(adv).double().cpu()[:, :3].sum(dim=1).tolist()
    print("train_step(adv_epsilon=1): clean loss %.4f -> %.4f, perturbed %.4f -> %.4f over 20 steps" % (clean[0], clean[20], adv[0], adv[20]))
    assert clean[20] < clean[0] and adv[20] < adv[0], (clean, adv)
    assert opt.step_count == 21 and m.step_counter == 21
    assert out["top"].shape[0] == 8 and out["adv_norm"].shape == (8,)
    with pytest.raises(ValueError, match="adv_epsilon"):
        train_step(m, opt, b, teacher=m, adv_epsilon=1.0)
    assert opt.step_count == 21


def test_cli_adv_epsilon(tmp_path):
    """one epoch on valid_head.txt with --adv_epsilon 1.0: the __fgm_1.0 directory, the log line and a parsable [Train] line exist;
    --testing is refused with the flag and, without it, reproduces the valid F1 line on a copy of model.pt in the plain-named directory"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    plain = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
             "--bert_dropout", "0.1", "--optim_choice", "bertadam", "--lr", "1e-2", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
             "--batchSize", "2", "--max_epoch", "1", "--experiment", str(tmp_path / "exp"), "--pre_trained_model", "bert",
             "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
             "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "1", "--n_best", "5"]
    args = plain + ["--adv_epsilon", "1.0", "--resume"]
    assert cli.main(args) == 0
    d = cli.exp_dir(cli.parse_arguments(args))
    assert d.endswith("__fgm_1.0") and os.path.isdir(d)
    pt = os.path.join(d, "model.pt")
    if not os.path.isfile(pt):         # written on a NEW BEST valid F1 only: otherwise the epoch's weights
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], pt)
    log = open(os.path.join(d, "log.train")).read().split("\n")
    assert sum(l.startswith("FGM: epsilon 1.0;") for l in log) == 1
    train = [l for l in log if l.startswith("[Train]\tEpoch: 00")]
    assert len(train) == 1
    loss, f1 = re.search(r"Loss: ([0-9.]+)\t\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)", train[0]).groups()
    assert 0.0 < float(loss) < 1e4 and 0.0 <= float(f1) <= 100.0
    valid = [l for l in log if l.startswith("[Valid]\tEpoch: 00")][0]
    f1, acc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", valid).groups()
    with pytest.raises(SystemExit):
        cli.main(args + ["--testing"])
    d_test = cli.exp_dir(cli.parse_arguments(plain))
    assert d_test != d and d == d_test + "__fgm_1.0"
    os.makedirs(d_test)
    shutil.copy(pt, os.path.join(d_test, "model.pt"))
    assert cli.main(plain + ["--testing"]) == 0
    line = [l for l in open(os.path.join(d_test, "log.test")).read().split("\n") if l.startswith("[Valid]")][0]
    tf1, tacc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", line).groups()
    assert (tf1, tacc) == (f1, acc), (line, valid)
