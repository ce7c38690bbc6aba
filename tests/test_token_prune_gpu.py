"""GPU: token pruning for predict - nbest_token_select and nbest_rows_compact against their restatements, the significance score
(nbest_attention_rollout_step on the mask) against fp64 column sums, model.predict(token_keep=...) against plain predict (no-op
schedules bit for bit, padding-only schedules within the eval-forward bounds) and against the fp64 oracle run on the kept indices,
the refusals, the training state it must leave alone and the command line."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
import token_prune_ref as R
from test_attn_probs_gpu import _build, _rnd
from test_head_gate_cpu import mixed_mask
from test_infer_gpu import _batch, _model, _same_state, _state
from test_model_gpu import SMALL_FACTOR, _cmp, _cmp_floor

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
NAN, INF = float("nan"), float("inf")


# ---- nbest_token_select ------------------------------------------------------------------------------------------------------------
SK = [(1, 1), (2, 1), (2, 2), (5, 3), (64, 63), (65, 33), (130, 64), (512, 511), (512, 1)]
KINDS = ["random", "equal", "duplicates", "masked_block", "few_real", "special"]


def _select_problem(kind, B, S, k):
    g = np.random.default_rng(S * 1000 + k + len(kind))
    sc = g.random((B, S)).astype(np.float32)
    mk = np.ones((B, S), dtype=np.uint8)
    if kind == "equal":
        sc[:] = 0.25
    elif kind == "duplicates":
        sc = g.choice(np.array([0.0, 0.125, 0.5, 0.5, 2.0], dtype=np.float32), size=(B, S))
        mk[:, S - S // 4:] = 0
    elif kind == "masked_block":
        mk[:, S // 3:S // 3 + max(1, S // 4)] = 0
        mk[B - 1, 0] = 0                                      # position 0 stays, masked or not
    elif kind == "few_real":
        mk[1, max(1, k // 2):] = 0                            # utterance 1: fewer real tokens than k (k >= 2)
        mk[0, S - S // 5:] = 0
        sc[mk == 0] = 0.0                                     # what the score kernel leaves on masked keys
    elif kind == "special":
        sc[g.random((B, S)) < 0.2] = NAN
        sc[g.random((B, S)) < 0.1] = INF
        sc[g.random((B, S)) < 0.1] = -INF
        sc[g.random((B, S)) < 0.1] = -0.0
        sc[g.random((B, S)) < 0.1] = 0.0
        mk[g.random((B, S)) < 0.25] = 0
    return sc, mk


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,k", SK)
def test_token_select_matches_reference(S, k, kind):
    """indices, both masks and the origins equal the restatement exactly; every output element is written and nothing around them"""
    from nbest_amd import hipabi as hb, trainer
    B = 3
    sc, mk = _select_problem(kind, B, S, k)
    want = trainer.token_select_reference(sc, mk, k)
    for b in range(B):
        assert want[b].tolist() == R.select_by_sorting(sc[b], mk[b], k)
    score, mask = torch.from_numpy(sc).to(DEV), torch.from_numpy(mk).to(DEV)
    org_in = (torch.arange(S, dtype=torch.int32)[None] * 3 + torch.arange(B, dtype=torch.int32)[:, None] + 7).to(DEV).contiguous()
    n = B * k
    bufs = [_guarded(n, torch.int32, -5), _guarded(n, torch.uint8, 9), _guarded(n, torch.float32, NAN), _guarded(n, torch.int32, -5)]
    (bi, idx), (bm, mo), (bf, mf), (bo, oo) = bufs
    L = hb.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    for origin in (org_in, None):
        rc = L.nbest_token_select(p(score), p(mask), p(origin) if origin is not None else None, k, p(idx), p(mo), p(mf), p(oo), B, S,
                                  hb.stream_ptr())
        assert rc == 0, hb.last_error()
        torch.cuda.synchronize()
        w = torch.from_numpy(want).to(DEV)
        assert torch.equal(idx.view(B, k).long(), w), "S=%d k=%d %s: indices differ" % (S, k, kind)
        assert torch.equal(mo.view(B, k), mask.gather(1, w).ne(0).to(torch.uint8)), "mask_out differs"
        assert torch.equal(mf.view(B, k), mask.gather(1, w).ne(0).float()), "maskf_out differs"
        src = org_in if origin is not None else torch.arange(S, dtype=torch.int32, device=DEV).expand(B, S)
        assert torch.equal(oo.view(B, k), src.gather(1, w)), "origin_out differs"
        for buf, fill in ((bi, -5), (bm, 9), (bo, -5)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), "a guard band was written"
        assert bool(torch.isnan(bf[:GUARD]).all()) and bool(torch.isnan(bf[GUARD + n:]).all()), "a guard band was written"
    # the wrapper, without origins
    i2, m2, f2, o2 = hb.token_select(score, mask, k, want_origin=False)
    torch.cuda.synchronize()
    assert o2 is None and torch.equal(i2, idx.view(B, k)) and torch.equal(m2, mo.view(B, k)) and torch.equal(f2, mf.view(B, k))


def test_token_select_chained_calls_compose_origin():
    from nbest_amd import hipabi as hb, trainer
    B, S, k1, k2 = 3, 130, 64, 17
    g = np.random.default_rng(9)
    s1, m1 = g.random((B, S)).astype(np.float32), np.ones((B, S), dtype=np.uint8)
    m1[1, 90:] = 0
    i1, mk1, f1, o1 = hb.token_select(torch.from_numpy(s1).to(DEV), torch.from_numpy(m1).to(DEV), k1)
    s2 = g.random((B, k1)).astype(np.float32)
    i2, mk2, f2, o2 = hb.token_select(torch.from_numpy(s2).to(DEV), mk1, k2, origin=o1)
    torch.cuda.synchronize()
    w1 = trainer.token_select_reference(s1, m1, k1)
    assert np.array_equal(o1.cpu().numpy(), w1)                                  # the first call's origins: its indices
    w2 = trainer.token_select_reference(s2, np.take_along_axis(m1, w1, 1), k2)
    assert np.array_equal(i2.cpu().numpy(), w2)
    assert np.array_equal(o2.cpu().numpy(), np.take_along_axis(w1, w2, 1)), "the second call's origins are not original positions"
    assert bool((o2[:, 0] == 0).all())


# ---- nbest_rows_compact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("B,S,k", [(3, 5, 3), (2, 130, 65), (1, 512, 1)])
def test_rows_compact_is_gather(B, S, k, H, dtype):
    from nbest_amd import hipabi as hb
    g = np.random.default_rng(B * S + k)
    src = _rnd(B, S, H, dtype=dtype, seed=S + H)
    idx = torch.from_numpy(np.stack([np.sort(g.choice(S, size=k, replace=False)) for _ in range(B)]).astype(np.int32)).to(DEV)
    if S == 512:
        idx[0, 0] = 511                                                           # the last row of the source
    n = B * k * H
    buf = torch.zeros(n + 2 * GUARD, dtype=dtype, device=DEV)
    buf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(-1)   # a NaN pattern no gathered value has
    out = buf[GUARD:GUARD + n].view(B, k, H)
    hb.rows_compact(src, idx, out=out)
    torch.cuda.synchronize()
    want = src.gather(1, idx.long()[:, :, None].expand(B, k, H))
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(out.view(it), want.contiguous().view(it)), "not torch.gather bit for bit"
    assert bool((buf[:GUARD].view(it) == -1).all()) and bool((buf[GUARD + n:].view(it) == -1).all()), "a guard band was written"
    assert torch.equal(hb.rows_compact(src, idx).view(it), want.contiguous().view(it))


def test_kernel_refusals():
    """each refusal returns its code, names its function and leaves sentinel-filled outputs as they were"""
    from nbest_amd import hipabi as hb
    L = hb.lib()
    ARG, SHAPE, DTYPE, ALIGN = -1, -2, -3, -4
    B, S, k, H = 2, 24, 8, 64
    p = lambda t: C.c_void_p(t.data_ptr())
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    nul = C.c_void_p(0)
    score = torch.rand(B, 600, device=DEV)
    mask = torch.ones(B, 600, dtype=torch.uint8, device=DEV)
    org = torch.zeros(B, 600, dtype=torch.int32, device=DEV)
    idx = torch.full((B, 600), -5, dtype=torch.int32, device=DEV)
    mo = torch.full((B, 600), 9, dtype=torch.uint8, device=DEV)
    mf = torch.full((B, 600), -7.0, device=DEV)
    oo = torch.full((B, 600), -5, dtype=torch.int32, device=DEV)
    good = dict(score=p(score), mask=p(mask), org=p(org), k=k, idx=p(idx), mo=p(mo), mf=p(mf), oo=p(oo), B=B, S=S)

    def sel(**kw):
        a = dict(good, **kw)
        return L.nbest_token_select(a["score"], a["mask"], a["org"], a["k"], a["idx"], a["mo"], a["mf"], a["oo"], a["B"], a["S"], hb.stream_ptr())

    for kw, code in [(dict(score=nul), ARG), (dict(mask=nul), ARG), (dict(idx=nul), ARG), (dict(mo=nul), ARG), (dict(mf=nul), ARG),
                     (dict(idx=p(score)), ARG), (dict(idx=p(mask)), ARG), (dict(idx=p(org)), ARG), (dict(mo=p(mask)), ARG),
                     (dict(oo=p(org)), ARG), (dict(k=0), SHAPE), (dict(k=S + 1), SHAPE), (dict(S=0, k=1), SHAPE), (dict(S=513), SHAPE),
                     (dict(B=0), SHAPE), (dict(score=off(score, 2)), ALIGN)]:
        rc = sel(**kw)
        assert rc == code, "token_select %s: returned %d, not %d" % (kw, rc, code)
        assert "token_select" in hb.last_error(), hb.last_error()
    src = torch.rand(B, S, H, device=DEV)
    dst = torch.full((B, 600, H), -7.0, device=DEV)
    ridx = torch.zeros(B, k, dtype=torch.int32, device=DEV)
    rgood = dict(src=p(src), idx=p(ridx), dst=p(dst), B=B, S=S, k=k, H=H, dtype=hb.F32)

    def rc_(**kw):
        a = dict(rgood, **kw)
        return L.nbest_rows_compact(a["src"], a["idx"], a["dst"], a["B"], a["S"], a["k"], a["H"], a["dtype"], hb.stream_ptr())

    for kw, code in [(dict(src=nul), ARG), (dict(idx=nul), ARG), (dict(dst=nul), ARG), (dict(dst=p(src)), ARG), (dict(dtype=2), DTYPE),
                     (dict(H=66), SHAPE), (dict(H=68, dtype=hb.BF16), SHAPE), (dict(k=0), SHAPE), (dict(k=S + 1), SHAPE), (dict(B=0), SHAPE),
                     (dict(src=off(src, 4)), ALIGN), (dict(dst=off(dst, 8)), ALIGN)]:
        rc = rc_(**kw)
        assert rc == code, "rows_compact %s: returned %d, not %d" % (kw, rc, code)
        assert "rows_compact" in hb.last_error(), hb.last_error()
    torch.cuda.synchronize()
    assert bool((idx == -5).all()) and bool((mo == 9).all()) and bool((mf == -7.0).all()) and bool((oo == -5).all()) and bool((dst == -7.0).all()), \
        "a refused call wrote an output"
    assert sel() == 0 and sel(org=nul, oo=nul) == 0 and rc_() == 0                  # the same arguments, unbroken, run
    torch.cuda.synchronize()


# ---- the score -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", [5, 65])
def test_score_is_the_column_sum_over_unmasked_queries(S, dtype):
    """nbest_attention_rollout_step with r_in = the mask as floats and residual 0 against fp64 column sums of
    nbest_attention_probs' output over the unmasked query rows, head mean: the bound of tests/test_rollout_gpu.py (fp32 summation of
    at most S heads non-negative terms), 1e-4 of the row's largest entry.  A masked query row is present and counts for nothing."""
    from nbest_amd import hipabi as hb, trainer
    B, heads = 2, 2
    qkv = _rnd(B * S, 3 * heads * 64, dtype=dtype, s=0.5 if dtype == torch.float32 else 1.0, seed=S)
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    mask[0, 2] = 0
    mask[1, S - 2:] = 0
    _, lse = hb.attention_fwd(qkv, mask, B, S, heads)
    P = hb.attention_probs(qkv, mask, lse, B, S, heads)
    got = hb.attention_rollout_step(qkv, mask, lse, mask.float(), 0.0, B, S, heads)
    torch.cuda.synchronize()
    want = torch.einsum("bi,bhij->bj", mask.double(), P.double()) / heads
    ref, _ = trainer.token_prune_reference(P, mask, 1)
    assert np.abs(ref - want.cpu().numpy()).max() <= 1e-12, "token_prune_reference states another score"
    top = want.max(-1).values
    err = (got.double() - want).abs().max(-1).values
    print("score %s S=%d: max |got - fp64| / largest = %.3e" % (dtype, S, (err / top).max().item()))
    assert (err <= R.TOL * top).all(), (err / top).tolist()
    assert bool((got[~mask.bool()] == 0).all()), "a masked key has a score"
    unmasked_only = torch.einsum("bhij->bj", P.double()) / heads               # every query row, masked ones included
    assert (unmasked_only - want).abs().max().item() > 1e-3, "the masked query rows make no difference: the case checks nothing"


# ---- predict: schedules that change nothing ------------------------------------------------------------------------------------------
def _models(labels, dtype):
    m2, _, _, meta, b2 = _build("bert_L2", labels, dtype)
    m3, cfg3, _ = _model(labels, L=3, dtype=dtype)
    m3.eval()
    b3 = _batch(cfg3, labels, 3, 5)
    return [("bert_L2", m2, b2["ids"], b2["seg"] if meta["seg"] else None), ("L3 B3 S5", m3, b3["ids"], b3["seg"])]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_noop_schedule_is_predict_bit_for_bit(dtype, labels):
    for tag, m, ids, seg in _models(labels, dtype):
        L, (B, S) = m.cfg.num_hidden_layers, ids.shape
        base = {k: v.clone() for k, v in m.predict(ids, seg_ids=seg).items()}
        for keep in ([S] * (L - 1), [512] * (L - 1)):
            out = m.predict(ids, seg_ids=seg, token_keep=keep, return_token_kept=True)
            torch.cuda.synchronize()
            assert set(out) == set(base) | {"token_kept", "token_counts"}
            for k in base:
                assert torch.equal(out[k].view(torch.uint8), base[k].view(torch.uint8)), "%s %s: %s differs from predict()" % (tag, keep, k)
            assert out["token_counts"] == [S] * L
            assert out["token_kept"].dtype == torch.int32 and out["token_kept"].shape == (L - 1, B, S)
            assert torch.equal(out["token_kept"], torch.arange(S, dtype=torch.int32, device=DEV).expand(L - 1, B, S))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dropping_only_padding_agrees_with_predict(dtype, labels):
    """keep = the longest real length of the batch: every utterance keeps all of its tokens (and padding, in index order), so the
    scores are those of predict() up to the order of the sums - the bounds of test_predict_agrees_with_eval_forward"""
    m, cfg, _ = _model(labels, L=3, dtype=dtype)
    m.eval()
    b = _batch(cfg, labels, 4, 48)
    pad = torch.zeros(4, 9, dtype=b["ids"].dtype, device=DEV)
    ids, seg = torch.cat([b["ids"], pad], 1).contiguous(), torch.cat([b["seg"], pad], 1).contiguous()
    real = (ids > 0).sum(1)
    longest, S = int(real.max()), ids.shape[1]
    assert longest < S and int(real.min()) < longest
    assert bool(((ids > 0).long().cumsum(1)[:, -1] == real).all()) and bool((ids[:, :longest] > 0).sum(1).eq(real).all()), "padding is not trailing"
    base = m.predict(ids, seg_ids=seg)
    out = m.predict(ids, seg_ids=seg, token_keep=[longest, longest], return_token_kept=True)
    torch.cuda.synchronize()
    assert out["token_counts"] == [S, longest, longest]
    want = torch.cat([torch.arange(longest, dtype=torch.int32), torch.full((S - longest,), -1, dtype=torch.int32)]).to(DEV)
    assert torch.equal(out["token_kept"], want.expand(2, 4, S)), "kept positions are not the first %d" % longest
    f32 = dtype == torch.float32
    _cmp("padding-only final", out["final"], base["final"].cpu(), atol=1e-6 if f32 else 2e-3)
    _cmp("padding-only top", out["top"], base["top"].cpu(), atol=1e-6 if f32 else 2e-3)
    if f32:
        assert torch.equal(out["pred"], base["pred"])


# ---- predict: end to end against the oracle ------------------------------------------------------------------------------------------
def _check_kept(tag, kept, cnt, S):
    """structure of token_kept [L-1, B, S]: cnt[l + 1] ascending original positions starting at 0, then -1; every row a subset of the
    row below"""
    Lm1, B, _ = kept.shape
    for l in range(Lm1):
        n = cnt[l + 1]
        assert bool((kept[l, :, n:] == -1).all()) and bool((kept[l, :, :n] >= 0).all()) and bool((kept[l, :, :n] < S).all()), "%s layer %d" % (tag, l)
        assert bool((kept[l, :, 0] == 0).all()), "%s layer %d: position 0 was dropped" % (tag, l)
        assert bool((kept[l, :, 1:n] > kept[l, :, :n - 1]).all()), "%s layer %d: positions are not ascending" % (tag, l)
        for u in range(B):
            below = set(range(S)) if l == 0 else set(kept[l - 1, u, :cnt[l]].tolist())
            assert set(kept[l, u, :n].tolist()) <= below, "%s layer %d utterance %d: a dropped token came back" % (tag, l, u)
        if cnt[l + 1] == cnt[l] and l > 0:
            assert torch.equal(kept[l], kept[l - 1]), "%s layer %d eliminated nothing but its row differs from the one below" % (tag, l)


def _check_valid_topk(tag, score, org, mask, kept_row, n):
    """``kept_row`` (original positions) is a top-n of fp64 ``score`` [S_l] over the tokens ``org`` with ``mask``, up to TOL of the
    largest score: no dropped real token scores more than that above a kept one; padding is kept only once every real token is"""
    score, org, mask = np.asarray(score, dtype=np.float64), np.asarray(org), np.asarray(mask).astype(bool)
    here = set(kept_row[:n].tolist())
    cur = [j for j in range(len(org)) if int(org[j]) in here]
    assert len(cur) == n, "%s: a kept position is not among the layer's tokens" % tag
    real = [j for j in range(1, len(org)) if mask[j]]
    ks = [float(score[j]) for j in real if j in cur]
    ds = [float(score[j]) for j in real if j not in cur]
    if ds:
        assert all(mask[j] or j == 0 for j in cur), "%s: padding was kept while a real token was dropped" % tag
        top = float(score[mask].max())
        over =(max(ds) - min(ks)) / top if ks else 0.0
        print("%s: best dropped - worst kept = %.3e of the largest score" % (tag, over))
        assert over <= R.TOL, "%s: a dropped token scores %.3e of the largest score above a kept one" % (tag, over)


@pytest.mark.parametrize("name", sorted(R.E2E))
def test_end_to_end_fp32_against_the_oracle(name, labels):
    """fp32 predict under the schedule of token_prune_ref.E2E (its inputs: test_token_prune_cpu.py).  The kept set of every
    eliminating layer is a valid top-k of the oracle's fp64 scores (the oracle following the GPU's own kept sets below that layer);
    the scores match the oracle run on the kept indices at the bar of test_predict_matches_reference_outputs; same labels."""
    from oracle import stc
    keep = R.E2E[name]
    m, cfg, _, meta, b = _build(name, labels, torch.float32)
    seg = b["seg"] if meta["seg"] else None
    out = m.predict(b["ids"], seg_ids=seg, token_keep=keep, return_token_kept=True)
    torch.cuda.synchronize()
    B, S = b["ids"].shape
    cnt = R.counts(S, keep)
    assert out["token_counts"] == cnt
    kept = out["token_kept"].cpu()
    _check_kept(name, kept, cnt, S)
    om, _, ob = R.oracle_model(name, labels)
    ref = R.oracle_pruned(om, ob["ids"], ob["seg"] if meta["seg"] else None, keep, kept=kept)
    elim = [l for l in range(meta["L"] - 1) if cnt[l + 1] < cnt[l]]
    assert len(elim) >= 3 and sorted(ref["scores"]) == elim
    for l in elim:
        score, org, mask = ref["scores"][l]
        for u in range(B):
            _check_valid_topk("%s layer %d utterance %d" % (name, l, u), score[u], org[u], mask[u], kept[l, u], cnt[l + 1])
    tag = "token_keep %s/f32 " % name
    _cmp(tag + "top", out["top"], ref["top"].float(), atol=1e-4)
    _cmp(tag + "final", out["final"], ref["final"].float(), atol=1e-4)
    bott = m._bottoms_dict(out["bott"])
    for k, v in ref["bottoms"].items():
        _cmp(tag + "bottoms[%s]" % k, bott[k], v.float(), atol=1e-4)
    odec = stc.decode_indices(ref["top"].float(), {k: v.float() for k, v in ref["bottoms"].items()}, labels.top2bottom, labels.idx2label)
    assert torch.equal(out["pred"].cpu().long(), odec), "decoded labels differ from the oracle's on the same kept indices"
    plain = m.predict(b["ids"], seg_ids=seg)
    assert (plain["final"] - out["final"]).abs().max().item() > 1e-3, "dropping tokens changed nothing: the schedule is a no-op"


def test_bf16_kept_set_and_scores(labels):
    """bf16, bert_L4_outliers under its E2E schedule.  Layer 0: the kept set is a valid top-k of fp64 scores formed from the model's
    own forward(return_attns=True) layer-0 map, at the same tolerance.  final: against the fp64 oracle (what the fp32 reference
    computes) run on the bf16 run's kept indices, within the factor-and-floor policy of the bf16 predict test (SMALL_FACTOR x the
    case's stored storage floor, rms within FLOOR_FACTOR x its rms)."""
    from nbest_amd import trainer
    name = "bert_L4_outliers"
    keep = R.E2E[name]
    meta, z = load_case(name)
    m, cfg, _, _, b = _build(name, labels, torch.bfloat16)
    seg = b["seg"] if meta["seg"] else None
    out = m.predict(b["ids"], seg_ids=seg, token_keep=keep, return_token_kept=True)
    _, _, _, attns, _, _ = m(type("O", (), {})(), b["ids"], seg_ids=seg, return_attns=True)
    torch.cuda.synchronize()
    B, S = b["ids"].shape
    cnt = R.counts(S, keep)
    assert cnt[1] < cnt[0], "layer 0 eliminates nothing"
    kept = out["token_kept"].cpu()
    _check_kept(name + " bf16", kept, cnt, S)
    mask = (b["ids"] > 0).cpu()
    score, _ = trainer.token_prune_reference(attns[0], mask, cnt[1])
    for u in range(B):
        _check_valid_topk("%s bf16 layer 0 utterance %d" % (name, u), score[u], np.arange(S), mask[u], kept[0, u], cnt[1])
    om, _, ob = R.oracle_model(name, labels)
    ref = R.oracle_pruned(om, ob["ids"], ob["seg"] if meta["seg"] else None, keep, kept=kept)
    _cmp_floor("token_keep %s/bf16 final" % name, out["final"], ref["final"].float(), z["floor/final"], factor=SMALL_FACTOR)


# ---- refusals, training state --------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(labels):
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, L=3, dtype=torch.bfloat16)
    m.eval()
    b = _batch(cfg, labels, 3, 40)
    ids, seg = b["ids"], b["seg"]
    base = {k: v.clone() for k, v in m.predict(ids, seg_ids=seg, token_keep=[30, 20]).items()}
    torch.cuda.synchronize()
    before = _state(m)
    for keep, word in (([30], "L - 1"), ([30, 20, 10], "L - 1"), ([30, 0], ">= 1"), ([20, 30], "non-increasing")):
        with pytest.raises(ValueError, match=word):
            m.predict(ids, seg_ids=seg, token_keep=keep)
    with pytest.raises(ValueError, match="return_attns"):
        m.predict(ids, seg_ids=seg, token_keep=[30, 20], return_attns=True)
    with pytest.raises(RuntimeError, match="fp8"):
        m.predict(ids, seg_ids=seg, token_keep=[30, 20], fp8=True)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    for kw in (dict(), dict(compact=True)):
        m.set_head_mask(mask, **kw)
        with pytest.raises(RuntimeError, match="not built"):
            m.predict(ids, seg_ids=seg, token_keep=[30, 20])
        m.set_head_mask(None)
    # the composite itself: the descriptor and buffers predict just used, a sentinel-filled cls_out
    B, S = ids.shape
    d = m._desc(B, S, "infer").desc
    i, s, p, k = m._inputs(ids, seg)
    ws = m._infer_ws
    cls = torch.full((B, cfg.hidden_size), -7.0, dtype=torch.bfloat16, device=DEV)
    kept = torch.full((2, B, S), -9, dtype=torch.int32, device=DEV)
    L = hb.lib()
    q = lambda t: C.c_void_p(t.data_ptr())

    def call(keep, n, gate=None, ws_bytes=None):
        arr = (C.c_int32 * 4)(*keep) if keep is not None else None
        d.head_gate = gate
        try:
            return L.nbest_encoder_infer_tokens(C.byref(d), q(m.arena.weights), q(m.arena.p), q(i), q(s), q(p), q(k), q(ws),
                                                ws.numel() if ws_bytes is None else ws_bytes, q(cls), arr, n, q(kept), hb.stream_ptr())
        finally:
            d.head_gate = None

    ARG, WORKSPACE = -1, call([30, 20, 0, 0], 2, ws_bytes=L.nbest_encoder_infer_ws_bytes(C.byref(d)))
    assert WORKSPACE not in (0, ARG) and "workspace" in hb.last_error()   # infer's own workspace is too small for the token rows
    for keep, n in (([30, 20, 0, 0], 1), ([30, 20, 10, 0], 3), (None, 2), ([30, 0, 0, 0], 2), ([20, 30, 0, 0], 2), ([-1, -1, 0, 0], 2)):
        assert call(keep, n) == ARG, (keep, n, hb.last_error())
        assert "encoder_infer_tokens" in hb.last_error()
    gate = torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads, device=DEV)
    assert call([30, 20, 0, 0], 2, gate=q(gate)) == ARG and "head gates" in hb.last_error()
    torch.cuda.synchronize()
    assert bool((cls == -7.0).all()) and bool((kept == -9).all()), "a refused call wrote its outputs"
    _same_state(before, _state(m))
    after = m.predict(ids, seg_ids=seg, token_keep=[30, 20])
    torch.cuda.synchronize()
    for key in base:
        assert torch.equal(base[key], after[key]), "predict %s changed" % key


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_after_token_keep_predict_is_unchanged(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_predict in (False, True):
        m, cfg, _ = _model(labels, dtype=dtype)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_predict:
            g0, step0 = m.arena.g.clone(), m.step_counter
            out = m.predict(b["ids"], seg_ids=b["seg"], token_keep=[24], return_token_kept=True)
            assert out["token_counts"] == [48, 24]
            assert torch.equal(m.arena.g, g0) and m.step_counter == step0
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after predict(token_keep=...) differs"


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_token_keep(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--lr", "3e-5", "--bert_lr", "3e-5", "--batchSize", "8", "--max_epoch", "1", "--experiment", exp,
              "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "3", "--n_best", "3", "--resume"]
    assert cli.main(common) == 0                               # a small random-weight model after one epoch on the 8 lines
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    plain, noop, noop2, cut = (str(tmp_path / n) for n in ("a.pred", "b.pred", "c.pred", "d.pred"))
    t_noop, t_cut = str(tmp_path / "b.tokens.jsonl"), str(tmp_path / "d.tokens.jsonl")
    assert cli.main(common + ["--predict", src, "--predict_output", plain]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", noop, "--token_keep", "512,512", "--predict_tokens", t_noop]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", noop2, "--token_keep", "512:512"]) == 0
    assert open(plain, "rb").read() == open(noop, "rb").read() == open(noop2, "rb").read(), ".pred differs under a no-op --token_keep"
    keep = [12, 5]
    assert cli.main(common + ["--predict", src, "--predict_output", cut, "--token_keep", "12:5", "--predict_tokens", t_cut]) == 0
    lines = open(plain).read().strip("\n").split("\n")
    assert len(open(cut).read().strip("\n").split("\n")) == len(lines)
    assert [l.split("\t<=>\t")[0] for l in open(cut).read().strip("\n").split("\n")] == [l.split("\t<=>\t")[0] for l in lines]
    n_in = len(open(src).read().strip("\n").split("\n"))
    for path, kp in ((t_noop, [512, 512]), (t_cut, keep)):
        recs = [json.loads(l) for l in open(path).read().strip("\n").split("\n")]
        assert [r["line"] for r in recs] == list(range(1, n_in + 1))
        for r in recs:
            assert set(r) == {"line", "segments", "tokens", "kept"}
            assert r["segments"][0] == "cls" and len(r["tokens"]) == len(r["segments"]) and len(r["kept"]) == 2
            ntok = sum(r["tokens"])
            for l, row in enumerate(r["kept"]):
                assert len(row) == len(r["segments"]) and all(0 <= x <= t for x, t in zip(row, r["tokens"]))
                assert row[0] == 1, "[CLS] was dropped"
                # S_{l+1} tokens stay, real ones before padding: the counts sum to S_{l+1} minus the padding among them
                assert sum(row) == min(kp[l], ntok), (r["line"], l, row)
    assert any(sum(r["tokens"]) > keep[0] for r in recs), "no utterance is longer than the first count: nothing was dropped"
    with pytest.raises(SystemExit, match="token_keep"):
        cli.main(common + ["--predict", src, "--token_keep", "12,5,5"])
