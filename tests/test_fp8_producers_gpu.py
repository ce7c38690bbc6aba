"""The e4m3 copies and amax records of the fp8 PRODUCERS, kernel by kernel and bit for bit (include/nbest_hip.h, "The fp8 PRODUCERS
on their own"): LayerNorm forward (y8), attention forward (ctx8; short and long kernel), LayerNorm backward fast path and the three
bf16 attention backwards (Fp8Grad), the cast with a history and amax_bf16.  The reference side is tests/fp8_producer_ref.py (checked
on the CPU by test_fp8_producers_cpu.py); conversions to e4m3 are torch's, on the CPU.

Contract A (LayerNorm forward, attention forward / backward, cast): the bytes are e4m3(out . s) of the bf16 tensor `out` the same call
stores, element for element, and the recorded amax is max |out| exactly.  Contract B (LayerNorm backward): the byte is rounded from
the fp32 value before its bf16 rounding - after the dropout mask and scale - so it lies within e4m3's half ulp plus a bf16 rounding of
out . s, a dropped element is byte 0x00, and bf16(recorded amax) == max |out| (round-to-nearest is monotone).  No tolerance here is
measured; the autograd tolerances of the LayerNorm backward are those of test_dropout_parity_gpu.test_layernorm_bwd_dropout.

s = 2^floor(log2(T / amax_prev)), T = 224 (activations) / 56 (gradients).  Histories 3.0, 0.37 and 150.0 give 64 | 512 | 1 and
16 | 128 | 1/4: all well inside a binade of T / amax, and 0.37 saturates most tensors here (the clamp is part of the reference).
"Recorded amax" is the maximum over the 16 slot words AND what nbest_fp8_amax_fold makes of them.

Conditions every producer is put through (C.1 - C.7 of the issue): outputs bit-equal to the plain entry; with nothing requested the
fp8 entry is the plain entry; record-only mode records what full mode records; attention backward with dqkv = NULL; slot words are
raised, never lowered, and only slot words are written; saturation under a history 8 x (and 64 x) too small; refusals.

Attention: the inputs, masks and fp32 references of test_dropout_parity_gpu._attn_problem (B = 4, heads = 3), S = 17 | 97 | 130 | 256 |
257: forward <1> <4> <5> <8> long; backward bwd2 with four waves, bwd3, bwd2 with eight waves (twice), long.  LayerNorm forward:
(4133, 256) has 1034 blocks' worth of rows for a grid capped at 1024, so the row loop and its clamped prefetch run twice.
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import nbest_amd  # noqa: E402,F401
from nbest_amd import hipabi as hb  # noqa: E402

import fp8_producer_ref as ref  # noqa: E402
import test_dropout_parity_gpu as dp  # noqa: E402  (_exact, _attn_problem and its shapes, LN_P / LN_SEED / LN_STREAM)
import test_kernels_gpu as tk  # noqa: E402  (rnd / close / tol_of / _log / _keep_mask: one kernel_parity.log for all kernel tests)

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
B, HEADS, H = dp.B, dp.HEADS, dp.H
W = hb.AMAX_TENSOR_WORDS
POS = ref.slot_positions(W)
NONSLOT = torch.ones(W, dtype=torch.bool)
NONSLOT[POS] = False
HISTORIES = (None, 3.0, 0.37, 150.0)
SENTINEL = 0x5A5A5A5A
_exact = dp._exact


def _bits(v):
    return None if v is None else ref.float_bits(v).to(DEV)


def _slots():
    return torch.zeros(W, dtype=torch.int32, device=DEV)


_EQUAL = [0, 0]          # bit-equality checks of the running test that held, and their elements: one log line per test


def _bytes_equal(tag, got, want):
    """got and want are the same bits (a failure is logged and raised by _exact, successes are counted)"""
    bad = got.view(torch.uint8) != want.view(torch.uint8)
    if bool(bad.any()):
        _exact(tag, bad)
    _EQUAL[0] += 1
    _EQUAL[1] += got.numel()


@pytest.fixture(autouse=True)
def _log_equalities(request):
    _EQUAL[:] = [0, 0]
    yield
    tk._log("%-58s %d bit-equality checks (plain entry / other modes) over %d elements held" % (request.node.name, _EQUAL[0], _EQUAL[1]))


def _recorded(tag, slots):
    """the recorded amax of a slot block that started as zeros: max over the 16 slot words == the fold's result; no other word
    written; the fold zeroes the slot words"""
    host = slots.cpu()
    assert not bool(host[NONSLOT].any()), tag + ": a word that is no slot position was written"
    m = host[POS].view(torch.float32).max().item()
    work, out = slots.clone(), torch.full((1,), -1, dtype=torch.int32, device=DEV)
    hb.fp8_amax_fold(work, out)
    folded = out.view(torch.float32).item()
    assert folded == m, "%s: fold gives %r, the slot words hold %r" % (tag, folded, m)
    assert not bool(work.any()), tag + ": slot words not zeroed by the fold"
    return m


def _history_for(true_amax, target, shrink):
    """a history `shrink` times smaller than the true amax, moved off a binade edge of target / history if it sits near one"""
    h = true_amax / shrink
    return h if ref.binade_margin(h, target) > 0.05 else h * 1.25


def _check_stored(tag, out, b8, slots, hist, target):
    """contract A for one call: bytes == e4m3(out . s) element for element, no NaN code, recorded amax == max |out|"""
    s = ref.pow2_scale(hist, target)
    o = out.float().cpu()
    got = b8.cpu()
    bad, nan = got != ref.e4m3_bytes(o * s), ref.is_nan_code(got)
    true = o.abs().max().item()
    rec = _recorded(tag, slots) if slots is not None else None
    ok = not bool(bad.any()) and not bool(nan.any()) and rec in (None, true)
    tk._log("%-58s s=%-6g bytes != e4m3(out s): %d of %d, NaN codes %d, saturated %d, recorded %s max|out| %.9g %s" % (
        tag, s, int(bad.sum()), bad.numel(), int(nan.sum()), int(((o * s).abs() > ref.E4M3_MAX).sum()),
        "-" if rec is None else "%.9g" % rec, true, "OK" if ok else "FAIL"))
    assert not bool(bad.any()), "%s: %d of %d bytes differ from e4m3(out * %g), first at %s" % (tag, int(bad.sum()), bad.numel(), s, bad.nonzero()[0].tolist())
    assert not bool(nan.any()), "%s: %d e4m3 NaN codes" % (tag, int(nan.sum()))
    assert rec in (None, true), "%s: recorded amax %r, max |out| %r" % (tag, rec, true)
    return true


def _check_slot_semantics(tag, run, fresh):
    """condition 5: `run(slots)` on a block whose slot word 0 holds 1e-30 (must be raised to what a zeroed block gets: `fresh`),
    slot word 1 holds 1e30 (must survive), every other slot word 0, and every word that is no slot position a sentinel"""
    pre = torch.full((W,), SENTINEL, dtype=torch.int32)
    pre[POS] = 0
    pre[POS[0]], pre[POS[1]] = ref.float_bits(1e-30)[0], ref.float_bits(1e30)[0]
    fresh = fresh.cpu()
    assert fresh[POS[0]:POS[0] + 1].view(torch.float32).item() > 1e-30, tag + ": block 0 recorded nothing"
    want = torch.where(NONSLOT, pre, fresh)
    want[POS[1]] = pre[POS[1]]
    got = pre.clone().to(DEV)
    run(got)
    _exact(tag + " slots: raised | kept | rest untouched", got.cpu() != want)


# ---- attention ----------------------------------------------------------------------------------
ATTN_S = [17, 97, 130, 256, 257]
ATTN_P = [0.0, 0.2]


def _attn_outlier(pr, S, backward):
    """the case's inputs with ONE outlier whose effect peaks in the last valid row, token S - 1 of utterance 0 (all keys unmasked), in the
    first head h whose dropout decision keeps (query S - 1, key S - 1): K[S-1] = Q[S-1] makes query S - 1 attend to key S - 1 (score
    |q|^2 / 8, about 8, among scores of order 1); forward: V[S-1] x 60, so ctx[S-1] is about 60 V[S-1] while every other query sees it
    through a small probability; backward: dctx[S-1] x 60 instead"""
    qkv, dctx = pr.qkv.clone(), pr.dctx.clone()
    h = int(pr.keep[0, :, S - 1, S - 1].nonzero()[0])
    v = qkv.view(B, S, 3, HEADS, 64)
    v[0, S - 1, 1, h] = v[0, S - 1, 0, h]
    if backward:
        dctx.view(B, S, HEADS, 64)[0, S - 1, h] *= 60
    else:
        v[0, S - 1, 2, h] *= 60
    return qkv, dctx


def _row_of_max(t):
    return int(t.float().abs().amax(dim=1).argmax())


@pytest.mark.parametrize("p", ATTN_P, ids=["p0", "p0.2"])
@pytest.mark.parametrize("S", ATTN_S)
def test_attention_fwd_ctx8(S, p):
    pr = dp._attn_problem(BF, S, p)
    drop = dict(drop_p=p, seed=dp.SEED, drop_stream=dp.STREAM)
    tag = "fp8 attn fwd S=%d p=%g" % (S, p)
    ctx0, lse0 = hb.attention_fwd(pr.qkv, pr.mask, B, S, HEADS, **drop)
    tk.close(tag + " ctx (the tensor the bytes are compared with)", ctx0, pr.ctx, tk.tol_of(BF))
    full = None
    for want_keep in ((False, True) if S <= 256 else (False,)):
        plain = hb.attention_fwd(pr.qkv, pr.mask, B, S, HEADS, want_keep=want_keep, **drop)
        # condition 2: nothing requested
        ctx, lse, keep, none = hb.attention_fwd_fp8(pr.qkv, pr.mask, B, S, HEADS, want_keep=want_keep, want8=False, **drop)
        assert none is None
        _bytes_equal(tag + " nothing requested: ctx", ctx, plain[0])
        _bytes_equal(tag + " nothing requested: lse", lse, plain[1])
        for hist in HISTORIES:
            t = "%s kw=%d hist=%s" % (tag, want_keep, hist)
            slots = _slots()
            ctx, lse, keep, ctx8 = hb.attention_fwd_fp8(pr.qkv, pr.mask, B, S, HEADS, want_keep=want_keep, amax_prev=_bits(hist),
                                                        amax_slots=slots, **drop)
            _bytes_equal(t + " ctx == plain entry", ctx, plain[0])          # condition 1
            _bytes_equal(t + " lse == plain entry", lse, plain[1])
            _bytes_equal(t + " ctx == entry without keep words", ctx, ctx0)
            if want_keep:
                assert keep is not None and torch.equal(keep, plain[2]), t + ": keep words differ from the plain entry's"
            true = _check_stored(t, ctx, ctx8, slots, hist, ref.ACT_TARGET)
            full = slots.clone() if full is None else full
            assert torch.equal(slots, full), t + ": the slot words depend on the history or on the keep words"
    # condition 3: record-only mode (the calibration pass) records what full mode records
    slots = _slots()
    ctx, _, _, none = hb.attention_fwd_fp8(pr.qkv, pr.mask, B, S, HEADS, amax_slots=slots, want8=False, **drop)
    assert none is None and torch.equal(slots, full), tag + ": record-only slot words differ from full mode's"
    _bytes_equal(tag + " record-only: ctx", ctx, ctx0)
    # a copy without a record
    ctx8 = hb.attention_fwd_fp8(pr.qkv, pr.mask, B, S, HEADS, amax_prev=_bits(3.0), **drop)[3]
    _check_stored(tag + " copy only", ctx0, ctx8, None, 3.0, ref.ACT_TARGET)
    # condition 6: saturation
    for shrink in (8, 64):
        hist = _history_for(true, ref.ACT_TARGET, shrink)
        assert true * ref.pow2_scale(hist, ref.ACT_TARGET) > ref.E4M3_MAX          # it does saturate
        slots = _slots()
        ctx8 = hb.attention_fwd_fp8(pr.qkv, pr.mask, B, S, HEADS, amax_prev=_bits(hist), amax_slots=slots, **drop)[3]
        _check_stored(tag + " saturating x%d" % shrink, ctx0, ctx8, slots, hist, ref.ACT_TARGET)
    # condition 5
    _check_slot_semantics(tag, lambda s: hb.attention_fwd_fp8(pr.qkv, pr.mask, B, S, HEADS, amax_prev=_bits(3.0), amax_slots=s, **drop), full)


@pytest.mark.parametrize("p", ATTN_P, ids=["p0", "p0.2"])
@pytest.mark.parametrize("S", ATTN_S)
def test_attention_fwd_ctx8_outlier_in_last_row(S, p):
    pr = dp._attn_problem(BF, S, p)
    drop = dict(drop_p=p, seed=dp.SEED, drop_stream=dp.STREAM)
    qkv, _ = _attn_outlier(pr, S, backward=False)
    tag = "fp8 attn fwd outlier S=%d p=%g" % (S, p)
    ctx0, lse0 = hb.attention_fwd(qkv, pr.mask, B, S, HEADS, **drop)
    assert _row_of_max(ctx0) == S - 1, tag + ": the outlier does not put max |ctx| into the last valid row"
    for hist in (None, 150.0):
        slots = _slots()
        ctx, lse, _, ctx8 = hb.attention_fwd_fp8(qkv, pr.mask, B, S, HEADS, amax_prev=_bits(hist), amax_slots=slots, **drop)
        _bytes_equal(tag + " ctx == plain entry", ctx, ctx0)
        _bytes_equal(tag + " lse == plain entry", lse, lse0)
        _check_stored("%s hist=%s" % (tag, hist), ctx, ctx8, slots, hist, ref.ACT_TARGET)


ATTN_BWD_CASES = [(S, p, kw) for S in ATTN_S for p in ATTN_P for kw in ((False, True) if S <= 256 else (False,))]
ATTN_BWD_IDS = ["S%d-p%g-%s" % (S, p, "keepwords" if kw else "rehash") for S, p, kw in ATTN_BWD_CASES]


def _attn_fwd_for_bwd(qkv, mask, S, drop, keepwords):
    r = hb.attention_fwd(qkv, mask, B, S, HEADS, want_keep=keepwords, **drop)
    keep = r[2] if keepwords else None
    assert not keepwords or keep is not None
    return r[0], r[1], keep


@pytest.mark.parametrize("S,p,keepwords", ATTN_BWD_CASES, ids=ATTN_BWD_IDS)
def test_attention_bwd_dqkv8(S, p, keepwords):
    pr = dp._attn_problem(BF, S, p)
    drop = dict(drop_p=p, seed=dp.SEED, drop_stream=dp.STREAM)
    tag = "fp8 attn bwd S=%d p=%g %s" % (S, p, "kw" if keepwords else "rh")
    ctx, lse, keep = _attn_fwd_for_bwd(pr.qkv, pr.mask, S, drop, keepwords)
    args = (pr.qkv, pr.mask, ctx, pr.dctx, lse, B, S, HEADS)
    dbias0 = torch.zeros(3 * H, device=DEV)
    dqkv0 = hb.attention_bwd(*args, dbias=dbias0, keep=keep, **drop)
    d, r = dqkv0.float().reshape(B * S, 3, H), pr.dqkv.reshape(B * S, 3, H)
    for i, nm in enumerate("QKV"):
        tk.close(tag + " d%s (the tensor the bytes are compared with)" % nm, d[:, i], r[:, i], 2 * tk.tol_of(BF))
    # condition 2: nothing requested
    dbias = torch.zeros(3 * H, device=DEV)
    dqkv, none = hb.attention_bwd_fp8(*args, dbias=dbias, keep=keep, want8=False, **drop)
    assert none is None
    _bytes_equal(tag + " nothing requested: dqkv", dqkv, dqkv0)
    _bytes_equal(tag + " nothing requested: dbias", dbias, dbias0)
    full = None
    for hist in HISTORIES:
        t = "%s hist=%s" % (tag, hist)
        slots, dbias = _slots(), torch.zeros(3 * H, device=DEV)
        dqkv, out8 = hb.attention_bwd_fp8(*args, dbias=dbias, keep=keep, amax_prev=_bits(hist), amax_slots=slots, **drop)
        _bytes_equal(t + " dqkv == plain entry", dqkv, dqkv0)                # condition 1
        _bytes_equal(t + " dbias == plain entry", dbias, dbias0)
        true = _check_stored(t, dqkv, out8, slots, hist, ref.GRAD_TARGET)
        full = slots.clone() if full is None else full
        assert torch.equal(slots, full), t + ": the recorded amax depends on the history"
        # condition 4: dqkv = NULL writes the same bytes and the same amax (and the fused bias gradient)
        slots2, dbias2 = _slots(), torch.zeros(3 * H, device=DEV)
        none, out8b = hb.attention_bwd_fp8(*args, dbias=dbias2, keep=keep, amax_prev=_bits(hist), amax_slots=slots2, want_dqkv=False, **drop)
        assert none is None
        _bytes_equal(t + " dqkv=NULL: bytes", out8b, out8)
        _bytes_equal(t + " dqkv=NULL: dbias", dbias2, dbias0)
        assert torch.equal(slots2, slots), t + ": dqkv=NULL records another amax"
    # condition 3: record-only
    slots = _slots()
    dqkv, none = hb.attention_bwd_fp8(*args, keep=keep, amax_slots=slots, want8=False, **drop)
    assert none is None and torch.equal(slots, full), tag + ": record-only slot words differ from full mode's"
    _bytes_equal(tag + " record-only: dqkv", dqkv, dqkv0)
    # a copy without a record, with and without dqkv
    for want_dqkv in (True, False):
        out8 = hb.attention_bwd_fp8(*args, keep=keep, amax_prev=_bits(3.0), want_dqkv=want_dqkv, **drop)[1]
        _check_stored(tag + " copy only dqkv=%d" % want_dqkv, dqkv0, out8, None, 3.0, ref.GRAD_TARGET)
    # condition 6: a history 8 x too small is what the gradients' headroom covers - amax lands in (112, 448] and NOTHING saturates, the
    # bytes must simply still be right; 64 x is the case that does saturate
    for shrink in (8, 64):
        hist = _history_for(true, ref.GRAD_TARGET, shrink)
        top = true * ref.pow2_scale(hist, ref.GRAD_TARGET)
        assert top > (2 * ref.E4M3_MAX if shrink == 64 else ref.E4M3_MAX / 4)
        slots = _slots()
        out8 = hb.attention_bwd_fp8(*args, keep=keep, amax_prev=_bits(hist), amax_slots=slots, want_dqkv=False, **drop)[1]
        _check_stored(tag + (" history / 8 (inside the headroom)" if shrink == 8 else " saturating x64"), dqkv0, out8, slots, hist, ref.GRAD_TARGET)
    # condition 5
    _check_slot_semantics(tag, lambda s: hb.attention_bwd_fp8(*args, keep=keep, amax_prev=_bits(3.0), amax_slots=s, **drop), full)


@pytest.mark.parametrize("S,p,keepwords", ATTN_BWD_CASES, ids=ATTN_BWD_IDS)
def test_attention_bwd_dqkv8_outlier_in_last_row(S, p, keepwords):
    pr = dp._attn_problem(BF, S, p)
    drop = dict(drop_p=p, seed=dp.SEED, drop_stream=dp.STREAM)
    qkv, dctx = _attn_outlier(pr, S, backward=True)
    tag = "fp8 attn bwd outlier S=%d p=%g %s" % (S, p, "kw" if keepwords else "rh")
    ctx, lse, keep = _attn_fwd_for_bwd(qkv, pr.mask, S, drop, keepwords)
    args = (qkv, pr.mask, ctx, dctx, lse, B, S, HEADS)
    dqkv0 = hb.attention_bwd(*args, keep=keep, **drop)
    assert _row_of_max(dqkv0) == S - 1, tag + ": the outlier does not put max |dqkv| into the last valid row"
    for hist, want_dqkv in ((None, True), (150.0, True), (150.0, False)):
        slots = _slots()
        dqkv, out8 = hb.attention_bwd_fp8(*args, keep=keep, amax_prev=_bits(hist), amax_slots=slots, want_dqkv=want_dqkv, **drop)
        if want_dqkv:
            _bytes_equal(tag + " dqkv == plain entry", dqkv, dqkv0)
        _check_stored("%s hist=%s dqkv=%d" % (tag, hist, want_dqkv), dqkv0, out8, slots, hist, ref.GRAD_TARGET)


# ---- LayerNorm forward --------------------------------------------------------------------------
LNF_CASES = [(37, 256), (300, 512), (37, 768), (300, 1024), (4133, 256)]


def _ln_inputs(M, H_):
    x = tk.rnd(M, H_, dtype=BF, seed=31)
    return x, 1 + 0.1 * tk.rnd(H_, seed=32), 0.1 * tk.rnd(H_, seed=33)


@pytest.mark.parametrize("outlier", [False, True], ids=["plain", "outlier"])
@pytest.mark.parametrize("M,H_", LNF_CASES, ids=["%dx%d" % c for c in LNF_CASES])
def test_layernorm_fwd_y8(M, H_, outlier):
    x, g, b = _ln_inputs(M, H_)
    tag = "fp8 ln_fwd %dx%d%s" % (M, H_, " outlier" if outlier else "")
    if outlier:                              # one element of the last row at 60 among unit normals: its normalised value is 15 or more
        x[M - 1, 5] = 60.0
    y0, st0 = hb.layernorm_fwd(x, g, b, 1e-12)
    tk.close(tag + " y (the tensor the bytes are compared with)", y0, torch.nn.functional.layer_norm(x.float(), (H_,), g, b, 1e-12), tk.tol_of(BF))
    if outlier:
        assert _row_of_max(y0) == M - 1, tag + ": the outlier does not put max |y| into the last row"
    y, st, none = hb.layernorm_fwd_fp8(x, g, b, 1e-12, want8=False)           # condition 2
    assert none is None
    _bytes_equal(tag + " nothing requested: y", y, y0)
    _bytes_equal(tag + " nothing requested: stats", st, st0)
    full = None
    for hist in HISTORIES:
        t = "%s hist=%s" % (tag, hist)
        slots = _slots()
        y, st, y8 = hb.layernorm_fwd_fp8(x, g, b, 1e-12, amax_prev=_bits(hist), amax_slots=slots)
        _bytes_equal(t + " y == plain entry", y, y0)                          # condition 1
        _bytes_equal(t + " stats == plain entry", st, st0)
        true = _check_stored(t, y, y8, slots, hist, ref.ACT_TARGET)
        full = slots.clone() if full is None else full
        assert torch.equal(slots, full), t + ": the recorded amax depends on the history"
    # condition 3 as this producer has it: WITHOUT y8 it records nothing (the encoder's calibration pass measures y with amax_bf16)
    slots = _slots()
    y, st, none = hb.layernorm_fwd_fp8(x, g, b, 1e-12, amax_slots=slots, want8=False)
    assert none is None and not bool(slots.any()), tag + ": recorded without a copy"
    _bytes_equal(tag + " record-only: y", y, y0)
    cal = _slots()
    hb.amax_bf16(y0, cal)                    # ... and that launch records what the fused record would have
    assert _recorded(tag + " amax_bf16(y)", cal) == true
    y8 = hb.layernorm_fwd_fp8(x, g, b, 1e-12, amax_prev=_bits(3.0))[2]       # a copy without a record
    _check_stored(tag + " copy only", y0, y8, None, 3.0, ref.ACT_TARGET)
    for shrink in (8, 64):                   # condition 6
        hist = _history_for(true, ref.ACT_TARGET, shrink)
        assert true * ref.pow2_scale(hist, ref.ACT_TARGET) > ref.E4M3_MAX          # it does saturate
        slots = _slots()
        y8 = hb.layernorm_fwd_fp8(x, g, b, 1e-12, amax_prev=_bits(hist), amax_slots=slots)[2]
        _check_stored(tag + " saturating x%d" % shrink, y0, y8, slots, hist, ref.ACT_TARGET)
    _check_slot_semantics(tag, lambda s: hb.layernorm_fwd_fp8(x, g, b, 1e-12, amax_prev=_bits(3.0), amax_slots=s), full)   # condition 5


# ---- LayerNorm backward -------------------------------------------------------------------------
def _check_rounded_before_bf16(tag, out, b8, slots, hist, keep, not_tiny):
    """contract B for one call: out = the bf16 tensor the byte covers (dx_drop under dropout, else dx), keep = the dropout mask or None"""
    s = ref.pow2_scale(hist, ref.GRAD_TARGET)
    o = out.float().cpu()
    got = b8.cpu()
    nan = ref.is_nan_code(got)
    v = (o * s).clamp(-ref.E4M3_MAX, ref.E4M3_MAX)
    err, bound = (ref.dequant(got) - v).abs(), ref.fp32_rounded_bound(v)
    out_of_bound = ~(err <= bound)                                       # (a NaN byte is out of bound too)
    true = o.abs().max().item()
    rec = _recorded(tag, slots) if slots is not None else None
    rb = None if rec is None else torch.tensor(rec).bfloat16().item()
    ok = not bool(out_of_bound.any()) and not bool(nan.any()) and rb in (None, true)
    tk._log("%-58s s=%-6g |byte - out s| > max(2^-4 |v|, 2^-10) + 2^-7 |v|: %d of %d (max err / bound %.3f), NaN codes %d, saturated %d, "
            "recorded %s -> bf16 %s max|out| %.9g %s" % (tag, s, int(out_of_bound.sum()), err.numel(), (err / bound).max().item(), int(nan.sum()),
                                                      int(((o * s).abs() > ref.E4M3_MAX).sum()), "-" if rec is None else "%.9g" % rec,
                                                      "-" if rb is None else "%.9g" % rb, true, "OK" if ok else "FAIL"))
    assert not bool(nan.any()), "%s: %d e4m3 NaN codes" % (tag, int(nan.sum()))
    assert not bool(out_of_bound.any()), "%s: %d of %d bytes outside the bound, first at %s" % (tag, int(out_of_bound.sum()), err.numel(), out_of_bound.nonzero()[0].tolist())
    assert rb in (None, true), "%s: bf16(recorded amax %r) = %r, max |out| %r" % (tag, rec, rb, true)
    if keep is not None:
        k = keep.cpu()
        _exact(tag + " dropped element is byte 0x00", (got != 0) & ~k)
        # a kept element that is not tiny and whose scaled bf16 value is at least one subnormal step (2^-9) cannot round to a zero byte:
        # that needs |x s| <= 2^-10, and the bf16 rounding moves x by 2^-9 of itself at most
        _exact(tag + " kept element is a nonzero byte", ((got & 0x7F) == 0) & k & not_tiny.cpu() & (v.abs() >= 2.0 ** -9))
    return true


@pytest.mark.parametrize("outlier", [False, True], ids=["plain", "outlier"])
@pytest.mark.parametrize("p", [0.0, dp.LN_P], ids=["p0", "p0.25"])
@pytest.mark.parametrize("M", [37, 300])
@pytest.mark.parametrize("H_", [256, 512, 768, 1024])
def test_layernorm_bwd_out8(H_, M, p, outlier):
    x, g, _ = _ln_inputs(M, H_)
    dy = tk.rnd(M, H_, dtype=BF, seed=34)
    drop = dict(drop_p=p, seed=dp.LN_SEED, drop_stream=dp.LN_STREAM)
    keep, scale = tk._keep_mask(M, H_, p, dp.LN_SEED, dp.LN_STREAM)
    tag = "fp8 ln_bwd %dx%d p=%g%s" % (M, H_, p, " outlier" if outlier else "")
    if outlier:                              # one kept element of the last row at 60 among unit normals: dx of that element follows it
        dy[M - 1, int(keep[M - 1].nonzero()[0])] = 60.0
    _, stats = hb.layernorm_fwd(x, g, torch.zeros_like(g), 1e-12)
    xr, gr, br = x.float().clone().requires_grad_(True), g.clone().requires_grad_(True), torch.zeros_like(g).requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (H_,), gr, br, 1e-12).backward(dy.float())
    dxd_ref = xr.grad * keep * scale
    tol = tk.tol_of(BF)
    not_tiny = xr.grad.abs() > tol * xr.grad.abs().max()
    covered = (lambda dx, dxd: dxd) if p > 0 else (lambda dx, dxd: dx)
    km = keep if p > 0 else None

    def same(t, a, b_):
        for nm, u, v in zip(("dx", "dx_drop", "dgamma", "dbeta", "dbias"), a, b_):
            assert (u is None) == (v is None), "%s: %s present in one call only" % (t, nm)
            if u is not None:
                _bytes_equal("%s %s" % (t, nm), u, v)

    plain = hb.layernorm_bwd(dy, x, stats, g, **drop)
    dx0, dxd0, dg0, db0, dbias0 = plain
    out0 = covered(dx0, dxd0)
    if outlier:
        assert _row_of_max(out0) == M - 1, tag + ": the outlier does not put the maximum into the last row"
    # the tensor the bytes are compared with, and the sums of the same launch, against autograd (tolerances of test_layernorm_bwd_dropout)
    tk.close(tag + " dx", dx0, xr.grad, tol)
    if p > 0:
        _exact(tag + " dx_drop zero where dropped", (dxd0.float() != 0) & ~keep)
        _exact(tag + " dx_drop nonzero where kept", (dxd0.float() == 0) & keep & not_tiny)
        tk.close(tag + " dx_drop", dxd0, dxd_ref, tol)
    tk.close(tag + " dgamma", dg0, gr.grad, 5 * tol)
    tk.close(tag + " dbeta", db0, br.grad, 5 * tol)
    tk.close(tag + " dbias", dbias0, dxd_ref.sum(0), 5 * tol)
    r = hb.layernorm_bwd_fp8(dy, x, stats, g, want8=False, **drop)           # condition 2
    assert r[5] is None
    same(tag + " nothing requested:", r[:5], plain)
    full8 = {}
    full = None
    for hist in HISTORIES:
        t = "%s hist=%s" % (tag, hist)
        slots = _slots()
        r = hb.layernorm_bwd_fp8(dy, x, stats, g, amax_prev=_bits(hist), amax_slots=slots, **drop)
        same(t + " == plain entry:", r[:5], plain)                            # condition 1
        true = _check_rounded_before_bf16(t, out0, r[5], slots, hist, km, not_tiny)
        full8[hist] = r[5]
        full = slots.clone() if full is None else full
        assert torch.equal(slots, full), t + ": the recorded amax depends on the history"
    # the other instantiations write the bytes and the record of the full call: no bias sum (DBIAS = false), no sums at all (PARAMS = false),
    # and under dropout dx_drop = NULL (only its e4m3 copy is wanted: the mode the fp8 backward runs)
    modes = [("no dbias", dict(want_dbias=False)), ("no params", dict(want_params=False))]
    if p > 0:
        modes += [("dx_drop=NULL", dict(want_dx_drop=False)), ("dx_drop=NULL no params", dict(want_dx_drop=False, want_params=False))]
    for nm, kw in modes:
        ref_out = hb.layernorm_bwd(dy, x, stats, g, **dict(drop, **{k: v for k, v in kw.items() if k != "want_dx_drop"}))
        for hist in (None, 3.0):
            t = "%s %s hist=%s" % (tag, nm, hist)
            slots = _slots()
            r = hb.layernorm_bwd_fp8(dy, x, stats, g, amax_prev=_bits(hist), amax_slots=slots, **drop, **kw)
            if "want_dx_drop" in kw:
                assert r[1] is None
                same(t + " == plain entry:", r[:5], (ref_out[0], None) + tuple(ref_out[2:]))
            else:
                same(t + " == plain entry:", r[:5], ref_out)
            _bytes_equal(t + " dx == full call", r[0], dx0)
            _bytes_equal(t + " bytes == full call", r[5], full8[hist])
            assert torch.equal(slots, full), t + ": records another amax than the full call"
    slots = _slots()                         # condition 3: record-only
    r = hb.layernorm_bwd_fp8(dy, x, stats, g, amax_slots=slots, want8=False, **drop)
    assert r[5] is None and torch.equal(slots, full), tag + ": record-only slot words differ from full mode's"
    same(tag + " record-only == plain entry:", r[:5], plain)
    for shrink in (8, 64):                   # condition 6 (8 x: inside the gradients' headroom, nothing saturates; 64 x saturates)
        hist = _history_for(true, ref.GRAD_TARGET, shrink)
        top = true * ref.pow2_scale(hist, ref.GRAD_TARGET)
        assert top > (2 * ref.E4M3_MAX if shrink == 64 else ref.E4M3_MAX / 4)
        slots = _slots()
        r = hb.layernorm_bwd_fp8(dy, x, stats, g, amax_prev=_bits(hist), amax_slots=slots, **drop)
        _check_rounded_before_bf16(tag + (" history / 8 (inside the headroom)" if shrink == 8 else " saturating x64"), out0, r[5], slots, hist, km, not_tiny)
    _check_slot_semantics(tag, lambda s: hb.layernorm_bwd_fp8(dy, x, stats, g, amax_prev=_bits(3.0), amax_slots=s, **drop), full)   # condition 5


# ---- the cast with a history, amax_bf16 ---------------------------------------------------------
CAST_N = [8, 8 * 4096 * 256 + 40]            # one element group | one group past the grid cap: the second stride iteration
AMAX_N = [8, 2048 * 2048 + 40]


@functools.lru_cache(maxsize=None)
def _flat(n):
    return types.SimpleNamespace(x=tk.rnd(n, dtype=BF, seed=9))


@pytest.mark.parametrize("where", ["first", "last", "none"])
@pytest.mark.parametrize("n", CAST_N)
def test_cast_with_history(n, where):
    x = _flat(n).x.clone()
    if where != "none":                      # the maximum once in the first element group, once in the last
        x[0 if where == "first" else n - 1] = -300.0
    tag = "fp8 cast n=%d max %s" % (n, where)
    plain = hb.cast_fp8(x)
    _bytes_equal(tag + " nothing requested == plain entry", hb.cast_fp8_scaled(x), plain)
    full = None
    for hist in HISTORIES:
        slots = _slots()
        b8 = hb.cast_fp8_scaled(x, amax_prev=_bits(hist), amax_slots=slots)
        true = _check_stored("%s hist=%s" % (tag, hist), x, b8, slots, hist, ref.ACT_TARGET)
        assert where == "none" or true == 300.0
        full = slots.clone() if full is None else full
        assert torch.equal(slots, full)
    _check_stored(tag + " copy only", x, hb.cast_fp8_scaled(x, amax_prev=_bits(3.0)), None, 3.0, ref.ACT_TARGET)
    for shrink in (8, 64):
        hist = _history_for(true, ref.ACT_TARGET, shrink)
        slots = _slots()
        _check_stored(tag + " saturating x%d" % shrink, x, hb.cast_fp8_scaled(x, amax_prev=_bits(hist), amax_slots=slots), slots, hist, ref.ACT_TARGET)
    _check_slot_semantics(tag, lambda s: hb.cast_fp8_scaled(x, amax_prev=_bits(3.0), amax_slots=s), full)


@pytest.mark.parametrize("where", ["first", "last", "none"])
@pytest.mark.parametrize("n", AMAX_N)
def test_amax_bf16(n, where):
    x = _flat(n).x.clone()
    if where != "none":
        x[0 if where == "first" else n - 1] = -300.0
    tag = "fp8 amax_bf16 n=%d max %s" % (n, where)
    slots = _slots()
    hb.amax_bf16(x, slots)
    rec, true = _recorded(tag, slots), x.float().abs().max().item()
    tk._log("%-58s recorded=%.9g max|x|=%.9g %s" % (tag, rec, true, "OK" if rec == true else "FAIL"))
    assert rec == true and (where == "none" or true == 300.0)
    cast = _slots()
    hb.cast_fp8_scaled(x, amax_slots=cast)   # the cast's grid is another one: the same maximum, possibly in other slot words
    assert _recorded(tag + " cast", cast) == rec
    _check_slot_semantics(tag, lambda s: hb.amax_bf16(x, s), slots)


# ---- condition 7: refusals that need no launch --------------------------------------------------
SHAPE, ARG = r"\(-2\)", r"\(-1\)"            # NBEST_ERR_SHAPE, NBEST_ERR_ARG


def test_refusals():
    for dtype, H_ in ((F32, 256), (BF, 320)):
        x = tk.rnd(8, H_, dtype=dtype, seed=31)
        g, b = torch.ones(H_, device=DEV), torch.zeros(H_, device=DEV)
        y, stats = hb.layernorm_fwd(x, g, b, 1e-12)
        with pytest.raises(RuntimeError, match=SHAPE):
            hb.layernorm_fwd_fp8(x, g, b, 1e-12, amax_slots=_slots())
        with pytest.raises(RuntimeError, match=SHAPE):
            hb.layernorm_fwd_fp8(x, g, b, 1e-12)
        with pytest.raises(RuntimeError, match=SHAPE):
            hb.layernorm_bwd_fp8(x, x, stats, g, amax_slots=_slots())
        with pytest.raises(RuntimeError, match=SHAPE):
            hb.layernorm_bwd_fp8(x, x, stats, g, amax_slots=_slots(), want8=False)
        # ANY fp8 argument: a copy or a history alone too, with and without dropout, with and without dx_drop (the generic kernels
        # these shapes run know no copy and store dx_drop unconditionally)
        for kw in (dict(), dict(amax_prev=_bits(3.0), want8=False), dict(drop_p=0.25, seed=7, drop_stream=3),
                   dict(drop_p=0.25, seed=7, drop_stream=3, want_dx_drop=False),
                   dict(drop_p=0.25, seed=7, drop_stream=3, want_dx_drop=False, want_params=False)):
            with pytest.raises(RuntimeError, match=SHAPE):
                hb.layernorm_bwd_fp8(x, x, stats, g, **kw)
        for kw in (dict(amax_slots=_slots(), want8=False), dict(amax_prev=_bits(3.0), want8=False)):
            with pytest.raises(RuntimeError, match=SHAPE):
                hb.layernorm_fwd_fp8(x, g, b, 1e-12, **kw)
        # ... while the same shapes pass with nothing requested
        _bytes_equal("refusals: %s H=%d plain" % (dtype, H_), hb.layernorm_fwd_fp8(x, g, b, 1e-12, want8=False)[0], y)
    # LayerNorm backward writes its copy only where it records: a copy or a history without the slot block is refused, not a silent
    # no-op (fast-path shape; with and without dropout, with dx_drop = NULL)
    x, g = tk.rnd(8, 256, dtype=BF, seed=31), torch.ones(256, device=DEV)
    stats = hb.layernorm_fwd(x, g, torch.zeros_like(g), 1e-12)[1]
    for kw in (dict(), dict(amax_prev=_bits(3.0)), dict(amax_prev=_bits(3.0), want8=False), dict(drop_p=0.25, seed=7, drop_stream=3),
               dict(drop_p=0.25, seed=7, drop_stream=3, want_dx_drop=False)):
        with pytest.raises(RuntimeError, match=ARG):
            hb.layernorm_bwd_fp8(x, x, stats, g, **kw)
    with pytest.raises(RuntimeError, match=ARG):         # dropout without dx_drop and without a copy: nothing to write the masked gradient to
        hb.layernorm_bwd_fp8(x, x, stats, g, drop_p=0.25, seed=7, drop_stream=3, want_dx_drop=False, want8=False, amax_slots=_slots())
    S = 17
    pr = dp._attn_problem(F32, 37, 0.2)
    ctx, lse = hb.attention_fwd(pr.qkv, pr.mask, B, 37, HEADS)
    for kw in (dict(), dict(want8=False, amax_slots=_slots()), dict(want8=False, amax_prev=_bits(3.0))):
        with pytest.raises(RuntimeError, match=SHAPE):
            hb.attention_fwd_fp8(pr.qkv, pr.mask, B, 37, HEADS, **kw)
        with pytest.raises(RuntimeError, match=SHAPE):
            hb.attention_bwd_fp8(pr.qkv, pr.mask, ctx, pr.dctx, lse, B, 37, HEADS, **kw)
    _bytes_equal("refusals: fp32 attention plain", hb.attention_fwd_fp8(pr.qkv, pr.mask, B, 37, HEADS, want8=False)[0], ctx)
    pb = dp._attn_problem(BF, S, 0.0)
    cb, lb = hb.attention_fwd(pb.qkv, pb.mask, B, S, HEADS)
    with pytest.raises(RuntimeError, match=ARG):         # neither dqkv nor a copy: nothing to write
        hb.attention_bwd_fp8(pb.qkv, pb.mask, cb, pb.dctx, lb, B, S, HEADS, want8=False, want_dqkv=False)
    x = tk.rnd(20, dtype=BF, seed=9)
    with pytest.raises(RuntimeError, match=ARG):
        hb.cast_fp8_scaled(x, amax_slots=_slots())
    with pytest.raises(RuntimeError, match=ARG):
        hb.amax_bf16(x, _slots())
    with pytest.raises(RuntimeError, match=ARG):
        hb.check(hb.lib().nbest_amax_bf16(hb.ptr(x[:16]), 16, hb.ptr(None), hb.stream_ptr()), "amax_bf16")
    with pytest.raises(RuntimeError, match=ARG):
        hb.check(hb.lib().nbest_amax_bf16(hb.ptr(None), 16, hb.ptr(_slots()), hb.stream_ptr()), "amax_bf16")
