"""The dropout-on kernels against fp32 references that apply the SAME mask: attention forward / backward, LayerNorm backward,
embedding forward / backward.  The mask is tests/test_kernels_gpu.py::_keep_mask, the independent restatement of the counter-based
decision (element index m * N + n); with it known, drop(P) is deterministic and torch autograd on fp32 gives every value.

Attention: B = 4, heads = 3 (bh takes both parities), d = 64, drop_p = 0.2 (one case 0.1), seed 5, stream 9; key mask rows
  0 all ones | 1 last 9 keys masked (cut inside the last key block) | 2 first 5 keys only (whole key blocks masked) |
  3 holes, j % 3 != 1, and keys 0..31 masked when S > 40 (first key block masked) - no row is fully masked.
Sequence lengths and what they run with DROP = true (even S: one hash per key pair, odd S: one per element):
  key blocks  S          bf16 forward                     bf16 backward
  1           17, 32     attn_fwd_bf16_kernel<1,true>     attn_bwd2_bf16_kernel<1,.>
  2           33, 64     <2,true>                         attn_bwd2<2,.>
  3           80, 95     <3,true>                         attn_bwd2<3,.>
  4           97, 128    <4,true>                         attn_bwd3_bf16_kernel<4,.>
  5           130, 159   <5,true>                         attn_bwd2<5,.> (eight waves from here)
  6           161, 192   <6,true>                         attn_bwd2<6,.>
  7           193, 224   <7,true>                         attn_bwd2<7,.>
  8           225, 256   <8,true>                         attn_bwd2<8,.>
  9 .. 16     257, 290, 511, 512   attn_fwd_long_bf16_kernel   attn_bwd_long_bf16_kernel
  fp32        37, 130, 300         attn_fwd_f32_kernel         attn_bwd_f32_kernel + attn_bwd_f32_kv_kernel (two query blocks from S = 130)
Every bf16 case with S <= 256 runs twice: keepwords = False is the re-hashing backward (KB = false), keepwords = True takes the
forward's keep words into attention_bwd(keep=...) (KB = true).
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import nbest_amd  # noqa: E402,F401
from nbest_amd import hipabi as hb  # noqa: E402

import test_kernels_gpu as tk  # noqa: E402  (_keep_mask; close / rnd / tol_of / _log: one kernel_parity.log for all kernel tests)

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
B, HEADS = 4, 3
H = HEADS * 64
SEED, STREAM = 5, 9

BF16_S = [17, 32, 33, 64, 80, 95, 97, 128, 130, 159, 161, 192, 193, 224, 225, 256, 257, 290, 511, 512]
ATTN_CASES = ([(BF, S, 0.2, kw) for S in BF16_S for kw in ((False, True) if S <= 256 else (False,))]
              + [(BF, 128, 0.1, False), (BF, 128, 0.1, True)]
              + [(F32, S, 0.2, False) for S in (37, 130, 300)])
ATTN_IDS = ["%s-S%d-p%g-%s" % ("bf16" if d == BF else "f32", S, p, "keepwords" if kw else "rehash") for d, S, p, kw in ATTN_CASES]


def _exact(name, bad):
    """an exact (element-for-element) condition: ``bad`` marks the elements that break it"""
    n = int(bad.sum())
    tk._log("%-58s mismatches=%d of %d %s" % (name, n, bad.numel(), "OK" if n == 0 else "FAIL"))
    assert n == 0, "%s: %d of %d elements differ, first at %s" % (name, n, bad.numel(), bad.nonzero()[0].tolist())


def _key_mask(S):
    m = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    m[1, S - 9:] = 0
    m[2, 5:] = 0
    m[3] = (torch.arange(S, device=DEV) % 3 != 1).to(torch.uint8)
    if S > 40:
        m[3, :32] = 0
    assert bool((m.sum(1) > 0).all())                     # a row with no key at all is outside the kernels' contract
    return m


@functools.lru_cache(maxsize=None)
def _attn_problem(dtype, S, p):
    """inputs of a case and its fp32 reference (computed once, shared by the tests, never written to): P = softmax(Q K^T / 8 + mask),
    Pd = P . keep . scale, ctx = Pd V, and the gradients of <ctx, dctx> by autograd"""
    qkv = tk.rnd(B * S, 3 * H, dtype=dtype, seed=61)
    dctx = tk.rnd(B * S, H, dtype=dtype, seed=62)
    mask = _key_mask(S)
    keep, scale = tk._keep_mask(B * HEADS * S, S, p, SEED, STREAM)
    keep = keep.view(B, HEADS, S, S)
    qr = qkv.float().clone().requires_grad_(True)
    q, k, v = qr.reshape(B, S, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~mask.bool()[:, None, None, :], float("-inf"))
    P = torch.softmax(sc, -1)
    Pd = P * keep * scale
    ctx = (Pd @ v).permute(0, 2, 1, 3).reshape(B * S, H)
    ctx.backward(dctx.float())
    valid = mask.bool()[:, None, None, :].expand(B, HEADS, S, S)
    return types.SimpleNamespace(qkv=qkv, dctx=dctx, mask=mask, keep=keep, scale=scale, valid=valid, P=P.detach(), Pd=Pd.detach(),
                                 lse=torch.logsumexp(sc, -1).detach(), ctx=ctx.detach(), dqkv=qr.grad, drop=dict(drop_p=p, seed=SEED, drop_stream=STREAM))


def _unit_rows(t, g, n):
    """t [B, S, heads, 64] <- 0, then t[b, 64 g + c, h, c] = 1 for c < n"""
    t.zero_()
    c = torch.arange(n, device=DEV)
    t[:, 64 * g + c, :, c] = 1
    return t


def _fwd_applied(pr, S, want_keep):
    """the matrix drop(P) [B, heads, S, S] the forward applied, read back 64 key columns per run through a one-hot V: ctx_g[b, i, h, c] =
    drop(P)[b, h, i, 64 g + c] with no summation.  Also the lse (bit-equal over the runs: it does not depend on V)"""
    out = torch.zeros(B, HEADS, S, S, device=DEV)
    lse0 = None
    for g in range((S + 63) // 64):
        n = min(64, S - 64 * g)
        x = pr.qkv.clone()
        _unit_rows(x.view(B, S, 3, HEADS, 64)[:, :, 2], g, n)
        ctx, lse = hb.attention_fwd(x, pr.mask, B, S, HEADS, want_keep=want_keep, **pr.drop)[:2]
        c = ctx.view(B, S, HEADS, 64).permute(0, 2, 1, 3).float()
        out[..., 64 * g:64 * g + n] = c[..., :n]
        _exact("attn applied fwd: value columns past the last key stay 0", c[..., n:] != 0)
        if lse0 is None:
            lse0 = lse
        else:
            assert torch.equal(lse, lse0), "lse changed with V (run %d)" % g
    return out, lse0


def _bwd_applied(pr, S, keepwords):
    """the matrix the backward applied, through a one-hot dctx on the ctx / lse of a real forward: dV_g[b, j, h, c] =
    drop(P)[b, h, 64 g + c, j] (dV depends on nothing else)"""
    r = hb.attention_fwd(pr.qkv, pr.mask, B, S, HEADS, want_keep=keepwords, **pr.drop)
    ctx, lse = r[:2]
    keep = r[2] if keepwords else None
    assert not keepwords or keep is not None
    out = torch.zeros(B, HEADS, S, S, device=DEV)
    for g in range((S + 63) // 64):
        n = min(64, S - 64 * g)
        dctx = torch.empty(B * S, H, dtype=pr.qkv.dtype, device=DEV)
        _unit_rows(dctx.view(B, S, HEADS, 64), g, n)
        dqkv = hb.attention_bwd(pr.qkv, pr.mask, ctx, dctx, lse, B, S, HEADS, keep=keep, **pr.drop)
        dv = dqkv.view(B, S, 3, HEADS, 64)[:, :, 2].permute(0, 2, 3, 1).float()           # [b, h, c, j]
        out[:, :, 64 * g:64 * g + n, :] = dv[:, :, :n, :]
        _exact("attn applied bwd: dV columns past the last query stay 0", dv[:, :, n:, :] != 0)
    return out


def _check_applied(tag, got, pr, dtype):
    _exact(tag + " zero at masked keys", (got != 0) & ~pr.valid)
    _exact(tag + " nonzero == keep", ((got != 0) != pr.keep) & pr.valid)
    tk.close(tag + " values", got, pr.Pd, tk.tol_of(dtype))


@pytest.mark.parametrize("dtype,S,p,keepwords", ATTN_CASES, ids=ATTN_IDS)
def test_attention_applied_decisions(dtype, S, p, keepwords):
    """Test 1: the keep decision and the probability each kernel applies to every (query, key), read back exactly (no sum hides a
    single wrong element): zero at masked keys, (value != 0) == keep at every unmasked key of every query row, the values against
    softmax . keep . scale, lse independent of V and equal to the pre-dropout log-sum-exp."""
    pr = _attn_problem(dtype, S, p)
    # kept means nonzero only if no unmasked probability underflows: unit-normal Q, K keep them far above bf16's smallest normal
    assert pr.P[pr.valid].min().item() > 1e-30
    tag = "attn applied %s S=%d p=%g %s" % ("bf16" if dtype == BF else "f32", S, p, "kw" if keepwords else "rh")
    fwd, lse = _fwd_applied(pr, S, keepwords)
    _check_applied(tag + " fwd", fwd, pr, dtype)
    tk.close(tag + " lse", lse, pr.lse, tk.tol_of(dtype))
    _check_applied(tag + " bwd", _bwd_applied(pr, S, keepwords), pr, dtype)


@pytest.mark.parametrize("dtype,S,p,keepwords", ATTN_CASES, ids=ATTN_IDS)
def test_attention_dropout_values_and_grads(dtype, S, p, keepwords):
    """Test 2: ctx, lse, dQ, dK, dV and the fused bias gradient against autograd through Pd = softmax . keep . scale (tolerances of
    test_attention_fwd_bwd: tol, 2 tol on dQ / dK / dV, 5 tol on the column sums), then the bias gradient ADDED to a pre-filled
    vector (accumulate: partial_rows_sum on the bf16 path, colsum on the fp32 one)."""
    pr = _attn_problem(dtype, S, p)
    tol = tk.tol_of(dtype)
    tag = "attn drop %s S=%d p=%g %s" % ("bf16" if dtype == BF else "f32", S, p, "kw" if keepwords else "rh")
    r = hb.attention_fwd(pr.qkv, pr.mask, B, S, HEADS, want_keep=keepwords, **pr.drop)
    ctx, lse = r[:2]
    keep = r[2] if keepwords else None
    assert not keepwords or keep is not None
    tk.close(tag + " ctx", ctx, pr.ctx, tol)
    tk.close(tag + " lse", lse, pr.lse, tol)
    dbias = torch.zeros(3 * H, device=DEV)
    dqkv = hb.attention_bwd(pr.qkv, pr.mask, ctx, pr.dctx, lse, B, S, HEADS, dbias=dbias, keep=keep, **pr.drop)
    tk.close(tag + " fused bias grad", dbias, pr.dqkv.sum(0), 5 * tol)
    d, ref = dqkv.float().reshape(B * S, 3, H), pr.dqkv.reshape(B * S, 3, H)
    for i, nm in enumerate("QKV"):
        tk.close(tag + " d" + nm, d[:, i], ref[:, i], 2 * tol)
    pre = tk.rnd(3 * H, s=float(dbias.abs().max().item()), seed=63)
    acc = pre.clone()
    dqkv2 = hb.attention_bwd(pr.qkv, pr.mask, ctx, pr.dctx, lse, B, S, HEADS, dbias=acc, keep=keep, accumulate=True, **pr.drop)
    _exact(tag + " dqkv unchanged by accumulate", dqkv2.float() != dqkv.float())
    tk.close(tag + " bias grad accumulated", acc, pre + pr.dqkv.sum(0), 5 * tol)
    tk.close(tag + " bias grad accumulated = pre-fill + overwritten", acc, pre + dbias, 1e-6)        # one fp32 addition per element


# ------------------------------------------------------------------------------------------------
LN_P, LN_SEED, LN_STREAM = 0.25, 7, 3
# bf16 H = 256 .. 1024: ln_bwd_fast_kernel<V = 1 .. 4, DROP = true, .>; bf16 H = 320 and fp32: the generic ln_bwd_kernel
LN_CASES = [(BF, 256), (BF, 512), (BF, 768), (BF, 1024), (BF, 320), (F32, 768)]


@pytest.mark.parametrize("M", [37, 300])
@pytest.mark.parametrize("dtype,H_", LN_CASES, ids=["%s-H%d" % ("bf16" if d == BF else "f32", h) for d, h in LN_CASES])
def test_layernorm_bwd_dropout(dtype, H_, M):
    """Test 3: dx, dx_drop = dx . keep . scale, dgamma, dbeta and dbias = sum_m dx_drop under dropout against autograd of layer_norm;
    the same without the bias sum (DBIAS = false), and without any parameter output (PARAMS = false), whose dx / dx_drop must be the
    bits of the full call.  M = 37 / 300: 2 / 10 blocks with a ragged last one."""
    x = tk.rnd(M, H_, dtype=dtype, seed=31)
    g, b = 1 + 0.1 * tk.rnd(H_, seed=32), 0.1 * tk.rnd(H_, seed=33)
    dy = tk.rnd(M, H_, dtype=dtype, seed=34)
    _, stats = hb.layernorm_fwd(x, g, b, 1e-12)
    xr, gr, br = x.float().clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (H_,), gr, br, 1e-12).backward(dy.float())
    keep, scale = tk._keep_mask(M, H_, LN_P, LN_SEED, LN_STREAM)
    dxd_ref = xr.grad * keep * scale
    tol = tk.tol_of(dtype)
    not_tiny = xr.grad.abs() > tol * xr.grad.abs().max()          # an element within tol of the reference cannot be 0 there
    drop = dict(drop_p=LN_P, seed=LN_SEED, drop_stream=LN_STREAM)
    tag = "ln_bwd drop %s %dx%d" % ("bf16" if dtype == BF else "f32", M, H_)

    def check(tag, dx, dxd, dg, db):
        _exact(tag + " dx_drop zero where dropped", (dxd.float() != 0) & ~keep)
        _exact(tag + " dx_drop nonzero where kept", (dxd.float() == 0) & keep & not_tiny)
        tk.close(tag + " dx", dx, xr.grad, tol)
        tk.close(tag + " dx_drop", dxd, dxd_ref, tol)
        tk.close(tag + " dgamma", dg, gr.grad, 5 * tol)
        tk.close(tag + " dbeta", db, br.grad, 5 * tol)

    dx, dxd, dg, db, dbias = hb.layernorm_bwd(dy, x, stats, g, **drop)
    check(tag, dx, dxd, dg, db)
    tk.close(tag + " dbias", dbias, dxd_ref.sum(0), 5 * tol)
    dx1, dxd1, dg1, db1, none = hb.layernorm_bwd(dy, x, stats, g, want_dbias=False, **drop)
    assert none is None
    check(tag + " no dbias", dx1, dxd1, dg1, db1)
    dx0, dxd0, *sums = hb.layernorm_bwd(dy, x, stats, g, want_params=False, **drop)
    assert sums == [None, None, None]
    _exact(tag + " no params: dx bits", dx0.view(torch.uint8) != dx.view(torch.uint8))
    _exact(tag + " no params: dx_drop bits", dxd0.view(torch.uint8) != dxd.view(torch.uint8))


# ------------------------------------------------------------------------------------------------
EMB_P, EMB_SEED, EMB_STREAM = 0.1, 11, 2


@pytest.mark.parametrize("H_", [768, 1024, 320])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_embed_fwd_bwd_dropout(dtype, H_):
    """Test 4: the layout of test_embed_fwd_bwd (padding rows included) with drop_p = 0.1: out = LN(e) . keep . scale with keep over
    [B S, H] at element index m H + n - zero pattern exact, values close - and the table / gamma / beta gradients against autograd
    through the same masked expression."""
    Be, S, V = 3, 40, 500
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(2, V, (Be, S), generator=gen).to(DEV)
    ids[1, 30:] = 0
    ids[2, 20:] = 0                                          # padding rows (row 0 = padding_idx: no gradient)
    seg = (torch.arange(S)[None, :] > 12).long().expand(Be, S).contiguous().to(DEV)
    pos = torch.arange(S)[None, :].expand(Be, S).contiguous().to(DEV)
    word, tt, pt = (tk.rnd(V, H_, dtype=dtype, s=0.5, seed=51), tk.rnd(2, H_, dtype=dtype, s=0.5, seed=52),
                    tk.rnd(64, H_, dtype=dtype, s=0.5, seed=53))
    gam, bet = 1 + 0.1 * tk.rnd(H_, seed=54), 0.1 * tk.rnd(H_, seed=55)
    drop = dict(drop_p=EMB_P, seed=EMB_SEED, drop_stream=EMB_STREAM)
    out, stats = hb.embed_ln_fwd(ids, seg, pos, word, tt, pt, gam, bet, 1e-12, **drop)
    wr, tr, pr = (t.float().clone().requires_grad_(True) for t in (word, tt, pt))
    gr, br = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    e = torch.nn.functional.embedding(ids, wr, padding_idx=0) + tr[seg] + pr[pos]
    ln = torch.nn.functional.layer_norm(e, (H_,), gr, br, 1e-12).reshape(Be * S, H_)
    keep, scale = tk._keep_mask(Be * S, H_, EMB_P, EMB_SEED, EMB_STREAM)
    ref = ln * keep * scale
    tol = tk.tol_of(dtype)
    tag = "embed drop %s H=%d" % ("bf16" if dtype == BF else "f32", H_)
    # kept means nonzero only if no LayerNorm output is 0 to begin with: both sides compute xhat * gamma + beta in fp32 from the same
    # inputs, a few roundings of 2^-24 on terms below 4 (< 1e-6 in all), so a reference element above 1e-6 cannot come out as 0
    assert ln.detach().abs().min().item() > 1e-6
    _exact(tag + " fwd (out != 0) == keep", (out.float() != 0) != keep)
    tk.close(tag + " fwd", out, ref, tol)
    dout = tk.rnd(Be * S, H_, dtype=dtype, seed=56)
    ref.backward(dout.float())
    dword, dtt, dpt, dg, db = hb.embed_ln_bwd(ids, seg, pos, word, tt, pt, gam, stats, dout, Be, S, word_pad_id=0, **drop)
    for nm, got, want in (("dword", dword, wr.grad), ("dtype", dtt, tr.grad), ("dpos", dpt, pr.grad), ("dgamma", dg, gr.grad),
                          ("dbeta", db, br.grad)):
        tk.close(tag + " bwd " + nm, got, want, 5 * tol)
    assert dword[0].abs().max().item() == 0.0
