"""GPU: the optimizer kernels of csrc/optim.hip (nbest_bertadam_step / _norms / _update, nbest_adam_step / _clip_coef / _update) on the
hand-built table of tests/optim_ref.py, in guard-filled buffers: every element of m, v and p against the fp64 statement of the rule
(fed the clip coefficient the kernel itself produced), the block sums of squares and the coefficients against fp64, the bit-exact
contracts (guards, the inactive tensor, g, the bf16 copy, lr_mult = 0, run-to-run), the block-range form against the step form,
and the argument checks.  The bounds are tests/optim_ref.py's: K = 4 x the worst ratio of the reference's own fp32 arithmetic
(tests/test_optim_kernels_cpu.py), never what the kernels give."""
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

WS_GUARD = -4321.0
RANGES = ((0, 9), (9, 9), (9, 40), (40, 76))     # cut inside the 3-block (8..10) and the 65-block (11..75) tensor; one range empty


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Env:
    """the table on the device, the shared (never written) initial state and gradients, and the fp64 norms of each gradient"""

    def __init__(self):
        import nbest_amd  # noqa: F401
        from nbest_amd import hipabi as hb
        self.hb, self.L = hb, hb.lib()
        assert self.L.nbest_bertadam_chunk() == R.CHUNK
        self.tab = tab = R.table()
        arr = (hb.TensorDesc * len(tab.tensors))()
        for d, t in zip(arr, tab.tensors):
            d.offset, d.numel, d.lr, d.wd, d.active, d.block_start = t.offset, t.numel, t.lr, t.wd, t.active, t.block_start
        self.descs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        self.n_t, self.n_b = len(tab.tensors), tab.n_blocks
        self.state = R.state(tab)
        self.grads = [R.grad(tab, 100 + k) for k in range(len(R.LR_MULTS))]
        self.norms = {(k, mgn): R.ref_norms(tab, g, mgn) for k, g in enumerate(self.grads) for mgn in R.MAX_GRAD_NORMS}
        self.cov = R.covered(tab)
        self.act = R.covered(tab, active_only=True)

    def bufs(self, lowp=True, k=0):
        p, m, v = (x.clone().cuda() for x in self.state)
        low = torch.full((self.tab.total,), 7.0, dtype=torch.bfloat16, device="cuda") if lowp else None
        return dict(p=p, g=self.grads[k].cuda(), m=m, v=v, low=low)

    def ws(self, rule):
        """(ws with 8 guard floats behind the bytes the call is told about, ws_bytes)"""
        n = self.n_b + (self.n_t if rule == "bertadam" else 2)
        return torch.full((n + 8,), WS_GUARD, device="cuda"), 4 * n

    def step(self, rule, b, h, mgn, ws, ws_bytes):
        """the step form; returns its return code"""
        hb, L, P = self.hb, self.L, self.hb.ptr
        if rule == "bertadam":
            return L.nbest_bertadam_step(P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["low"]), P(self.descs), self.n_t, self.n_b,
                                         h.lr_mult, h.b1, h.b2, h.eps, mgn, P(ws), ws_bytes, hb.stream_ptr())
        return L.nbest_adam_step(MODES[rule], P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["low"]), P(self.descs), self.n_t,
                                 self.n_b, h.lr_mult, h.bc1, h.bc2s, h.b1, h.b2, h.eps, mgn, P(ws), ws_bytes, hb.stream_ptr())

    def coefs(self, rule, ws):
        """the coefficient of every tensor as the kernel left it in ws: coef [n_tensors] behind the partials, or clip[0] for all"""
        tail = ws[self.n_b:self.n_b + (self.n_t if rule == "bertadam" else 2)].cpu()
        return tail if rule == "bertadam" else tail[0].expand(self.n_t)

    def block_mask(self, lo, hi):
        """the elements of blocks [lo, hi)"""
        mask = torch.zeros(self.tab.total, dtype=torch.bool)
        for t in self.tab.tensors:
            for blk in range(max(lo, t.block_start), min(hi, t.block_start + (t.numel + R.CHUNK - 1) // R.CHUNK)):
                c0 = (blk - t.block_start) * R.CHUNK
                mask[t.offset + c0:t.offset + min(c0 + R.CHUNK, t.numel)] = True
        return mask


MODES = {"adam": 0, "adamw": 1}                   # include/nbest_hip.h NBEST_ADAM_L2 / NBEST_ADAMW


@pytest.fixture(scope="module")
def env():
    e = Env()
    assert MODES == {"adam": e.hb.ADAM_L2, "adamw": e.hb.ADAMW}
    return e


def _chain(env, rule, lowp, mgn):
    """three chained steps (lr_mult 0, 0.3, 0.7); per step the state before (CPU), the state after (CPU) and ws"""
    b, out = env.bufs(lowp), []
    for k, lr_mult in enumerate(R.LR_MULTS):
        b["g"] = env.grads[k].cuda()
        before = {n: b[n].cpu() for n in ("p", "m", "v")} | {"low": b["low"].cpu() if lowp else None}
        ws, ws_bytes = env.ws(rule)
        env.hb.check(env.step(rule, b, R.hyper(rule, k + 1, lr_mult), mgn, ws, ws_bytes), rule)
        torch.cuda.synchronize()
        after = {n: b[n].cpu() for n in ("p", "m", "v", "g")} | {"low": b["low"].cpu() if lowp else None}
        out.append((before, after, ws.cpu()))
    return out


@pytest.mark.parametrize("mgn", R.MAX_GRAD_NORMS)
@pytest.mark.parametrize("lowp", [True, False], ids=["lowp", "nolowp"])
@pytest.mark.parametrize("rule", R.RULES)
def test_step_matches_fp64_per_element(env, rule, lowp, mgn):
    """after each of three chained steps, every element of m, v and p of the active tensors against optim_ref.ref_step from the fp32
    state before the step and the coefficient read back from ws, within K[rule][q] x 2^-24 in optim_ref.ratios' units.  Bit-exact:
    guard elements and the inactive tensor in p, m, v and p_lowp, the gradient arena (the kernels read g, they do not scale it in
    place), p_lowp = bf16(p) on the active tensors (float4 and scalar path), p under lr_mult = 0 while m and v move, the guard
    behind ws_bytes, and a second run from the same inputs."""
    tab, K = env.tab, R.K[rule]
    runs = [_chain(env, rule, lowp, mgn) for _ in range(2)]
    for (_, a0, w0), (_, a1, w1) in zip(*runs):
        assert all(_same(a0[n], a1[n]) for n in ("p", "m", "v")) and _same(w0, w1), "two runs differ"
        assert not lowp or _same(a0["low"], a1["low"])
    worst = dict.fromkeys(R.QUANTITIES, 0.0)
    for k, (before, after, ws) in enumerate(runs[0]):
        h = R.hyper(rule, k + 1, R.LR_MULTS[k])
        assert _same(after["g"], env.grads[k]), "the gradient arena was written"
        assert _same(ws[-8:], torch.full((8,), WS_GUARD)), "ws written past ws_bytes"
        assert torch.isfinite(ws[:-8]).all()
        for n in ("p", "m", "v") + (("low",) if lowp else ()):
            assert _same(after[n][~env.act], before[n][~env.act]), "%s: guard elements or the inactive tensor written" % n
            assert torch.isfinite(after[n][env.act].float()).all(), n
        if lowp:
            assert _same(after["low"][env.act], after["p"].to(torch.bfloat16)[env.act]), "p_lowp is not bf16(p)"
        coefs = env.coefs(rule, ws)
        for t, c in zip(tab.tensors, coefs):
            s = slice(t.offset, t.offset + t.numel)
            if not t.active:
                continue
            ref = R.ref_step(rule, before["p"][s], env.grads[k][s], before["m"][s], before["v"][s], c.item(), t, h)
            for q, r in R.ratios(after["m"][s], after["v"][s], after["p"][s], ref).items():
                worst[q] = max(worst[q], r)
            if h.lr_mult == 0.0:
                assert _same(after["p"][s], before["p"][s]), "lr_mult = 0 moved p"
                assert not torch.equal(after["m"][s], before["m"][s]) and not torch.equal(after["v"][s], before["v"][s])
            elif t.numel > 8:
                assert not torch.equal(after["p"][s], before["p"][s])
    R.log("optim-kernel %-8s %-6s max_grad_norm %g: worst ratios in 2^-24 vs fp64  m %.2f (K %d)  v %.2f (K %d)  p %.2f (K %d)"
          % (rule, "lowp" if lowp else "nolowp", mgn, worst["m"], K["m"], worst["v"], K["v"], worst["p"], K["p"]))
    for q in R.QUANTITIES:
        assert worst[q] <= K[q], (rule, q, worst[q], K[q])


@pytest.mark.parametrize("mgn", R.MAX_GRAD_NORMS)
@pytest.mark.parametrize("rule", ["bertadam", "adam"])
def test_norms_and_coefficients_match_fp64(env, rule, mgn):
    """partial[blk] of sumsq_kernel against the fp64 block sum within (chain + 1) x 2^-24 relative.  The longest chain of additions a
    term passes through: float4 path 2 (the tree over a float4's squares) + 17 (the thread's sum: 16 float4 of a full chunk and one
    tail element of a ragged one) + 6 (wave_sum) + 4 (block_sum over the four waves) = 29; scalar path 64 + 6 + 4 = 74; + 1 for the
    squaring.  Every term is non-negative, so no cancellation enters.  Blocks of the inactive tensor and of the zero gradient are
    exactly 0.  coef[t] (BertAdam) and clip[0], clip[1] (Adam) within half that bound + 4 x 2^-24; exactly 1 with max_grad_norm <= 0,
    for the zero gradient and for norms below max_grad_norm; nothing non-finite."""
    tab = env.tab
    for k in range(len(R.LR_MULTS)):
        b = env.bufs(True, k)
        ws, ws_bytes = env.ws(rule)
        env.hb.check(env.step(rule, b, R.hyper(rule, k + 1, 0.5), mgn, ws, ws_bytes), rule)
        torch.cuda.synchronize()
        ws = ws.cpu().double()
        assert torch.isfinite(ws).all()
        partial, coef, clip, total = env.norms[(k, mgn)]
        worst = 0.0
        for i, t in enumerate(tab.tensors):
            for blk in range(t.block_start, t.block_start + (t.numel + R.CHUNK - 1) // R.CHUNK):
                want, got = partial[blk].item(), ws[blk].item()
                if not t.active or t.gnorm == 0.0:
                    assert want == 0.0 and got == 0.0, (t.numel, blk, got)
                    continue
                worst = max(worst, abs(got - want) / (R.partial_bound(t) * want))
                assert abs(got - want) <= R.partial_bound(t) * want, (t.numel, blk, got, want)
            if rule == "bertadam":
                got, want = ws[env.n_b + i].item(), coef[i].item()
                if mgn <= 0 or not t.active or t.gnorm < mgn:
                    assert got == 1.0 and want == 1.0, (t.numel, got)
                else:
                    assert 0.0 < got < 0.05 and abs(got - want) <= R.coef_bound(t) * want, (t.numel, got, want)
        if rule == "adam":
            c, n = ws[env.n_b].item(), ws[env.n_b + 1].item()
            assert abs(n - total) <= R.coef_bound() * total, (n, total)
            assert (c == 1.0 and clip == 1.0) if mgn <= 0 else (0.0 < c < 0.05 and abs(c - clip) <= R.coef_bound() * clip), (c, clip)
        R.log("optim-norms  %-8s max_grad_norm %g step %d: worst |partial - fp64| / bound %.3f" % (rule, mgn, k + 1, worst))


def _range_calls(env, rule, b, h, mgn, partial, coef):
    """the range form over RANGES; yields after the norms of each range (\"norms\", i) and after the update of each (\"update\", i)"""
    hb, L, P = env.hb, env.L, env.hb.ptr
    for i, (lo, hi) in enumerate(RANGES):
        hb.check(L.nbest_bertadam_norms(P(b["g"]), P(env.descs), env.n_t, env.n_b, lo, hi, P(partial), hb.stream_ptr()), "norms")
        torch.cuda.synchronize()
        yield "norms", i
    if rule != "bertadam":
        hb.check(L.nbest_adam_clip_coef(P(partial), env.n_b, mgn, P(coef), hb.stream_ptr()), "adam_clip_coef")
    for i, (lo, hi) in enumerate(RANGES):
        if rule == "bertadam":
            rc = L.nbest_bertadam_update(P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["low"]), P(env.descs), env.n_t, env.n_b, lo, hi,
                                         P(partial), P(coef), h.lr_mult, h.b1, h.b2, h.eps, mgn, hb.stream_ptr())
        else:
            rc = L.nbest_adam_update(MODES[rule], P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["low"]), P(env.descs), env.n_t, env.n_b,
                                     lo, hi, P(coef), h.lr_mult, h.bc1, h.bc2s, h.b1, h.b2, h.eps, hb.stream_ptr())
        hb.check(rc, "update")
        torch.cuda.synchronize()
        yield "update", i


@pytest.mark.parametrize("rule", R.RULES)
def test_range_form_is_the_step_form(env, rule):
    """what the sharded optimizer runs: `partial` zeroed, nbest_bertadam_norms over the ranges (cuts inside two multi-block tensors, one
    range empty), then the update per range (nbest_bertadam_update; for Adam nbest_adam_clip_coef + nbest_adam_update).  After the
    first range alone nothing outside its blocks has moved, in `partial` or in the arenas, and its own blocks hold the step form's
    bits; after all ranges p, m, v, p_lowp, partial and the coefficients are bit-equal to nbest_bertadam_step / nbest_adam_step"""
    mgn, h = 1.0, R.hyper(rule, 2, 0.3)
    want = env.bufs(True, 1)
    ws, ws_bytes = env.ws(rule)
    env.hb.check(env.step(rule, want, h, mgn, ws, ws_bytes), rule)
    torch.cuda.synchronize()
    b, first = env.bufs(True, 1), env.bufs(True, 1)
    partial = torch.zeros(env.n_b, device="cuda")
    coef = torch.full((env.n_t if rule == "bertadam" else 2,), WS_GUARD, device="cuda")
    lo, hi = RANGES[0]
    inside = env.block_mask(lo, hi).cuda()
    assert inside.any() and (env.block_mask(0, env.n_b) == env.cov).all()
    for what, i in _range_calls(env, rule, b, h, mgn, partial, coef):
        if what == "norms" and i == 0:
            assert _same(partial[lo:hi], ws[lo:hi]) and (_bits(partial[hi:]) == 0).all(), "norms wrote outside their range"
        if what == "update" and i == 0:
            for n in ("p", "m", "v", "low"):
                assert _same(b[n][~inside], first[n][~inside]), "%s: the update of blocks [%d, %d) wrote outside them" % (n, lo, hi)
                assert _same(b[n][inside], want[n][inside]), n
    assert _same(partial, ws[:env.n_b]) and _same(coef, ws[env.n_b:env.n_b + coef.numel()])
    for n in ("p", "m", "v", "low"):
        assert _same(b[n], want[n]), n
    assert not _same(b["p"], first["p"])


def test_refused_calls_change_nothing(env):
    """a workspace one byte short: NBEST_ERR_WORKSPACE; a range outside [0, n_blocks] or with blk_lo > blk_hi, or a mode that is
    neither NBEST_ADAM_L2 nor NBEST_ADAMW: NBEST_ERR_ARG; nothing is enqueued - every buffer keeps its bits, ws included"""
    hb, L, P, s = env.hb, env.L, env.hb.ptr, env.hb.stream_ptr
    ERR_ARG, ERR_WORKSPACE = -1, -6
    b = env.bufs(True)
    ws, ws_bytes = env.ws("bertadam")
    partial = torch.zeros(env.n_b, device="cuda")
    coef = torch.full((env.n_t,), WS_GUARD, device="cuda")
    keep = {n: x.clone() for n, x in b.items()} | dict(ws=ws.clone(), partial=partial.clone(), coef=coef.clone())
    hB, hA = R.hyper("bertadam", 1, 0.5), R.hyper("adam", 1, 0.5)
    arenas = (P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["low"]), P(env.descs), env.n_t, env.n_b)
    assert L.nbest_bertadam_step(*arenas, 0.5, hB.b1, hB.b2, hB.eps, 1.0, P(ws), 4 * (env.n_b + env.n_t) - 1, s()) == ERR_WORKSPACE
    assert "workspace" in hb.last_error()
    for mode in MODES.values():
        assert L.nbest_adam_step(mode, *arenas, 0.5, hA.bc1, hA.bc2s, hA.b1, hA.b2, hA.eps, 1.0, P(ws), 4 * (env.n_b + 2) - 1, s()) == ERR_WORKSPACE
    for mode in (-1, 2):
        assert L.nbest_adam_step(mode, *arenas, 0.5, hA.bc1, hA.bc2s, hA.b1, hA.b2, hA.eps, 1.0, P(ws), ws_bytes, s()) == ERR_ARG
        assert L.nbest_adam_update(mode, *arenas, 0, env.n_b, P(coef), 0.5, hA.bc1, hA.bc2s, hA.b1, hA.b2, hA.eps, s()) == ERR_ARG
    for lo, hi in ((5, 4), (-1, 3), (0, env.n_b + 1), (env.n_b + 1, env.n_b + 1)):
        assert L.nbest_bertadam_norms(P(b["g"]), P(env.descs), env.n_t, env.n_b, lo, hi, P(partial), s()) == ERR_ARG, (lo, hi)
        assert L.nbest_bertadam_update(*arenas, lo, hi, P(partial), P(coef), 0.5, hB.b1, hB.b2, hB.eps, 1.0, s()) == ERR_ARG, (lo, hi)
        assert L.nbest_adam_update(0, *arenas, lo, hi, P(coef), 0.5, hA.bc1, hA.bc2s, hA.b1, hA.b2, hA.eps, s()) == ERR_ARG, (lo, hi)
    torch.cuda.synchronize()
    now = dict(b, ws=ws, partial=partial, coef=coef)
    for n, x in keep.items():
        assert _same(now[n], x), n
