"""The optimizer kernels' test table, fp64 references and fp32 reference legs (nbest_bertadam_*, nbest_adam_*: csrc/optim.hip).

One module, read by tests/test_optim_kernels_cpu.py (no GPU: how far the reference's own fp32 arithmetic is from fp64, which is
where the kernel test's bounds come from) and by tests/test_optim_kernels_gpu.py (which runs the kernels).  torch on the CPU only.

* ``table()``: a hand-built descriptor table in the manner of tests/test_ema_gpu.py::_table - guard elements around every tensor, the
  scalar path (offset % 4 != 0), ragged chunk tails, a tensor of 65 blocks (the 64-lane loop of clip_coef_kernel wraps), an inactive
  two-block tensor, per-tensor lr and wd, gradients whose norm is far above / far below max_grad_norm and one all-zero gradient.
* ``ref_step``: ONE step of a rule in fp64 from the fp32 state (p, g, m, v) of a tensor, following include/nbest_hip.h's formula for
  the rule.  The clip coefficient is an INPUT (the element arithmetic is judged apart from the norm) and the constants are those
  torch's kernels receive from the reference's Python floats: float32(b), float32(1 - b) with 1 - b formed in double, float32(eps),
  float32(lr lr_mult [/ bc1]).  ``ref_norms``: the fp64 block sums of squares, per-tensor and global coefficients.
* ``leg_step``: the same step in torch CPU fp32 ops in the reference's operation order (BertAdam: the body of
  oracle/bertadam.py::OracleBertAdam.step; Adam: torch.optim.Adam's single-tensor update; AdamW: HF AdamW(correct_bias=False)).
* ``ratios``: the errors of (m, v, p) against ``ref_step`` in units of 2^-24 of each quantity's own scale.
* ``K``: the kernel test's bound per rule and quantity, 4 x the leg's worst ratio, rounded up (``LEG_WORST``: measured by the CPU test,
  which fails when a leg exceeds its entry).
"""
import math
import os
from collections import namedtuple

import numpy as np
import torch

EPS = 2.0 ** -24
CHUNK = 16384                                   # nbest_bertadam_chunk(): elements per block
GUARD = 12345.678
NUMELS = (1, 3, 4, 255, 16383, 16384, 16385, 40000, 64 * CHUNK + 5)
UNALIGNED = (255, 40000)                        # offset % 4 != 0: the scalar path (one of them multi-block)
INACTIVE = 16385                                # two blocks
ZERO_GRAD = 16384                               # an active tensor whose gradient is all zero: coefficient exactly 1, partial exactly 0
LRS = (1e-3, 3e-5, 5e-4)
WDS = (0.01, 0.0)
NORMS = (30.0, 0.05)                            # L2 norm of a tensor's gradient: far above / far below max_grad_norm = 1
RULES = ("bertadam", "adam", "adamw")           # adam: NBEST_ADAM_L2, adamw: NBEST_ADAMW
QUANTITIES = ("m", "v", "p")

Tensor = namedtuple("Tensor", "offset numel lr wd active block_start gnorm")
Table = namedtuple("Table", "tensors n_blocks total")
Hyper = namedtuple("Hyper", "b1 b2 eps lr_mult bc1 bc2s")


def table():
    """Table(tensors, n_blocks, total): at least 4 guard elements before, between and after the tensors; total = buffer length"""
    off, blk, out = 64, 0, []
    for i, n in enumerate(NUMELS):
        off = (off + 3) // 4 * 4 + 4
        if n in UNALIGNED:
            off += 1 + (i % 3)
        gnorm = 0.0 if n == ZERO_GRAD else NORMS[i % 2]
        out.append(Tensor(off, n, LRS[i % 3], WDS[i % 2], int(n != INACTIVE), blk, gnorm))
        blk += (n + CHUNK - 1) // CHUNK
        off += n
    assert {t.offset % 4 for t in out if t.numel in UNALIGNED} == {1, 2} and all(t.offset % 4 == 0 for t in out if t.numel not in UNALIGNED)
    assert all(b.offset - (a.offset + a.numel) >= 4 for a, b in zip(out, out[1:])) and out[0].offset >= 4
    assert {t.wd for t in out if t.active} == set(WDS) and {t.gnorm for t in out if t.active} == set(NORMS) | {0.0}
    assert blk == 76 and out[-1].block_start + 65 == blk
    return Table(out, blk, off + 64)


def covered(tab, active_only=False):
    c = torch.zeros(tab.total, dtype=torch.bool)
    for t in tab.tensors:
        if t.active or not active_only:
            c[t.offset:t.offset + t.numel] = True
    return c


def _signs(n):
    """+1, -1, +1, ... for the elements 0, 7, 14, ... of a tensor"""
    return 1.0 - 2.0 * (torch.arange((n + 6) // 7) % 2).float()


def state(tab, seed=11):
    """guard-filled fp32 (p, m, v): p ~ 0.05 N(0, 1), m ~ 0.01 N(0, 1), v in [1e-8, 1e-4].  Every 7th element of a tensor has p
    exactly 0, where the update is the whole of the new p and its error is not hidden below |p|; there m and every gradient of
    ``grad`` share a sign, so that nothing cancels in m either and lr |u| is a fair scale for the error of the update"""
    gen = torch.Generator().manual_seed(seed)
    p, m, v = (torch.full((tab.total,), x) for x in (-GUARD, GUARD, 2 * GUARD))
    for t in tab.tensors:
        s = slice(t.offset, t.offset + t.numel)
        p[s] = torch.randn(t.numel, generator=gen) * 0.05
        p[t.offset:t.offset + t.numel:7] = 0.0
        m[s] = torch.randn(t.numel, generator=gen) * 0.01
        m[t.offset:t.offset + t.numel:7] = m[t.offset:t.offset + t.numel:7].abs() * _signs(t.numel)
        v[s] = torch.rand(t.numel, generator=gen) * 1e-4 + 1e-8
    return p, m, v


def grad(tab, seed):
    """guard-filled fp32 gradient: N(0, 1) scaled to the tensor's norm (the inactive tensor has one too: it must not be read)"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((tab.total,), 3 * GUARD)
    for t in tab.tensors:
        x = torch.randn(t.numel, generator=gen)
        x[::7] = x[::7].abs() * _signs(t.numel)
        g[t.offset:t.offset + t.numel] = x * (t.gnorm / x.double().norm().item()) if t.gnorm else 0.0
    return g


def f32(x):
    """the double that equals float32(x)"""
    return float(np.float32(x))


def hyper(rule, step, lr_mult, b1=0.9, b2=0.999):
    """``step``: 1-based.  adam: eps 1e-8 and bias corrections; bertadam / adamw: eps 1e-6, none"""
    if rule == "adam":
        return Hyper(b1, b2, 1e-8, lr_mult, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step))
    return Hyper(b1, b2, 1e-6, lr_mult, 1.0, 1.0)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "m v p m_scale p_scale")


def ref_step(rule, p, g, m, v, c, t, h):
    """one step of ``rule`` on one tensor in fp64 from its fp32 state; c: the clip coefficient (float), t: the Tensor, h: Hyper.
    m_scale = |b1 m0| + |(1 - b1) c g| (adam: + |(1 - b1) wd p|, the other term of the gradient its moments see) and
    p_scale = |p0| + lr |u| (lr |u| = |p_ref - p0|) are the denominators of ``ratios``"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    b1, b2, ob1, ob2, eps = f32(h.b1), f32(h.b2), f32(1.0 - h.b1), f32(1.0 - h.b2), f32(h.eps)
    wd, ge = f32(t.wd), float(c) * g
    m_scale = (b1 * m).abs() + (ob1 * ge).abs()
    if rule == "adam":
        if wd != 0.0:
            ge = ge + wd * p
            m_scale = m_scale + (ob1 * wd * p).abs()
        m1 = m + ob1 * (ge - m)
        v1 = b2 * v + ob2 * ge * ge
        p1 = p - f32(t.lr * h.lr_mult / h.bc1) * (m1 / (v1.sqrt() / f32(h.bc2s) + eps))
    else:
        m1 = b1 * m + ob1 * ge
        v1 = b2 * v + ob2 * ge * ge
        u = m1 / (v1.sqrt() + eps)
        if rule == "bertadam":
            if wd > 0.0:
                u = u + wd * p
            p1 = p - f32(t.lr * h.lr_mult) * u
        else:
            p1 = p - f32(t.lr * h.lr_mult) * u
            if wd > 0.0:
                p1 = p1 - f32(t.lr * h.lr_mult * t.wd) * p1
    return Ref(m1, v1, p1, m_scale, p.abs() + (p1 - p).abs())


def ref_norms(tab, g, max_grad_norm):
    """fp64: block sums of squares [n_blocks] (0 for the blocks of inactive tensors), the per-tensor coefficient
    min(1, max_grad_norm / (||g_t|| + 1e-6)) [n_tensors], the global coefficient and the total norm (coefficients 1 when
    max_grad_norm <= 0)"""
    partial = torch.zeros(tab.n_blocks, dtype=torch.float64)
    coef = torch.ones(len(tab.tensors), dtype=torch.float64)
    for i, t in enumerate(tab.tensors):
        if not t.active:
            continue
        x = g[t.offset:t.offset + t.numel].double()
        for b in range((t.numel + CHUNK - 1) // CHUNK):
            partial[t.block_start + b] = (x[b * CHUNK:(b + 1) * CHUNK] ** 2).sum()
        if max_grad_norm > 0:
            nb = (t.numel + CHUNK - 1) // CHUNK
            coef[i] = min(1.0, max_grad_norm / (math.sqrt(partial[t.block_start:t.block_start + nb].sum().item()) + f32(1e-6)))
    total = math.sqrt(partial.sum().item())
    return partial, coef, (min(1.0, max_grad_norm / (total + f32(1e-6))) if max_grad_norm > 0 else 1.0), total


# ---- fp32 legs: the reference's own operations, torch CPU ------------------------------------------------------------------------------
def leg_coefs(rule, tab, g, max_grad_norm):
    """the clip coefficient of every tensor (fp32 tensors of one element) as the reference computes it: bertadam per tensor
    (torch.nn.utils.clip_grad_norm_(p, max_norm) of optimization.py:270-271), adam / adamw one for all (clip_grad_norm_(params))"""
    one = torch.ones(())
    views = [g[t.offset:t.offset + t.numel] for t in tab.tensors]
    if max_grad_norm <= 0:
        return [one for _ in views]
    if rule == "bertadam":
        return [torch.clamp(max_grad_norm / (x.norm(2) + 1e-6), max=1.0) if t.active else one for x, t in zip(views, tab.tensors)]
    total = torch.stack([x.norm(2) for x, t in zip(views, tab.tensors) if t.active]).norm(2)
    return [torch.clamp(max_grad_norm / (total + 1e-6), max=1.0) for _ in views]


def leg_step(rule, p, g, m, v, c, t, h, float_formed=False):
    """one step on one tensor in torch CPU fp32, in place on p, m, v (g is not written); c: fp32 tensor.  float_formed (bertadam): the
    constants float32(1) - float32(b) the kernel used to form, instead of the float32(1 - b) torch receives"""
    ob1, ob2 = 1 - h.b1, 1 - h.b2
    if float_formed:
        ob1, ob2 = float(np.float32(1) - np.float32(h.b1)), float(np.float32(1) - np.float32(h.b2))
    grad = g * c
    if rule == "bertadam":                                  # oracle/bertadam.py::OracleBertAdam.step
        m.mul_(h.b1).add_(grad, alpha=ob1)
        v.mul_(h.b2).addcmul_(grad, grad, value=ob2)
        upd = m / (v.sqrt() + h.eps)
        if t.wd > 0.0:
            upd = upd + t.wd * p
        p.add_(upd, alpha=-(t.lr * h.lr_mult))
    elif rule == "adam":                                    # torch.optim.adam._single_tensor_adam
        if t.wd != 0:
            grad = grad.add(p, alpha=t.wd)
        m.lerp_(grad, ob1)
        v.mul_(h.b2).addcmul_(grad, grad, value=ob2)
        denom = (v.sqrt() / h.bc2s).add_(h.eps)
        p.addcdiv_(m, denom, value=-(t.lr * h.lr_mult / h.bc1))
    else:                                                   # transformers.AdamW.step, correct_bias=False
        m.mul_(h.b1).add_(grad, alpha=ob1)
        v.mul_(h.b2).addcmul_(grad, grad, value=ob2)
        denom = v.sqrt().add_(h.eps)
        p.addcdiv_(m, denom, value=-(t.lr * h.lr_mult))
        if t.wd > 0.0:
            p.add_(p, alpha=-(t.lr * h.lr_mult * t.wd))


# ---- error ratios --------------------------------------------------------------------------------------------------------------------
def _ratio(err, scale):
    """err / scale in units of 2^-24; where the scale is 0 the value must be exact (inf otherwise)"""
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return (r / EPS).max().item()


def ratios(got_m, got_v, got_p, ref):
    """worst |m - m_ref| / (|b1 m0| + |(1 - b1) g'|), |v - v_ref| / v_ref, |p - p_ref| / (|p0| + lr |u_ref|) over a tensor, in units
    of 2^-24"""
    return dict(m=_ratio((got_m.double() - ref.m).abs(), ref.m_scale), v=_ratio((got_v.double() - ref.v).abs(), ref.v),
                p=_ratio((got_p.double() - ref.p).abs(), ref.p_scale))


LR_MULTS = (0.0, 0.3, 0.7)                      # three chained steps; the first moves m and v only
MAX_GRAD_NORMS = (1.0, 0.0)


def run_legs(rule, tab, float_formed=False):
    """three chained steps of the fp32 leg from ``state`` on gradients ``grad(tab, 100 + k)``, for both max_grad_norm: the worst
    ratios against ``ref_step`` (fed the coefficient the leg computed) per quantity"""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for mgn in MAX_GRAD_NORMS:
        p, m, v = state(tab)
        for k, lr_mult in enumerate(LR_MULTS):
            g, h = grad(tab, 100 + k), hyper(rule, k + 1, lr_mult)
            coefs = leg_coefs(rule, tab, g, mgn)
            for t, c in zip(tab.tensors, coefs):
                if not t.active:
                    continue
                s = slice(t.offset, t.offset + t.numel)
                ref = ref_step(rule, p[s], g[s], m[s], v[s], c.item(), t, h)
                leg_step(rule, p[s], g[s], m[s], v[s], c, t, h, float_formed=float_formed)
                for q, r in ratios(m[s], v[s], p[s], ref).items():
                    worst[q] = max(worst[q], r)
    return worst


# What run_legs measured (tests/test_optim_kernels_cpu.py asserts that no leg exceeds its entry), rounded up to one decimal.
LEG_WORST = {
    "bertadam": dict(m=2.0, v=2.0, p=6.9),        # 1.94, 1.99, 6.84
    "adam": dict(m=2.5, v=3.2, p=8.8),            # 2.44, 3.10, 8.70
    "adamw": dict(m=2.0, v=2.1, p=7.4),           # 1.95, 2.05, 7.39
}
# The kernel test's bound factors: 4 x the leg (fma contraction, the device's divide and square root), rounded up.
K = {rule: {q: math.ceil(4 * w) for q, w in d.items()} for rule, d in LEG_WORST.items()}

# ---- the norm kernels' addition chains (csrc/optim.hip sumsq_kernel, common.h block_sum) -----------------------------------------------
# float4 path: a thread's 16 float4 of a full chunk (+ 1 scalar tail element of a ragged one) are each squared and added in a tree of
# depth 2, then to the thread's sum: 2 + 17 additions; wave_sum: 6 xor-shuffle additions; block_sum: 4 additions of the wave totals.
# scalar path: 64 elements per thread, s += g g.
CHAIN_VEC = 2 + 17 + 6 + 4
CHAIN_SCALAR = 64 + 6 + 4


def partial_bound(t):
    """relative bound of partial[blk] for a block of tensor t: every addition on the longest chain and the squaring round once, all
    terms are non-negative, so the relative error is at most (chain + 1) 2^-24 to first order"""
    return ((CHAIN_SCALAR if t.offset % 4 else CHAIN_VEC) + 1) * EPS


def coef_bound(t=None):
    """relative bound of coef[t] (t = None: the global clip[0], clip[1]): the square root halves the partials' bound; + 4 x 2^-24 for
    the sum of the block sums, the square root, + 1e-6 and the division"""
    chain = CHAIN_SCALAR if t is None or t.offset % 4 else CHAIN_VEC
    return 0.5 * (chain + 1) * EPS + 4 * EPS


# ---- the parity lines: printed by both tests (pytest -s shows them) and, when NBEST_OPTIM_PARITY_LOG names a file, appended to it -
# profiles/optim_parity.txt is the record of one such run
def log(line):
    print(line)
    path = os.environ.get("NBEST_OPTIM_PARITY_LOG")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")
