"""The SAM / ASAM weight-space kernels' fp64 restatement and fp32 reference legs (nbest_sam_norms, nbest_sam_perturb,
nbest_sam_restore: csrc/sam.hip), on the hand-built descriptor table of tests/optim_ref.py.

One module, read by tests/test_sam_cpu.py (no GPU: the restatement against the closed form of a quadratic, ASAM's scale invariance,
and how far an fp32 restatement of the adaptive block sums is from fp64 - where the kernel test's bar comes from) and by
tests/test_sam_gpu.py (which runs the kernels).  torch / numpy on the CPU only.

* ``sam_reference(tab, p, g, rho, eta=None, norm=None)``: the step w -> w + e of include/nbest_hip.h's K9s in fp64 from the fp32
  arenas.  eta None: plain, e = s g; else adaptive, t = |p| + float32(eta), e = s t^2 g.  The scale s is an INPUT of the element
  arithmetic, as the clip coefficient is in optim_ref.ref_step: without ``norm`` it is rho / (||g|| + 1e-12) (adaptive: ||t g||) in
  fp64; with ``norm`` (the fp32 number the device left in clip[1]) it is formed as the kernel states it,
  float32(rho) / (norm + 1e-12f) in IEEE fp32 (one correctly rounded addition, one correctly rounded division - no freedom), so
  that the per-element bound judges the fma alone.  rho == 0, a norm that is 0 or not finite: s = 0.
* ``adaptive_partials``: the fp64 block sums of (t g)^2, 0 for the blocks of the inactive tensor.
* ``adaptive_leg_ratios``: the same block sums in fp32 (every product and every addition rounded) in several summation orders,
  against fp64: the worst relative error in units of 2^-24.  ``ASAM_LEG_WORST`` records it (tests/test_sam_cpu.py fails when a
  leg exceeds it) and ``ASAM_PARTIAL_K`` = 4 x that, rounded up, is the kernel test's bar - never taken from the kernels.
"""
import math
from collections import namedtuple

import numpy as np
import torch

import optim_ref as R

EPS = R.EPS
RHO, ASAM_RHO, ETA = 0.05, 0.5, 0.01            # the kernel tests' radii: the issue's rho for plain SAM, ASAM's usual 10 x, its default eta

SamRef = namedtuple("SamRef", "p e s norm")


def _blocks(t):
    return (t.numel + R.CHUNK - 1) // R.CHUNK


def state(tab):
    """the fp32 weights of optim_ref.state (guard-filled; every 7th element of a tensor exactly 0) and the gradient of
    optim_ref.grad(tab, 100): shared, never written"""
    return R.state(tab)[0], R.grad(tab, 100)


def adaptive_partials(tab, p, g, eta):
    """fp64 [n_blocks]: sum over the block of ((|p| + float32(eta)) g)^2; 0 for the blocks of inactive tensors"""
    out = torch.zeros(tab.n_blocks, dtype=torch.float64)
    for t in tab.tensors:
        if not t.active:
            continue
        s = slice(t.offset, t.offset + t.numel)
        x = ((p[s].double().abs() + R.f32(eta)) * g[s].double()) ** 2
        for b in range(_blocks(t)):
            out[t.block_start + b] = x[b * R.CHUNK:(b + 1) * R.CHUNK].sum()
    return out


def fp32_scale(rho, norm):
    """s as sam_perturb_kernel forms it, in IEEE fp32; ``norm``: the device's fp32 number"""
    norm = np.float32(norm)
    if not (rho > 0.0 and norm > 0.0 and np.isfinite(norm)):
        return 0.0
    return float(np.float32(rho) / np.float32(norm + np.float32(1e-12)))


def sam_reference(tab, p, g, rho, eta=None, norm=None):
    """SamRef(p' fp64 [total] (guards, gaps and the inactive tensor: p), e fp64 [total] (0 there), s, the norm used)"""
    p64, g64 = p.double(), g.double()
    act = R.covered(tab, active_only=True)
    t = None if eta is None else p64.abs() + R.f32(eta)
    if norm is None:
        x = g64 if eta is None else t * g64
        norm = math.sqrt((x[act] ** 2).sum().item())
        s = rho / (norm + 1e-12) if (rho > 0.0 and norm > 0.0 and math.isfinite(norm)) else 0.0
    else:
        s = fp32_scale(rho, norm)
    e = torch.zeros_like(p64)
    if s != 0.0:
        e[act] = (s * g64 if eta is None else s * (t * t) * g64)[act]
    return SamRef(p64 + e, e, s, float(norm))


# ---- the adaptive block sums in fp32: where the kernel test's bar comes from ----------------------------------------------------------
def _terms32(p, g, eta):
    """(t g)^2 with every operation rounded to fp32: t = |p| + eta, x = t g, x x"""
    x = (p.abs() + np.float32(eta)) * g
    return (x * x).numpy()


def _sum_orders(x):
    """fp32 sums of one block's terms in the orders a 256-lane reduction of a chunk can take (every addition rounded to fp32; one
    16 384-long chain is not among them: no workgroup adds that way, and its error, > 100 x 2^-24 here, would only widen the bar)"""
    seq = lambda v: float(np.cumsum(v, dtype=np.float32)[-1]) if v.size else 0.0
    out = {}
    # the scalar path's shape: lane i adds elements i, i + 256, ...; then the lanes' totals, forwards and backwards
    pad = np.zeros((-x.size) % 256, dtype=np.float32)
    lanes = np.cumsum(np.concatenate([x, pad]).reshape(-1, 256), axis=0, dtype=np.float32)[-1]
    out["lanes256"], out["lanes256_rev"] = seq(lanes), seq(lanes[::-1])
    # ... and on the float4 path: a tree of depth 2 per four elements, lane i takes the float4 i, i + 256, ...
    pad = np.zeros((-x.size) % 1024, dtype=np.float32)
    q = np.concatenate([x, pad]).reshape(-1, 256, 4)
    quad = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    out["float4"] = seq(np.cumsum(quad, axis=0, dtype=np.float32)[-1])
    out["float4_tree"] = float(torch.from_numpy(np.cumsum(quad, axis=0, dtype=np.float32)[-1].copy()).sum())
    out["pairwise"] = float(torch.from_numpy(np.ascontiguousarray(x)).sum())
    return out


def adaptive_leg_ratios(tab, p, g, eta):
    """{order: worst |fp32 block sum - fp64| / fp64 over the blocks of the active tensors, in units of 2^-24}"""
    ref = adaptive_partials(tab, p, g, eta)
    worst = {}
    for t in tab.tensors:
        if not t.active or t.gnorm == 0.0:
            continue
        x = _terms32(p[t.offset:t.offset + t.numel], g[t.offset:t.offset + t.numel], eta)
        for b in range(_blocks(t)):
            want = ref[t.block_start + b].item()
            for order, got in _sum_orders(x[b * R.CHUNK:(b + 1) * R.CHUNK]).items():
                worst[order] = max(worst.get(order, 0.0), abs(got - want) / want / EPS)
    return worst


# What adaptive_leg_ratios measured on (state(tab), ETA), rounded up to one decimal (tests/test_sam_cpu.py asserts that no order
# exceeds it); the kernel test's bar on partial[blk] is 4 x that: the device's fma contraction and its own order inside a wave.
ASAM_LEG_WORST = 11.4                           # lanes256 9.28, lanes256_rev 10.40, float4 11.37, float4_tree 2.09, pairwise 2.24
ASAM_PARTIAL_K = math.ceil(4 * ASAM_LEG_WORST)  # 46
