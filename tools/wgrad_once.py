#!/usr/bin/env python3
"""the 4 weight-gradient GEMM launches of one layer (for rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes)

    tools/wgrad_once.py [N]            N rounds of the four split-K launches of a layer (nbest_gemm)
    tools/wgrad_once.py N group [K]    per round: the grouped launch of TWO layers (nbest_wgrad_group, 8 problems, no K-splits) and the
                                       2 x 3 launches it replaces (FFN-down, FFN-up, QKV + attention-out paired; each GEMM + reduce),
                                       on cold operands (three operand sets in rotation), timed with events: us per LAYER, both ways
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import nbest_amd  # noqa
from nbest_amd import hipabi as hb
group = len(sys.argv) > 2 and sys.argv[2] == "group"
M = int(sys.argv[3]) if len(sys.argv) > 3 else 32768
H, F = 768, 3072
r = lambda *s: (torch.randn(*s, device="cuda") * 0.5).bfloat16()


def layer():
    x, big = r(M, H), r(M, F)
    return [(3 * H, H, r(M, 3 * H), x), (H, H, r(M, H), r(M, H)), (F, H, big, r(M, H)), (H, F, r(M, H), r(M, F))]


n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
if not group:
    shapes = layer()
    outs = [torch.empty(a, b, dtype=torch.float32, device="cuda") for a, b, _, _ in shapes]
    for it in range(n):
        for (a, b, dy, x), o in zip(shapes, outs):
            hb.gemm(dy, x, a, b, M, 1, 1, hb.EPI_F32_SPLITK, out=o)
    torch.cuda.synchronize()
    sys.exit(0)

sets = [layer() + layer() for _ in range(3)]
outs = [torch.empty(a, b, dtype=torch.float32, device="cuda") for a, b, _, _ in sets[0]]
ev = lambda: torch.cuda.Event(enable_timing=True)
tg, ts = [], []
for it in range(n + 2):
    s = sets[it % 3]
    e0, e1, e2 = ev(), ev(), ev()
    e0.record()
    hb.wgrad_group([(dy, x) for _, _, dy, x in s], outs=outs)
    e1.record()
    for l in (0, 4):
        for j in (3, 2):
            a, b, dy, x = s[l + j]
            hb.gemm(dy, x, a, b, M, 1, 1, hb.EPI_F32_SPLITK, out=outs[l + j])
        hb.wgrad_pair(s[l][2], s[l][3], s[l + 1][2], s[l + 1][3], out1=outs[l], out2=outs[l + 1])
    e2.record()
    torch.cuda.synchronize()
    if it >= 2:
        tg.append(e0.elapsed_time(e1) * 500.0)
        ts.append(e1.elapsed_time(e2) * 500.0)
med = lambda v: sorted(v)[len(v) // 2]
print("K = %d token rows, us per layer: grouped launch of two layers %.1f (min %.1f), three split-K launches + reduces %.1f (min %.1f)"
      % (M, med(tg), min(tg), med(ts), min(ts)))
