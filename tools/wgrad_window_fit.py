#!/usr/bin/env python3
"""does a fuller grouped weight-gradient launch cost what today's 216-tile launch costs?  (premise of rolling 256-tile windows)

    tools/wgrad_window_fit.py [N] [K]   N rounds (default 9) of two grouped launches (nbest_wgrad_group, no K-splits), alternating, in one
                                        process on cold operands (three operand sets in rotation), each timed with its own event pair:
                                          6 x (3072 x 768) gradients = 216 tiles of 256 x 256 at K token rows (default 32 768)
                                          7 x (3072 x 768) gradients = 252 tiles
                                        prints every timing, the medians and the ratio (profiles/wgrad_window_fit.txt)
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import nbest_amd  # noqa
from nbest_amd import hipabi as hb
n = int(sys.argv[1]) if len(sys.argv) > 1 else 9
M = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
H, F = 768, 3072
r = lambda *s: (torch.randn(*s, device="cuda") * 0.5).bfloat16()
sets = [[(r(M, F), r(M, H)) for _ in range(7)] for _ in range(3)]
outs = [torch.empty(F, H, dtype=torch.float32, device="cuda") for _ in range(7)]
ev = lambda: torch.cuda.Event(enable_timing=True)
t = {6: [], 7: []}
for it in range(n + 2):
    s = sets[it % 3]
    for cnt in ((6, 7) if it % 2 == 0 else (7, 6)):          # which of the two goes first alternates too
        e0, e1 = ev(), ev()
        e0.record()
        hb.wgrad_group(s[:cnt], outs=outs[:cnt])
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            t[cnt].append(e0.elapsed_time(e1) * 1000.0)
        s = sets[(it + 1) % 3]                                # the second launch of a round reads another set: cold as well
med = lambda v: sorted(v)[len(v) // 2]
for cnt in (6, 7):
    print("%d x (%d x %d), %3d tiles, K = %d rows, us per launch: %s" % (cnt, F, H, cnt * 36, M, " ".join("%.1f" % v for v in t[cnt])))
m6, m7 = med(t[6]), med(t[7])
print("medians: 216 tiles %.1f us (min %.1f), 252 tiles %.1f us (min %.1f), ratio %.4f (break-even of the windows 256 / 216 = 1.185, gate 1.09)"
      % (m6, min(t[6]), m7, min(t[7]), m7 / m6))
