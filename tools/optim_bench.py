#!/usr/bin/env python3
"""time the three fused optimizers on a bert-base-sized arena (109.6 M parameters, bf16 compute copy): BertAdam
(nbest_bertadam_*), torch Adam and HF AdamW (nbest_adam_*), run alternately in one process with device events.

Per optimizer: the whole step over both descriptor tables (block norms + clip coefficient + update, as HipBertAdam / HipAdam
launch it, without the transposed / packed weight refresh that follows every optimizer alike) and the update launches alone.
Bytes come from the shapes: the norms read g (4 B per trainable parameter); the update reads p, g, m, v and writes p, m, v
and the bf16 copy (30 B).  Share of HBM peak against 8 TB/s (MI355X).

    python tools/optim_bench.py [--rounds 15] [--iters 10] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb
from nbest_amd.arena import ParamArena

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    a = ParamArena(ncfg.bert_base(), labels, "cuda", compute_dtype=torch.bfloat16)
    gen = torch.Generator(device="cuda").manual_seed(0)
    a.p.copy_(torch.randn(a.total, generator=gen, device="cuda") * 0.02)
    a.g.copy_(torch.randn(a.total, generator=gen, device="cuda") * 1e-3)
    a.m, a.v = torch.zeros_like(a.p), torch.zeros_like(a.p)
    L = hb.lib()
    is_emb = lambda n: n.startswith("bert_encoder.embeddings.")
    tables = {}
    for kind in ("bertadam", "adam", "adamw"):
        tabs = []
        for sel in (lambda n: not is_emb(n), is_emb):
            d, n_t, n_b = a.build_descs(5e-4, 5e-4 if kind == "adam" else 1e-5, select=sel, wd=1e-4 if kind == "adam" else None)
            tabs.append((d, n_t, n_b))
        tables[kind] = tabs
    n_total_blocks = sum(t[2] for t in tables["adam"])
    partial = torch.zeros(n_total_blocks, dtype=torch.float32, device="cuda")
    clip = torch.ones(2, dtype=torch.float32, device="cuda")
    coef = torch.zeros(4096, dtype=torch.float32, device="cuda")
    P = lambda t: hb.ptr(t)
    s = lambda: hb.stream_ptr()
    n_param = sum(x.numel for x in a.slots if "pooler" not in x.name)

    def bertadam_update():
        base = 0
        for d, n_t, n_b in tables["bertadam"]:
            hb.check(L.nbest_bertadam_update(P(a.p), P(a.g), P(a.m), P(a.v), P(a.w16), P(d), n_t, n_b, 0, n_b, P(partial[base:]), P(coef),
                                             0.5, 0.9, 0.999, 1e-6, 1.0, s()), "bertadam_update")
            base += n_b

    def norms(kind):
        base = 0
        for d, n_t, n_b in tables[kind]:
            hb.check(L.nbest_bertadam_norms(P(a.g), P(d), n_t, n_b, 0, n_b, P(partial[base:]), s()), "bertadam_norms")
            base += n_b

    def adam_update(kind):
        mode, bc1, bc2 = (hb.ADAM_L2, 0.1, 0.0316) if kind == "adam" else (hb.ADAMW, 1.0, 1.0)
        for d, n_t, n_b in tables[kind]:
            hb.check(L.nbest_adam_update(mode, P(a.p), P(a.g), P(a.m), P(a.v), P(a.w16), P(d), n_t, n_b, 0, n_b, P(clip), 0.5, bc1, bc2,
                                         0.9, 0.999, 1e-8 if kind == "adam" else 1e-6, s()), "adam_update")

    def adam_step(kind):
        norms(kind)
        hb.check(L.nbest_adam_clip_coef(P(partial), n_total_blocks, 5.0, P(clip), s()), "adam_clip_coef")
        adam_update(kind)

    cases = [("bertadam", "step", lambda: (norms("bertadam"), bertadam_update())),
             ("bertadam", "update", bertadam_update),
             ("adam", "step", lambda: adam_step("adam")),
             ("adam", "update", lambda: adam_update("adam")),
             ("adamw", "step", lambda: adam_step("adamw")),
             ("adamw", "update", lambda: adam_update("adamw"))]
    times = {(k, w): [] for k, w, _ in cases}
    for _, _, f in cases:                       # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):                # alternate: every optimizer sees the same clocks
        for k, w, f in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[(k, w)].append(e0.elapsed_time(e1) / args.iters * 1e3)
    assert torch.isfinite(a.p).all() and torch.isfinite(a.m).all() and torch.isfinite(a.v).all()
    res = dict(n_param=n_param, hbm_peak_tbs=HBM_PEAK / 1e12, rounds=args.rounds, iters=args.iters, kernels={})
    print("bert-base arena: %.1f M trainable parameters (pooler excluded), HBM peak %.1f TB/s" % (n_param / 1e6, HBM_PEAK / 1e12))
    print("%-9s %-7s %9s %9s %9s %9s %8s %9s" % ("optimizer", "what", "median us", "min us", "MB", "TB/s", "% peak", "vs bertadam"))
    for k, w, _ in cases:
        med, lo = statistics.median(times[(k, w)]), min(times[(k, w)])
        nbytes = (34 if w == "step" else 30) * n_param
        tbs = nbytes / (med * 1e-6) / 1e12
        ratio = med / statistics.median(times[("bertadam", w)])
        res["kernels"]["%s_%s" % (k, w)] = dict(median_us=round(med, 1), min_us=round(lo, 1), bytes=nbytes, tbs=round(tbs, 3),
                                                 share_of_peak=round(tbs * 1e12 / HBM_PEAK, 3), vs_bertadam=round(ratio, 3))
        print("%-9s %-7s %9.1f %9.1f %9.0f %9.2f %7.0f %% %9.3f" % (k, w, med, lo, nbytes / 1e6, tbs, 100 * tbs * 1e12 / HBM_PEAK, ratio))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fp:
            json.dump(res, fp, indent=1)


if __name__ == "__main__":
    main()
