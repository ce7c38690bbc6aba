#!/usr/bin/env python3
"""time the weight-EMA kernels (nbest_ema_update, nbest_ema_exchange: K9e) on a bert-base-sized arena (109.6 M parameters, bf16
compute copy) next to the fused BertAdam step (nbest_bertadam_step: K9), run alternately in one process with device events.

Each case covers both descriptor tables, as the optimizer launches them.  Bytes come from the shapes, per trainable parameter:
BertAdam 34 B (the norms read g, the update reads p, g, m, v and writes p, m, v and the bf16 copy), the EMA update 12 B (reads
ema and p, writes ema), the exchange 18 B (reads and writes p and ema, writes the bf16 copy; it also moves the pooler, which is
not trainable: 0.6 M elements).  Share of HBM peak against 8 TB/s (MI355X).  By bytes the EMA update should take about 12 / 34
of the BertAdam step.

    python tools/ema_bench.py [--rounds 15] [--iters 10] [--out profiles/ema_bench.txt]"""
import argparse
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    a = ParamArena(ncfg.bert_base(), labels, "cuda", compute_dtype=torch.bfloat16)
    gen = torch.Generator(device="cuda").manual_seed(0)
    a.p.copy_(torch.randn(a.total, generator=gen, device="cuda") * 0.02)
    a.g.copy_(torch.randn(a.total, generator=gen, device="cuda") * 1e-3)
    a.m, a.v = torch.zeros_like(a.p), torch.zeros_like(a.p)
    a.ema = a.p.clone()
    L = hb.lib()
    is_emb = lambda n: n.startswith("bert_encoder.embeddings.")
    tables = []
    for sel in (lambda n: not is_emb(n), is_emb):
        d, n_t, n_b = a.build_descs(5e-4, 1e-5, select=sel)
        tables.append((d, n_t, n_b, torch.empty((n_b + n_t + 16) * 4, dtype=torch.uint8, device="cuda")))
    P, s = hb.ptr, hb.stream_ptr
    n_param = sum(x.numel for x in a.slots if "pooler" not in x.name)
    n_all = sum(x.numel for x in a.slots)

    def bertadam_step():
        for d, n_t, n_b, ws in tables:
            hb.check(L.nbest_bertadam_step(P(a.p), P(a.g), P(a.m), P(a.v), P(a.w16), P(d), n_t, n_b, 0.5, 0.9, 0.999, 1e-6, 1.0, P(ws),
                                           ws.numel(), s()), "bertadam_step")

    def ema_update():
        for d, n_t, n_b, _ in tables:
            hb.check(L.nbest_ema_update(P(a.ema), P(a.p), P(d), n_t, n_b, 0.01, s()), "ema_update")

    def ema_exchange():
        for d, n_t, n_b, _ in tables:
            hb.check(L.nbest_ema_exchange(P(a.p), P(a.ema), P(a.w16), P(d), n_t, n_b, s()), "ema_exchange")

    cases = [("bertadam_step", bertadam_step, 34 * n_param), ("ema_update", ema_update, 12 * n_param),
             ("ema_exchange", ema_exchange, 18 * n_all)]
    assert args.iters % 2 == 0, "an even number of exchanges leaves the arenas as they were"
    times = {k: [] for k, _, _ in cases}
    for _, f, _ in cases:                       # warm-up
        for _ in range(4):
            f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):                # alternate: every kernel sees the same clocks
        for k, f, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.iters * 1e3)
    assert torch.isfinite(a.p).all() and torch.isfinite(a.ema).all()
    lines = ["bert-base arena: %.1f M trainable parameters (pooler excluded), HBM peak %.1f TB/s; %d rounds x %d calls, alternating, "
             "device events; both descriptor tables per call" % (n_param / 1e6, HBM_PEAK / 1e12, args.rounds, args.iters),
             "%-14s %9s %9s %9s %9s %8s %16s" % ("kernel", "median us", "min us", "MB", "TB/s", "% peak", "vs bertadam_step")]
    base = statistics.median(times["bertadam_step"])
    for k, _, nbytes in cases:
        med, lo = statistics.median(times[k]), min(times[k])
        tbs = nbytes / (med * 1e-6) / 1e12
        lines.append("%-14s %9.1f %9.1f %9.0f %9.2f %7.0f %% %16.3f" % (k, med, lo, nbytes / 1e6, tbs, 100 * tbs * 1e12 / HBM_PEAK, med / base))
    lines.append("ema_update / bertadam_step: measured %.3f, by bytes 12 / 34 = %.3f" % (statistics.median(times["ema_update"]) / base, 12 / 34))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
