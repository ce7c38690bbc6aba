#!/usr/bin/env python3
"""What R-Drop costs: the rdrop instantiation of the heads kernel beside the plain one, and the R-Drop step beside a plain step of
the same number of rows.

Kernel: hipabi.stc_heads against hipabi.stc_heads_rdrop (alpha 1), both on 512 CLS rows of H 768 (bf16), dropout 0.3, need_grad: the
two launches of each (forward + backward), many calls between two events, alternately, queued behind ~ 20 ms of GEMMs so that the
events bracket device time.

Step: train_step at bert-base bf16, S 128, n-best 5, BertAdam, dropout on (hidden 0.1, attention 0.1, heads 0.3): the R-Drop step on
256 utterances (rdrop_alpha 1: 512 rows after the duplication) against a plain step on 512 rows - the same encoder work, so the
difference is the new heads arithmetic plus the duplication (five concatenations and two device sorts); a plain step on 256 rows
for scale.  Alternately in one process on the same seeded batches, timed with device events: median over the rounds, min..max.

    python tools/rdrop_bench.py [--rounds 9] [--iters 10] [--layers 12] [--out profiles/rdrop_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb, synth
from nbest_amd.model import NBestSTCModel
from nbest_amd.optim import HipBertAdam
from nbest_amd.trainer import limit_host_threads, train_step


def timed(fn, iters, blocker=None):
    """ms per call between two device events.  ``blocker``: enqueued ahead of the first event - device work long enough for the host
    to queue all ``iters`` calls behind it, so that the events bracket back-to-back device time and not the host's launch rate"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
    if blocker is not None:
        blocker()
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    limit_host_threads()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    P, S = a.utterances, a.seq_len
    cfg = ncfg.bert_base(num_hidden_layers=a.layers)
    model = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.3, seed=999)
    model.load_reference_state(synth.model_state(cfg, labels, seed=1))
    model.train()
    optim = HipBertAdam(model, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=100000)

    # ---- the heads kernel alone ----------------------------------------------------------------------------------------------------
    B2, H = 2 * P, cfg.hidden_size
    gen = torch.Generator(device="cuda").manual_seed(3)
    dls = model.dls
    R, nb = dls.n_rows, labels.n_bottom
    hidden = torch.randn(B2, H, generator=gen, device="cuda").bfloat16()
    Wh, bh = model.arena.heads_wb()
    y = (torch.rand(B2, nb, generator=gen, device="cuda") < 0.02).float()
    dWh, dbh = torch.zeros(R, H, device="cuda"), torch.zeros(R, device="cuda")
    kw = dict(need_grad=True, drop_p=0.3, seed=5, drop_stream=900, dWh=dWh, dbh=dbh, ws=hb.heads_ws(B2, R, H, "cuda"))
    klegs = {"stc_heads": lambda i: hb.stc_heads(hidden, H, Wh, bh, dls, y, B2, H, **kw),
             "stc_heads_rdrop (alpha 1)": lambda i: hb.stc_heads_rdrop(hidden, H, Wh, bh, dls, y, 1.0, B2, H, **kw)}
    for fn in klegs.values():
        for i in range(20):
            fn(i)
    torch.cuda.synchronize()
    big = torch.randn(8192, 8192, device="cuda").bfloat16()

    def blocker():                             # ~ 20 ms of GEMMs: 200 calls take the host less than that to enqueue
        for _ in range(12):
            torch.mm(big, big)
    ktimes = {leg: [] for leg in klegs}
    for _ in range(a.rounds):
        for leg, fn in klegs.items():
            ktimes[leg].append(timed(fn, 200, blocker) * 1e3)
    say("K7, %d rows, H %d, R %d, bf16 CLS rows, dropout 0.3, forward + backward launches, queued behind ~ 20 ms of GEMMs so that the "
        "events bracket device time; %d rounds x 200 calls, alternating" % (B2, H, R, a.rounds))
    say("%-34s %10s %20s" % ("call", "us/call", "spread us"))
    for leg in klegs:
        say("%-34s %10.2f %9.2f..%-10.2f" % (leg, statistics.median(ktimes[leg]), min(ktimes[leg]), max(ktimes[leg])))
    k0, k1 = (statistics.median(ktimes[k]) for k in klegs)
    say("stc_heads_rdrop - stc_heads %+.2f us (%+.1f %%)" % (k1 - k0, 100 * (k1 - k0) / k0))
    del big

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def batches(B):
        out = []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            out.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
        return out
    small, large = batches(P), batches(B2)
    legs = {"plain, %d rows" % B2: lambda i: train_step(model, optim, large[i % 2]),
            "rdrop_alpha 1, %d utterances" % P: lambda i: train_step(model, optim, small[i % 2], rdrop_alpha=1.0),
            "plain, %d rows" % P: lambda i: train_step(model, optim, small[i % 2])}
    for fn in legs.values():                   # warm-up: buffers sized, kernels loaded, clocks up
        for i in range(4):
            fn(i)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, a.iters))
    say("")
    say("bert-base bf16, %d layers, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating" % (a.layers, S, a.rounds, a.iters))
    say("%-34s %10s %20s" % ("train_step", "ms/step", "spread ms"))
    for leg in legs:
        say("%-34s %10.3f %9.3f..%-10.3f" % (leg, statistics.median(times[leg]), min(times[leg]), max(times[leg])))
    m0, m1, m2 = (statistics.median(times[k]) for k in legs)
    say("the R-Drop step on %d utterances - the plain step on %d rows: %+.3f ms (%+.2f %%); it is %.2f x the plain step on %d rows"
        % (P, B2, m1 - m0, 100 * (m1 - m0) / m0, m1 / m2, P))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
