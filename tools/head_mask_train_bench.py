#!/usr/bin/env python3
"""What training under a head mask costs: train_step under set_head_mask(mask, trainable=True) beside the plain train_step, one
model, the same seeded batches.

bert-base bf16, S 128, n-best 5, BertAdam, dropout on (hidden 0.1, attention 0.1, heads 0.3).  The mask is the mixed mask of the
tests (two heads pruned and one gated 0.5 in every layer) and, for scale, an all-ones mask: under a trainable mask every stashed
layer runs nbest_head_gate_fwd into the stash's gctx region (one read and one write of [M][H]) and nbest_head_gate_bwd on dctx (one
read and - for the heads whose gate is not 1 - one write), so from byte counts alone a layer costs at most four [M][H] passes more.
The legs alternate in one process, timed with device events: median over the rounds, min..max.

    python tools/head_mask_train_bench.py [--rounds 9] [--iters 10] [--layers 12] [--out profiles/head_mask_train_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, synth
from nbest_amd.model import NBestSTCModel
from nbest_amd.optim import HipBertAdam
from nbest_amd.trainer import limit_host_threads, train_step


def timed(fn, iters):
    """ms per call between two device events"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def mixed_mask(L, heads):
    m = torch.ones(L, heads)
    for l in range(L):
        m[l, (3 * l + 1) % heads] = 0.0
        m[l, (5 * l + 4) % heads] = 0.0
        m[l, (2 * l + 7) % heads] = 0.5
    return m


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

    B, S = a.utterances, a.seq_len
    cfg = ncfg.bert_base(num_hidden_layers=a.layers)
    model = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.3, seed=999)
    model.load_reference_state(synth.model_state(cfg, labels, seed=1))
    model.train()
    optim = HipBertAdam(model, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=100000)
    batches = []
    for s in range(2):
        bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
        batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
    L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
    masks = {"no mask": None, "mixed_mask, trainable": mixed_mask(L, heads), "all-ones mask, trainable": torch.ones(L, heads)}
    step = lambda i: train_step(model, optim, batches[i % 2])

    def leg(mask):
        model.set_head_mask(mask, trainable=mask is not None)       # (outside the timed region: it copies the mask to the device)
        torch.cuda.synchronize()
        return timed(step, a.iters)

    act = {}
    for tag, mask in masks.items():            # warm-up: buffers sized, kernels loaded, clocks up
        model.set_head_mask(mask, trainable=mask is not None)
        for i in range(4):
            step(i)
        act[tag] = model._desc(B, S, 0).act_bytes
    torch.cuda.synchronize()
    times = {tag: [] for tag in masks}
    for _ in range(a.rounds):
        for tag, mask in masks.items():
            times[tag].append(leg(mask))
    M, H = B * S, cfg.hidden_size
    say("bert-base bf16, %d layers, B %d, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating" % (a.layers, B, S, a.rounds, a.iters))
    say("%-28s %10s %20s %14s" % ("train_step", "ms/step", "spread ms", "stash MiB"))
    for tag in masks:
        say("%-28s %10.3f %9.3f..%-10.3f %14.1f" % (tag, statistics.median(times[tag]), min(times[tag]), max(times[tag]), act[tag] / 2 ** 20))
    m0 = statistics.median(times["no mask"])
    for tag in list(masks)[1:]:
        m1 = statistics.median(times[tag])
        say("%s - no mask: %+.3f ms (%+.2f %%)" % (tag, m1 - m0, 100 * (m1 - m0) / m0))
    say("one [M][H] bf16 pass is %.1f MiB; the mask adds at most 4 of them per layer (2 forward, 2 backward): %.0f MiB per step over %d "
        "layers" % (M * H * 2 / 2 ** 20, 4 * a.layers * M * H * 2 / 2 ** 20, a.layers))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
