#!/usr/bin/env python3
"""What a LoRA step costs beside the full fine-tuning step, and what its two kernels reach.

bert-base bf16, B 256, S 128, n-best 5, BertAdam, dropout on (hidden 0.1, attention 0.1, heads 0.3).  Three models of the same
weights: the full fine-tune, LoRA r = 8 on query,value and on all six targets.  The train_step legs alternate in one process,
timed with device events: median over the rounds, min..max.  Then nbest_lora_grad and nbest_lora_merge alone, in us per call and in
GB/s of the bytes they must move: grad reads the dense gradient of the adapted blocks once (4 B per element); merge reads the
base copy (4 B) and writes the fp32 master and the bf16 copy (6 B).

    python tools/lora_bench.py [--rounds 7] [--iters 8] [--layers 12] [--rank 8] [--out profiles/lora_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, lora, synth
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rank", type=int, default=8)
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
    sd = synth.model_state(cfg, labels, seed=1)
    batches = []
    for s in range(2):
        bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
        batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
    legs = {"full fine-tune": None, "LoRA r=%d query,value" % a.rank: ("query", "value"), "LoRA r=%d all six" % a.rank: lora.TARGET_NAMES}
    steps, models = {}, {}
    for tag, targets in legs.items():
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.3, seed=999)
        m.load_reference_state(sd)
        m.train()
        if targets is not None:
            m.enable_lora(a.rank, 2.0 * a.rank, targets=targets)
        o = HipBertAdam(m, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=100000)
        models[tag] = m
        steps[tag] = (lambda m, o: lambda i: train_step(m, o, batches[i % 2]))(m, o)
        for i in range(4):                     # warm-up: buffers sized, kernels loaded, clocks up
            steps[tag](i)
    torch.cuda.synchronize()
    times = {tag: [] for tag in legs}
    for _ in range(a.rounds):
        for tag in legs:
            times[tag].append(timed(steps[tag], a.iters))
    say("bert-base bf16, %d layers, B %d, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating" % (a.layers, B, S, a.rounds, a.iters))
    say("%-28s %10s %20s %16s" % ("train_step", "ms/step", "spread ms", "trainable"))
    for tag in legs:
        m = models[tag]
        heads = sum(s.numel for s in m.arena.slots if s.name.startswith("clf."))
        n = heads + m.lora.n_trainable if m.lora is not None else sum(s.numel for s in m.arena.slots if "pooler" not in s.name)
        say("%-28s %10.3f %9.3f..%-10.3f %16d" % (tag, statistics.median(times[tag]), min(times[tag]), max(times[tag]), n))
    m0 = statistics.median(times["full fine-tune"])
    for tag in list(legs)[1:]:
        m1 = statistics.median(times[tag])
        say("%s - full: %+.3f ms (%+.2f %%)" % (tag, m1 - m0, 100 * (m1 - m0) / m0))
    say("")
    say("%-28s %-6s %10s %18s %10s %10s" % ("kernel (alone, 50 calls)", "", "us/call", "spread us", "MB moved", "GB/s"))
    for tag in list(legs)[1:]:
        m = models[tag]
        st = m.lora
        elems = sum(b.rows * b.cols for b in st.blocks)
        for name, fn, nbytes in (("grad", lambda i: st.project_grad(m.arena), 4 * elems), ("merge", lambda i: st.merge(m.arena), 10 * elems)):
            ts = [timed(fn, 50) * 1e3 for _ in range(a.rounds)]
            us = statistics.median(ts)
            say("%-28s %-6s %10.1f %8.1f..%-9.1f %10.1f %10.0f" % (tag, name, us, min(ts), max(ts), nbytes / 1e6, nbytes / us / 1e3))
    say("grad: 4 B read per adapted element (+ the tile partials: 1 / 64 of it per rank written and read back for dA, 1 / 256 for dB); "
        "merge: 4 B read, 4 + 2 B written")
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
