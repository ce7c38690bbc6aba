#!/usr/bin/env python3
"""the cost of the attention-map outputs: the eval forward (model.eval(), plain tensors) with and without return_attns, and
predict with and without return_attns, alternately in one process on the same seeded batches, timed with device events.

Per shape: ms per batch of each leg (median over rounds, min..max as the spread), the ratio of each pair, the bytes of maps each
attention leg writes and the rate they leave at (map bytes / the leg's extra time).

    python tools/attn_probs_bench.py [--rounds 7] [--iters 5] [--only NAME]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, synth
from nbest_amd.model import NBestSTCModel

SHAPES = [("bert-base bf16 B256 S128", ncfg.bert_base, torch.bfloat16, 256, 128),
          ("xlm-roberta-large bf16 B64 S256", ncfg.xlmr_large, torch.bfloat16, 64, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default=None, help="run the shapes whose name contains this string")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    print("%-34s %-14s %10s %18s %12s" % ("shape", "leg", "ms/batch", "spread ms", "maps GB"))
    opt = type("O", (), {})()
    for name, mk, dtype, B, S in SHAPES:
        if args.only and args.only not in name:
            continue
        cfg = mk(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=0.0, seed=1)
        m.load_reference_state(synth.model_state(cfg, labels, seed=1))
        m.eval()
        batches = []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
        seg = lambda b: b["seg"] if cfg.family == "bert" else None
        legs = {"eval": lambda b: m(opt, b["ids"], seg_ids=seg(b)),
                "eval+attns": lambda b: m(opt, b["ids"], seg_ids=seg(b), return_attns=True),
                "predict": lambda b: m.predict(b["ids"], seg_ids=seg(b)),
                "predict+attns": lambda b: m.predict(b["ids"], seg_ids=seg(b), return_attns=True)}
        L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
        maps = {"eval": 0, "eval+attns": L * B * heads * S * S * 4, "predict": 0, "predict+attns": L * B * heads * S * 4}
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn(batches[0])
                t0.record()
                for i in range(args.iters):
                    fn(batches[i % 2])
                t1.record()
                t1.synchronize()
                times[leg].append(t0.elapsed_time(t1) / args.iters)
        med = {leg: statistics.median(t) for leg, t in times.items()}
        for leg in legs:
            print("%-34s %-14s %10.3f %8.3f..%-8.3f %12.3f" % (name, leg, med[leg], min(times[leg]), max(times[leg]), maps[leg] / 1e9))
        for base in ("eval", "predict"):
            extra = med[base + "+attns"] - med[base]
            rate = maps[base + "+attns"] / (extra * 1e-3) / 1e12 if extra > 0 else float("inf")
            print("%-34s %s+attns / %s = %.3f (+%.3f ms, maps leave at %.2f TB/s of that)" % (
                name, base, base, med[base + "+attns"] / med[base], extra, rate))
        del m, batches, legs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
