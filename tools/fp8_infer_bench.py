#!/usr/bin/env python3
"""predict() (the bf16 path of an fp8w model) against predict(fp8=True) on the SAME fp8w model, alternately in one process on the same
seeded batches, timed with device events; also one fp8_calibrate call, and max |d| of the final scores between the two legs.

Per shape: ms per batch of each leg (median over rounds, min..max as the spread) and fp8 / bf16.

    python tools/fp8_infer_bench.py [--rounds 9] [--iters 10] [--only NAME] [--leg bf16|fp8]

``--leg``: run that leg alone, without timing (a kernel trace of one leg at a time)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, synth
from nbest_amd.model import NBestSTCModel

SHAPES = [("bert-base fp8w B256 S128", ncfg.bert_base, 256, 128),
          ("xlm-roberta-large fp8w B64 S256", ncfg.xlmr_large, 64, 256)]


def timed(fn, batches, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(batches[0])
    t0.record()
    for i in range(iters):
        fn(batches[i % 2])
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="run the shapes whose name contains this string")
    ap.add_argument("--leg", default=None, choices=("bf16", "fp8"))
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    print("%d rounds x %d batches per leg, the legs alternating inside a round" % (args.rounds, args.iters))
    print("%-34s %-10s %10s %18s" % ("shape", "leg", "ms/batch", "spread ms"))
    for name, mk, B, S in SHAPES:
        if args.only and args.only not in name:
            continue
        cfg = mk(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, seed=1, fp8_forward=True)
        m.load_reference_state(synth.model_state(cfg, labels, seed=1))
        m.eval()
        batches = []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
        seg = lambda b: b["seg"] if cfg.family == "bert" else None
        legs = {"bf16": lambda b: m.predict(b["ids"], seg_ids=seg(b)),
                "fp8": lambda b: m.predict(b["ids"], seg_ids=seg(b), fp8=True),
                "calibrate": lambda b: m.fp8_calibrate(b["ids"], seg_ids=seg(b))}
        for b in batches:
            legs["calibrate"](b)
        if args.leg:
            for i in range(args.iters):
                legs[args.leg](batches[i % 2])
            torch.cuda.synchronize()
            continue
        dmax = max((legs["bf16"](b)["final"] - legs["fp8"](b)["final"]).abs().max().item() for b in batches)
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, batches, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in legs:
            print("%-34s %-10s %10.3f %8.3f..%-8.3f" % (name, k, med[k], min(times[k]), max(times[k])))
        print("%-34s fp8 / bf16 = %.3f (%.1f %% %s), one fp8_calibrate call = %.3f ms, max |d final| bf16 vs fp8 = %.3e" % (
            name, med["fp8"] / med["bf16"], 100 * abs(1 - med["fp8"] / med["bf16"]), "faster" if med["fp8"] < med["bf16"] else "SLOWER",
            med["calibrate"], dmax))
        del m, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
