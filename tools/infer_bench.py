#!/usr/bin/env python3
"""the eval forward (forward_backward(need_grad=False): whole encoder with its activation stash, heads on the CLS rows) against
predict (nbest_encoder_infer: no stash, FFN-up without GELU', last layer on the CLS rows only), alternately in one process on the
same seeded batches, timed with device events.

Per shape: ms per batch and utterances per second of each leg (median over rounds, min..max as the spread), the peak allocated
bytes of each leg (torch.cuda.reset_peak_memory_stats before each, over the model's own allocations), and max |d| of the final
scores between the legs.

    python tools/infer_bench.py [--rounds 9] [--iters 10] [--only NAME] [--predict_only]"""
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
          ("bert-base f32 B256 S128", ncfg.bert_base, torch.float32, 256, 128),
          ("xlm-roberta-large bf16 B64 S256", ncfg.xlmr_large, torch.bfloat16, 64, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="run the shapes whose name contains this string")
    ap.add_argument("--predict_only", action="store_true", help="predict leg only, a few batches (for a kernel trace)")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    print("%-34s %-8s %10s %14s %18s %12s" % ("shape", "leg", "ms/batch", "utt/s", "spread ms", "peak MB"))
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
        legs = {"eval": lambda b: m.forward_backward(b["ids"], b["labels"], seg_ids=seg(b), need_grad=False),
                "predict": lambda b: m.predict(b["ids"], seg_ids=seg(b))}
        if args.predict_only:
            for _ in range(3):
                for b in batches:
                    legs["predict"](b)
            torch.cuda.synchronize()
            print("%-34s predict-only trace run done" % name)
            continue
        peak = {}
        for leg, fn in legs.items():           # first call of each leg: sizes its buffers; its peak is what the leg holds
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn(batches[0])
            torch.cuda.synchronize()
            peak[leg] = torch.cuda.max_memory_allocated() - base
        dmax = 0.0
        for b in batches:
            e, p = legs["eval"](b), legs["predict"](b)
            dmax = max(dmax, (e["final"] - p["final"]).abs().max().item())
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
        for leg in legs:
            med = statistics.median(times[leg])
            print("%-34s %-8s %10.3f %14.0f %8.3f..%-8.3f %12.1f" % (name, leg, med, B / med * 1e3, min(times[leg]), max(times[leg]),
                                                                   peak[leg] / 2**20))
        me, mp = statistics.median(times["eval"]), statistics.median(times["predict"])
        print("%-34s predict / eval = %.3f (%.1f %% faster), peak memory %.1f x smaller, max |d final| = %.3e" % (
            name, mp / me, 100 * (1 - mp / me), peak["eval"] / max(peak["predict"], 1), dmax))
        del m, batches, legs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
