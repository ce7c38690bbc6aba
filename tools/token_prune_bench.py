#!/usr/bin/env python3
"""predict without and with token elimination (model.predict(token_keep=...)), alternately in one process on the same seeded
batches, timed with device events.

Schedules per shape: geometric S -> S/2, S -> S/4, S -> S/8 (trainer.token_keep_schedule), the S -> S/4 one with every entry rounded
up to a multiple of 16 and of 64 (whole GEMM row tiles), and "pad": batches whose longest utterance is 3 S / 4, padded to S, under
keep = 3 S / 4 - only padding goes.  Per schedule: ms per batch (median over rounds, min..max as the spread), the ratio to plain
predict, and what the row counts alone predict, sum_l S_l / (L S).  The gap between the two is the cost of score, select and gather
(timed alone below, one launch each at the full shape, k = S / 2) and of GEMM tiles cut by an odd row count.

    python tools/token_prune_bench.py [--rounds 9] [--iters 10] [--only NAME]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb, synth, trainer
from nbest_amd.model import NBestSTCModel

SHAPES = [("bert-base bf16 B256 S128", ncfg.bert_base, torch.bfloat16, 256, 128),
          ("xlm-roberta-large bf16 B64 S256", ncfg.xlmr_large, torch.bfloat16, 64, 256)]


def timed(fn, args, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(args[0])
    t0.record()
    for i in range(iters):
        fn(args[i % len(args)])
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def counts(S, keep):
    out = [S]
    for k in keep:
        out.append(min(k, out[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="run the shapes whose name contains this string")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    print("%d rounds x %d batches per leg, the legs alternating inside a round" % (args.rounds, args.iters))
    for name, mk, dtype, B, S in SHAPES:
        if args.only and args.only not in name:
            continue
        cfg = mk(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        L, heads, H = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.hidden_size
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=0.0, seed=1)
        m.load_reference_state(synth.model_state(cfg, labels, seed=1))
        m.eval()
        full, short = [], []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            full.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
            bt = synth.nbest_batch(cfg, labels, B, 3 * S // 4, n_best=5, seed=21 + s, ragged=True)
            pad = lambda a: np.concatenate([a, np.zeros((B, S - a.shape[1]), dtype=a.dtype)], 1)   # (XLM-R: id 0 is masked too, quirk Q1)
            short.append({k: torch.from_numpy(pad(bt[k])).cuda() for k in ("ids", "seg")})
        seg = lambda b: b["seg"] if cfg.family == "bert" else None
        up = lambda keep, q: [min(S, (k + q - 1) // q * q) for k in keep]
        quarter = trainer.token_keep_schedule(L, S, S // 4)
        legs = [("plain", None, full), ("S:S/2", trainer.token_keep_schedule(L, S, S // 2), full), ("S:S/4", quarter, full),
                ("S:S/8", trainer.token_keep_schedule(L, S, S // 8), full), ("S:S/4 x16", up(quarter, 16), full),
                ("S:S/4 x64", up(quarter, 64), full), ("pad plain", None, short), ("pad", [3 * S // 4] * (L - 1), short)]
        times = {k: [] for k, _, _ in legs}
        for _ in range(args.rounds):
            for k, keep, batches in legs:
                times[k].append(timed(lambda b: m.predict(b["ids"], seg_ids=seg(b), token_keep=keep), batches, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        print("%-34s %-11s %10s %18s %8s %10s  %s" % ("shape", "schedule", "ms/batch", "spread ms", "ratio", "rows alone", "S_l"))
        for k, keep, _ in legs:
            base = med["pad plain"] if k.startswith("pad") else med["plain"]
            cnt = counts(S, keep or [])
            rows = sum(cnt) / float(L * S) if keep else 1.0
            print("%-34s %-11s %10.3f %8.3f..%-8.3f %8.3f %10.3f  %s" % (name, k, med[k], min(times[k]), max(times[k]), med[k] / base, rows,
                                                                        ",".join(str(x) for x in cnt) if keep else "-"))
        # the three launches of an eliminating layer alone, at the full shape
        k = S // 2
        qkv = (torch.randn(B * S, 3 * H, device="cuda") * 0.5).to(dtype)
        mask = full[0]["ids"].gt(0).to(torch.uint8).contiguous()
        _, lse = hb.attention_fwd(qkv, mask, B, S, heads)
        maskf, score = mask.float(), torch.empty(B, S, device="cuda")
        x = torch.randn(B, S, H, device="cuda").to(dtype)
        idx = hb.token_select(hb.attention_rollout_step(qkv, mask, lse, maskf, 0.0, B, S, heads), mask, k)[0]
        dst = torch.empty(B, k, H, dtype=dtype, device="cuda")
        one = {"score": lambda _: hb.attention_rollout_step(qkv, mask, lse, maskf, 0.0, B, S, heads, out=score),
               "select": lambda _: hb.token_select(score, mask, k), "gather": lambda _: hb.rows_compact(x, idx, out=dst)}
        for kname, fn in one.items():
            ts = [timed(fn, [None], 50) for _ in range(args.rounds)]
            print("%-34s %-11s %10.1f us per launch (%.1f..%.1f; k = %d%s)" % (
                name, kname, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), k,
                "; with the wrapper's four torch.empty calls" if kname == "select" else ""))
        del m, full, short
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
