#!/usr/bin/env python3
"""Attention rollout: what a nbest_attention_rollout_step launch costs, what model.attention_rollout adds to the eval forward it
runs, and what the same [L, B, S] result costs through the attention maps (forward(return_attns=True) + trainer.rollout_reference
on the device).  The legs alternate inside a round in one process on the same seeded batches, timed with device events.

Per shape: ms per call of each leg (median over rounds, min..max as the spread), ms per rollout_step launch, and the largest
|attention_rollout - maps route| of the final row.

    python tools/rollout_bench.py [--rounds 7] [--iters 5] [--only NAME] [--residual 0.5]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb, synth, trainer
from nbest_amd.model import NBestSTCModel

SHAPES = [("bert-base bf16 B256 S128", ncfg.bert_base, 256, 128),
          ("xlm-roberta-large bf16 B64 S256", ncfg.xlmr_large, 64, 256)]
STEP_LAUNCHES = 48          # rollout_step launches per timed "step" call (one launch is a few tens of microseconds)


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default=None, help="run the shapes whose name contains this string")
    ap.add_argument("--residual", type=float, default=0.5)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    rho = args.residual
    print("%d rounds x %d calls per leg, the legs alternating inside a round; residual %g" % (args.rounds, args.iters, rho))
    print("%-34s %-26s %10s %18s" % ("shape", "leg", "ms/call", "spread ms"))
    for name, mk, B, S in SHAPES:
        if args.only and args.only not in name:
            continue
        cfg = mk(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, seed=1)
        m.load_reference_state(synth.model_state(cfg, labels, seed=1))
        m.eval()
        L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
        batches = []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
        seg = lambda b: b["seg"] if cfg.family == "bert" else None
        opt = type("O", (), {})()

        def maps_route(b):
            attns = m(opt, b["ids"], seg_ids=seg(b), return_attns=True)[3]
            return trainer.rollout_reference(attns, rho)

        # the kernel alone: one eval forward leaves the stash, then STEP_LAUNCHES launches ping-pong over layer views of it
        rec = []
        m._passes_and_heads(batches[0]["ids"], seg(batches[0]), None, None, False, after_asr=rec.append, full_top=True)
        m._end_of_step(False, advance=False)
        views = list(m._stash_attention_views(rec[0]))
        rows = torch.zeros(2, B, S, device="cuda")
        rows[0, :, 0] = 1.0

        def steps(_):
            for i in range(STEP_LAUNCHES):
                q, l = views[L - 1 - i % L]
                hb.attention_rollout_step(q, rec[0].inputs[3], l, rows[i % 2], rho, B, S, heads, out=rows[1 - i % 2])

        # "step" runs first in every round: the other legs overwrite the stash (same shape, so the views stay valid memory)
        legs = {"rollout_step x %d" % STEP_LAUNCHES: steps,
                "eval forward": lambda b: m(opt, b["ids"], seg_ids=seg(b)),
                "attention_rollout": lambda b: m.attention_rollout(b["ids"], seg_ids=seg(b), residual=rho),
                "return_attns + reference": maps_route}
        dmax = max((m.attention_rollout(b["ids"], seg_ids=seg(b), residual=rho)["layers"].double() - maps_route(b)).abs().max().item()
                   for b in batches)
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, batches, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in legs:
            print("%-34s %-26s %10.3f %8.3f..%-8.3f" % (name, k, med[k], min(times[k]), max(times[k])))
        k0 = "rollout_step x %d" % STEP_LAUNCHES
        esz = 2
        mb = (B * S * 2 * cfg.hidden_size * esz + B * heads * S * 4 + 2 * B * S * 4 + B * S) / 1e6
        print("%-34s one rollout_step launch = %.4f ms (%.1f MB of Q, K, lse, mask and vectors: %.0f GB/s); attention_rollout - eval forward "
              "= %.3f ms for %d launches; the maps route / attention_rollout = %.2f; max |layers - maps route| = %.3e"
              % (name, med[k0] / STEP_LAUNCHES, mb, mb / 1e3 / (med[k0] / STEP_LAUNCHES / 1e3), med["attention_rollout"] - med["eval forward"], L,
                 med["return_attns + reference"] / med["attention_rollout"], dmax))
        del m, batches, views, rec
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
