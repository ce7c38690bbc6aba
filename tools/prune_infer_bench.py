#!/usr/bin/env python3
"""predict without a mask, under a head mask (gated: full-width layers, the pruned heads' context multiplied by 0) and under the same
mask compacted (set_head_mask(mask, compact=True): only the kept heads run), alternately in one process on the same seeded batches,
timed with device events.  Also the pack step of the compact leg alone (the gather nbest_head_prune_pack plus, bf16, the pack of the
images), as a time and as a share of the compact call.

Masks: deterministic - head h of layer l is pruned when (7 h + 3 l) % heads < round(frac * heads), for frac = 25 %, 50 % and 75 %
(the same number of heads in every layer, at positions that move with the layer).

Per shape and mask: ms per batch of each leg (median over rounds, min..max as the spread), compact / gated, and max |d| of the final
scores between the gated and the compact leg.

    python tools/prune_infer_bench.py [--rounds 9] [--iters 10] [--only NAME]"""
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
FRACS = (0.25, 0.50, 0.75)


def prune_mask(L, heads, frac):
    n = int(round(frac * heads))
    return torch.tensor([[0.0 if (7 * h + 3 * l) % heads < n else 1.0 for h in range(heads)] for l in range(L)])


def timed(fn, batches, rounds, iters):
    out = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(batches[0])
        t0.record()
        for i in range(iters):
            fn(batches[i % 2])
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / iters)
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
    print("%-34s %-6s %-8s %10s %18s" % ("shape", "pruned", "leg", "ms/batch", "spread ms"))
    for name, mk, dtype, B, S in SHAPES:
        if args.only and args.only not in name:
            continue
        cfg = mk(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=0.0, seed=1)
        m.load_reference_state(synth.model_state(cfg, labels, seed=1))
        m.eval()
        batches = []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
        seg = lambda b: b["seg"] if cfg.family == "bert" else None
        predict = lambda b: m.predict(b["ids"], seg_ids=seg(b))
        for frac in FRACS:
            mask = prune_mask(L, heads, frac)
            kept = int(mask.sum().item())

            def leg(kind):
                def run(b):
                    if kind == "plain":
                        m.set_head_mask(None)
                    elif kind == "gated":
                        m._head_mask, m._head_mask_compact = gated_state
                    else:
                        m._head_mask, m._head_mask_compact, m._prune = compact_state
                    return predict(b)
                return run
            # (the mask is installed once per kind - set_head_mask copies the mask off the device - and swapped in per call)
            m.set_head_mask(mask)
            gated_state = (m._head_mask, False)
            m.set_head_mask(mask, compact=True)
            compact_state = (m._head_mask, True, m._prune)
            packed = m._packed_bf16_ok()
            legs = {k: leg(k) for k in ("plain", "gated", "compact")}
            legs["pack"] = lambda b: compact_state[2].build(m, packed)
            dmax = max((legs["gated"](b)["final"] - legs["compact"](b)["final"]).abs().max().item() for b in batches)
            times = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    if k == "pack":
                        m._head_mask, m._head_mask_compact, m._prune = compact_state
                    times[k] += timed(fn, batches, 1, args.iters)
            med = {k: statistics.median(v) for k, v in times.items()}
            tag = "%2.0f %%" % (100 * frac)
            for k in legs:
                print("%-34s %-6s %-8s %10.3f %8.3f..%-8.3f" % (name, tag, k, med[k], min(times[k]), max(times[k])))
            print("%-34s %-6s %d of %d heads kept (per layer %s): compact / gated = %.3f (%.1f %% faster), compact / plain = %.3f, pack = %.1f %% of "
                  "the compact call, max |d final| gated vs compact = %.3e" % (
                      name, tag, kept, L * heads, sorted(set(len(ix) for ix in compact_state[2].kept)), med["compact"] / med["gated"],
                      100 * (1 - med["compact"] / med["gated"]), med["compact"] / med["plain"], 100 * med["pack"] / med["compact"], dmax))
            m.set_head_mask(None)
        del m, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
