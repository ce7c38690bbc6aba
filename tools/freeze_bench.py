"""Step time and peak memory of fine-tuning with frozen parameters (requires_grad False), one JSON line per configuration.

    python tools/freeze_bench.py [--steps 20 --warmup 5] [--only NAME ...]

The flagship step of bench.py (synthetic n-best batch, B 256, S 128, n_best 5, bf16, dropout on, forward + losses + backward +
BertAdam through trainer.train_step) with:
  bert-base: nothing frozen | the embeddings | the embeddings + layers 0..5 | the whole encoder (embeddings + 12 layers)
  xlm-roberta-base: nothing frozen | the embeddings
Peak memory is torch.cuda.max_memory_allocated over the timed steps, model and optimizer state included.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("bert", "none", False, 0), ("bert", "emb", True, 0), ("bert", "emb+6", True, 6), ("bert", "encoder", True, 12),
           ("xlm-roberta", "none", False, 0), ("xlm-roberta", "emb", True, 0)]


def run(model_name, emb, layers, B, S, steps, warmup):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.cli import freeze_parameters
    from nbest_amd.model import NBestSTCModel
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import train_step
    dev = torch.device("cuda", 0)
    labels = ncfg.LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
    cfg = ncfg.NAMED[model_name]()
    model = NBestSTCModel(cfg, labels, device=dev, compute_dtype=torch.bfloat16, dropout=0.3, seed=999)
    model.load_reference_state(synth.model_state(cfg, labels, seed=999))
    model.train()
    frozen = freeze_parameters(model, emb, layers)
    b = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=999)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    batch["tok_perm"] = torch.from_numpy(np.argsort(b["ids"].ravel(), kind="stable").astype(np.int32)).to(dev)
    opt = HipBertAdam(model, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=100000)
    for _ in range(warmup):
        train_step(model, opt, batch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    for _ in range(steps):
        out = train_step(model, opt, batch)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / steps
    assert np.isfinite(float(out["loss_parts"].sum().item()))
    n_frozen = sum(s.numel for s in model.arena.slots if s.name in frozen)
    return dict(model=model_name, B=B, S=S, dtype="bf16", frozen_embeddings=emb, frozen_layers=layers, frozen_params=n_frozen,
                ms_per_step=round(1000 * dt, 3), utt_per_s=round(B / dt, 1),
                peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), steps=steps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--only", nargs="*", default=None, help="MODEL:NAME entries of the table, e.g. bert:emb+6")
    a = ap.parse_args()
    for model_name, name, emb, layers in CONFIGS:
        if a.only and "%s:%s" % (model_name, name) not in a.only:
            continue
        res = run(model_name, emb, layers, a.batch, a.seq_len, a.steps, a.warmup)
        res["config"] = name
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
