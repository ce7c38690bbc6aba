#!/usr/bin/env python3
"""F1 trajectories with and without --ema_decay on the shipped text: the set-up of
tests/test_text_pipeline.py::test_f1_trajectory_tracks_reference_loop (2-layer bert, dropout 0, fixed batch order, 8 initialisation
seeds x 6 epochs = 144 BertAdam steps over valid[:384], evaluated after every epoch on valid[384:512], which is never trained on;
shapes, seeds and learning rates from tests/golden/case_traj.npz's meta), HIP path only.

For every decay: the held-out F1 after every epoch, evaluated on the averaged weights (``optimizer.ema_weights()``), and the mean
and seed standard deviation (ddof 1) of the final one; "off" evaluates the raw weights, as the trainer does without the flag.
Training is the same bits with and without the average, so the runs are paired per seed.

    python tools/ema_trajectory.py [--decays off,0.99] [--dtype bf16] [--out profiles/ema_trajectory.txt]"""
import argparse
import contextlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, inputs, synth, trainer
from nbest_amd.model import NBestSTCModel
from nbest_amd.optim import HipBertAdam

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decays", default="off,0.99")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    decays = [None if d == "off" else float(d) for d in args.decays.split(",")]
    meta = json.loads(str(np.load(os.path.join(GOLDEN, "case_traj.npz"))["meta"]))
    labels = ncfg.LabelSpace.from_json(os.path.join(GOLDEN, "label_space.json"))
    vocab = json.load(open(os.path.join(GOLDEN, "text_vocab.json")))
    data = trainer.read_wcn_data(os.path.join(GOLDEN, "valid_512.txt"))
    nt, nh = meta["n_train"], meta["n_held"]
    tr = tuple(list(x[:nt]) for x in data)
    he = tuple(list(x[nt:nt + nh]) for x in data)
    cfg = ncfg.bert_base(num_hidden_layers=meta["L"], vocab_size=len(vocab), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    label2idx = json.loads(str(np.load(os.path.join(GOLDEN, "case_text.npz"))["label2idx"]))
    memory = dict(label2idx=label2idx, idx2label=labels.idx2label)
    cd = torch.float32 if args.dtype == "f32" else torch.bfloat16
    lines = ["%d seeds x %d epochs over valid[:%d], held-out valid[%d:%d], %d-layer bert, %s, batch %d, BertAdam lr %g / %g, %d steps" % (
        len(meta["seeds"]), meta["epochs"], nt, nt, nt + nh, meta["L"], args.dtype, meta["batch"], meta["lr"], meta["bert_lr"],
        meta["epochs"] * (nt // meta["batch"]))]
    final = {}
    for decay in decays:
        tag = "off" if decay is None else "%g" % decay
        hists = []
        for seed in meta["seeds"]:
            m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=cd, dropout=0.0)
            m.load_reference_state(synth.model_state(cfg, labels, seed=seed))
            opt = types.SimpleNamespace(batchSize=meta["batch"], tokenizer=inputs.WordPieceTokenizer(vocab), pre_trained_model="bert",
                                        tod_pre_trained_model=None, without_system_act=False, add_l2_loss=False, add_segment_ids=True)
            opt.optimizer = HipBertAdam(m, lr=meta["lr"], bert_lr=meta["bert_lr"], warmup=0.1, t_total=meta["t_total"], ema_decay=decay)
            split_tr, split_he = trainer.EncodedSplit(tr, opt, memory), trainer.EncodedSplit(he, opt, memory)
            hist = []
            for _ in range(meta["epochs"]):
                trainer.train_epoch(m, split_tr, opt, memory, shuffle=False)
                with (opt.optimizer.ema_weights() if decay is not None else contextlib.nullcontext()):
                    _, (_, _, f), _, _ = trainer.eval_epoch(m, split_he, opt, memory)
                hist.append(f)
            hists.append(hist)
            lines.append("ema %-5s seed %d  held-out F1 by epoch: %s" % (tag, seed, " ".join("%5.1f" % x for x in hist)))
        h = np.asarray(hists)
        final[tag] = h[:, -1]
        lines.append("ema %-5s MEAN over %d seeds by epoch: %s | final held-out F1 %.2f, seed std %.2f" % (
            tag, len(h), " ".join("%5.1f" % x for x in h.mean(0)), h[:, -1].mean(), h[:, -1].std(ddof=1)))
    if "off" in final:
        for tag, f in final.items():
            if tag != "off":
                d = f - final["off"]
                lines.append("ema %-5s - off, paired per seed: mean %+.2f pt, standard error %.2f" % (tag, d.mean(), d.std(ddof=1) / np.sqrt(len(d))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
