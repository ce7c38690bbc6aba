#!/usr/bin/env python3
"""Held-out F1 with and without SAM / ASAM on the shipped text: the set-up of tools/rdrop_trajectory.py (fixed batch order, 8
initialisation seeds x 6 epochs = 144 BertAdam steps over valid[:384], evaluated after every epoch on valid[384:512], which is never
trained on; shapes, seeds and learning rates from tests/golden/case_traj.npz's meta; the shipped script's dropout on: heads 0.3,
encoder 0.1).

Per seed: one randomly initialised bert of --layers layers, trained without the flag ("off"), with --sam_rho at every value of
--rhos and with --sam_rho --sam_adaptive at every value of --asam_rhos (eta 0.01).  The runs of a seed share the initial weights, the
batch order and the dropout seed, so the differences are paired per seed.  Next to the F1 the mean sharpness per utterance of the
last epoch (hard loss at w + e minus at w) is printed.  The split is small and the model starts from random weights: this records a
trajectory, it does not establish an effect on F1.

    python tools/sam_trajectory.py [--rhos 0.02,0.05,0.1] [--asam_rhos 0.5,1] [--layers 2] [--dtype bf16] [--out profiles/sam_trajectory.txt]"""
import argparse
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
    ap.add_argument("--rhos", default="0.02,0.05,0.1")
    ap.add_argument("--asam_rhos", default="0.5,1")
    ap.add_argument("--eta", type=float, default=0.01)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.3)
    ap.add_argument("--bert_dropout", type=float, default=0.1)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    meta = json.loads(str(np.load(os.path.join(GOLDEN, "case_traj.npz"))["meta"]))
    labels = ncfg.LabelSpace.from_json(os.path.join(GOLDEN, "label_space.json"))
    vocab = json.load(open(os.path.join(GOLDEN, "text_vocab.json")))
    data = trainer.read_wcn_data(os.path.join(GOLDEN, "valid_512.txt"))
    nt, nh = meta["n_train"], meta["n_held"]
    tr = tuple(list(x[:nt]) for x in data)
    he = tuple(list(x[nt:nt + nh]) for x in data)
    label2idx = json.loads(str(np.load(os.path.join(GOLDEN, "case_text.npz"))["label2idx"]))
    memory = dict(label2idx=label2idx, idx2label=labels.idx2label)
    cd = torch.float32 if args.dtype == "f32" else torch.bfloat16
    cfg = ncfg.bert_base(num_hidden_layers=args.layers, vocab_size=len(vocab), hidden_dropout_prob=args.bert_dropout,
                         attention_probs_dropout_prob=args.bert_dropout)

    def run(model, rho, adaptive):
        """6 epochs of train_epoch; the held-out F1 after every epoch and the last epoch's mean sharpness per utterance"""
        opt = types.SimpleNamespace(batchSize=meta["batch"], tokenizer=inputs.WordPieceTokenizer(vocab), pre_trained_model="bert",
                                    tod_pre_trained_model=None, without_system_act=False, add_l2_loss=False, add_segment_ids=True,
                                    sam_rho=rho, sam_adaptive=adaptive, sam_eta=args.eta)
        opt.optimizer = HipBertAdam(model, lr=meta["lr"], bert_lr=meta["bert_lr"], warmup=0.1, t_total=meta["t_total"])
        split_tr, split_he = trainer.EncodedSplit(tr, opt, memory), trainer.EncodedSplit(he, opt, memory)
        hist, sharp = [], float("nan")
        for _ in range(meta["epochs"]):
            trainer.train_epoch(model, split_tr, opt, memory, shuffle=False)
            _, (_, _, f), _, _ = trainer.eval_epoch(model, split_he, opt, memory)
            hist.append(f)
            if rho is not None:
                sharp = opt.sam_epoch[0] / max(opt.sam_epoch[2], 1.0)
        return hist, sharp

    legs = [("off", None, False)] + [("sam %g" % float(x), float(x), False) for x in args.rhos.split(",") if x] \
        + [("asam %g" % float(x), float(x), True) for x in args.asam_rhos.split(",") if x]
    lines = ["%d seeds x %d epochs over valid[:%d], held-out valid[%d:%d], %d-layer bert from random weights, %s, dropout %g (heads) / %g "
             "(encoder), batch %d, BertAdam lr %g / %g, %d steps; asam eta %g"
             % (len(meta["seeds"]), meta["epochs"], nt, nt, nt + nh, args.layers, args.dtype, args.dropout, args.bert_dropout, meta["batch"],
                meta["lr"], meta["bert_lr"], meta["epochs"] * (nt // meta["batch"]), args.eta)]
    hists, sharps = {tag: [] for tag, _, _ in legs}, {tag: [] for tag, _, _ in legs}
    for seed in meta["seeds"]:
        sd = synth.model_state(cfg, labels, seed=seed)
        for tag, rho, adaptive in legs:
            model = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=cd, dropout=args.dropout, seed=seed)
            model.load_reference_state(sd)
            h, s = run(model, rho, adaptive)
            hists[tag].append(h)
            sharps[tag].append(s)
        for tag in hists:
            lines.append("%-9s seed %d  held-out F1 by epoch: %s%s" % (tag, seed, " ".join("%5.1f" % x for x in hists[tag][-1]),
                                                                     "" if tag == "off" else "   sharpness (last epoch) %.4f" % sharps[tag][-1]))
        print("\n".join(lines[-len(hists):]), flush=True)
    final = {}
    for tag, h in hists.items():
        h = np.asarray(h)
        final[tag] = h[:, -1]
        lines.append("%-9s MEAN over %d seeds by epoch: %s | final held-out F1 %.2f, seed std %.2f" % (
            tag, len(h), " ".join("%5.1f" % x for x in h.mean(0)), h[:, -1].mean(), h[:, -1].std(ddof=1)))
    for tag, f in final.items():
        if tag != "off":
            d = f - final["off"]
            lines.append("%-9s - off, paired per seed: mean %+.2f pt, standard error %.2f" % (tag, d.mean(), d.std(ddof=1) / np.sqrt(len(d))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
