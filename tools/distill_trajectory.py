#!/usr/bin/env python3
"""Held-out F1 of a distilled student with and without a temperature, on the shipped text: the set-up of tools/ema_trajectory.py
(dropout 0, fixed batch order, 8 initialisation seeds x 6 epochs = 144 BertAdam steps over valid[:384], evaluated after every
epoch on valid[384:512], which is never trained on; shapes, seeds and learning rates from tests/golden/case_traj.npz's meta).

Per seed: a 2-layer teacher trained on the split, then 1-layer students started from its layer 1 (student_state_from_teacher)
and trained on the same split - without a teacher ("hard"), on its probabilities ("none": --distill_from without
--distill_temperature) and on its logits at every temperature of --temperatures.  The runs of a seed share the teacher and the
student's initial weights, so the differences are paired per seed.  The split is small and the teacher is trained from random
weights on the very text the student sees: this records a trajectory, it does not establish an effect on F1.

    python tools/distill_trajectory.py [--temperatures 1,2,4] [--alpha 0.5] [--dtype bf16] [--out profiles/distill_trajectory.txt]"""
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
    ap.add_argument("--temperatures", default="1,2,4")
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    temps = [float(t) for t in args.temperatures.split(",")]
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

    def cfg_of(layers):
        return ncfg.bert_base(num_hidden_layers=layers, vocab_size=len(vocab), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)

    def run(model, teacher=None, temperature=None):
        """6 epochs of train_epoch; the held-out F1 after every epoch"""
        opt = types.SimpleNamespace(batchSize=meta["batch"], tokenizer=inputs.WordPieceTokenizer(vocab), pre_trained_model="bert",
                                    tod_pre_trained_model=None, without_system_act=False, add_l2_loss=False, add_segment_ids=True,
                                    teacher=teacher, distill_alpha=args.alpha, distill_temperature=temperature)
        opt.optimizer = HipBertAdam(model, lr=meta["lr"], bert_lr=meta["bert_lr"], warmup=0.1, t_total=meta["t_total"])
        split_tr, split_he = trainer.EncodedSplit(tr, opt, memory), trainer.EncodedSplit(he, opt, memory)
        hist = []
        for _ in range(meta["epochs"]):
            trainer.train_epoch(model, split_tr, opt, memory, shuffle=False)
            _, (_, _, f), _, _ = trainer.eval_epoch(model, split_he, opt, memory)
            hist.append(f)
        return hist

    legs = [("hard", False, None), ("none", True, None)] + [("T %g" % t, True, t) for t in temps]
    lines = ["%d seeds x %d epochs over valid[:%d], held-out valid[%d:%d], 2-layer bert teacher, 1-layer student from its layer 1, %s, "
             "batch %d, BertAdam lr %g / %g, %d steps, alpha %g" % (len(meta["seeds"]), meta["epochs"], nt, nt, nt + nh, args.dtype,
                                                                     meta["batch"], meta["lr"], meta["bert_lr"],
                                                                     meta["epochs"] * (nt // meta["batch"]), args.alpha)]
    hists = {tag: [] for tag in ["teacher"] + [l[0] for l in legs]}
    for seed in meta["seeds"]:
        teacher = NBestSTCModel(cfg_of(2), labels, device="cuda", compute_dtype=cd, dropout=0.0)
        teacher.load_reference_state(synth.model_state(cfg_of(2), labels, seed=seed))
        hists["teacher"].append(run(teacher))
        tsd = {k: v.detach().cpu() for k, v in teacher.state_dict().items()}
        teacher.eval()
        for tag, with_teacher, temperature in legs:
            student = NBestSTCModel(cfg_of(1), labels, device="cuda", compute_dtype=cd, dropout=0.0)
            student.load_reference_state(trainer.student_state_from_teacher(tsd, [1]))
            hists[tag].append(run(student, teacher if with_teacher else None, temperature))
        for tag in hists:
            lines.append("%-8s seed %d  held-out F1 by epoch: %s" % (tag, seed, " ".join("%5.1f" % x for x in hists[tag][-1])))
        print("\n".join(lines[-len(hists):]), flush=True)
    final = {}
    for tag, h in hists.items():
        h = np.asarray(h)
        final[tag] = h[:, -1]
        lines.append("%-8s MEAN over %d seeds by epoch: %s | final held-out F1 %.2f, seed std %.2f" % (
            tag, len(h), " ".join("%5.1f" % x for x in h.mean(0)), h[:, -1].mean(), h[:, -1].std(ddof=1)))
    for tag, f in final.items():
        if tag not in ("teacher", "none"):
            d = f - final["none"]
            lines.append("%-8s - none, paired per seed: mean %+.2f pt, standard error %.2f" % (tag, d.mean(), d.std(ddof=1) / np.sqrt(len(d))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
