#!/usr/bin/env python3
"""Held-out F1 of predict under token elimination, on the shipped text: the split and set-up of tools/head_prune_trajectory.py
(fixed batch order, 8 initialisation seeds, valid[:384] for training, valid[384:512] held out and never trained on; shapes, seeds
and learning rates from tests/golden/case_traj.npz's meta; dropout on: heads 0.3, encoder 0.1), with --layers 4 so that three layers
can eliminate.

Per seed: one randomly initialised bert is trained 6 epochs (144 BertAdam steps) WITHOUT pruning; the held-out part is then labelled
by trainer.predict_split without and with --token_keep S:S/2, S:S/4, S:S/8 (S = the longest encoded utterance of the split; a batch
shorter than a count drops nothing there) and with a constant count, the median utterance length.  Reported per schedule: held-out F1, its paired
difference to the unpruned predict, and the share of utterances whose label set is the unpruned one.  The split is small and the model
starts from random weights (its attention is close to uniform): this records a trajectory, it does not establish what a pretrained
encoder loses.

    python tools/token_prune_trajectory.py [--layers 4] [--dtype bf16] [--out profiles/token_prune_trajectory.txt]"""
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
from nbest_amd import config as ncfg, fscore, inputs, synth, trainer
from nbest_amd.model import NBestSTCModel
from nbest_amd.optim import HipBertAdam

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--dropout", type=float, default=0.3)
    ap.add_argument("--bert_dropout", type=float, default=0.1)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--seeds", type=int, default=None, help="use only the first N seeds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    meta = json.loads(str(np.load(os.path.join(GOLDEN, "case_traj.npz"))["meta"]))
    seeds = meta["seeds"][:args.seeds] if args.seeds else meta["seeds"]
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
    opt = types.SimpleNamespace(batchSize=meta["batch"], tokenizer=inputs.WordPieceTokenizer(vocab), pre_trained_model="bert",
                                tod_pre_trained_model=None, without_system_act=False, add_l2_loss=False, add_segment_ids=True)
    split_tr, split_he = trainer.EncodedSplit(tr, opt, memory), trainer.EncodedSplit(he, opt, memory)
    lens = [len(r[0]) for r in split_he.rows]
    S = max(lens)
    L = args.layers
    sched = [("unpruned", None)] + [("S:S/%d" % q, trainer.token_keep_schedule(L, S, max(1, S // q))) for q in (2, 4, 8)]
    med = int(np.median(lens))
    sched.append(("median length", [med] * (L - 1)))
    gold = [split_he.labels[j] for j in range(len(split_he))]

    def f1_of(cases):
        TP = FP = FN = 0
        for (_, pc), g in zip(cases, gold):
            TP, FP, FN = fscore.update_f1(pc, g, TP, FP, FN)
        return fscore.compute_f1(TP, FP, FN)[2]

    lines = ["%d seeds, %d epochs over valid[:%d] without pruning, held-out valid[%d:%d] (%d utterances, %d..%d tokens, median %d), %d-layer bert "
             "from random weights, %s, dropout %g (heads) / %g (encoder), batch %d, BertAdam lr %g / %g"
             % (len(seeds), meta["epochs"], nt, nt, nt + nh, len(gold), min(lens), S, med, L, args.dtype, args.dropout, args.bert_dropout,
                meta["batch"], meta["lr"], meta["bert_lr"])]
    for name, keep in sched[1:]:
        lines.append("schedule %-14s keep = %s" % (name, keep))
    f1 = {n: [] for n, _ in sched}
    agree = {n: [] for n, _ in sched}
    for seed in seeds:
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=cd, dropout=args.dropout, seed=seed)
        m.load_reference_state(synth.model_state(cfg, labels, seed=seed))
        opt.optimizer = HipBertAdam(m, lr=meta["lr"], bert_lr=meta["bert_lr"], warmup=0.1, t_total=meta["t_total"])
        for _ in range(meta["epochs"]):
            trainer.train_epoch(m, split_tr, opt, memory, shuffle=False)
        m.eval()
        base = None
        for name, keep in sched:
            cases = trainer.predict_split(m, split_he, opt, memory, **({} if keep is None else dict(token_keep=keep)))
            base = cases if base is None else base
            f1[name].append(f1_of(cases))
            agree[name].append(100.0 * sum(set(a[1]) == set(b[1]) for a, b in zip(cases, base)) / len(cases))
        lines.append("seed %d  held-out F1 (same labels as unpruned, %%): %s"
                     % (seed, "  ".join("%s %.1f (%.0f)" % (n, f1[n][-1], agree[n][-1]) for n, _ in sched)))
        print(lines[-1], flush=True)
        del m
    for n, _ in sched:
        a, g = np.asarray(f1[n]), np.asarray(agree[n])
        d = a - np.asarray(f1["unpruned"])
        se = lambda x: x.std(ddof=1) / np.sqrt(len(x)) if len(x) > 1 else float("nan")
        lines.append("%-14s MEAN over %d seeds: held-out F1 %.2f (seed std %.2f); - unpruned, paired per seed: %+.2f pt, standard error %.2f; "
                     "same label set as unpruned: %.1f %% of utterances, standard error %.1f"
                     % (n, len(a), a.mean(), a.std(ddof=1) if len(a) > 1 else float("nan"), d.mean(), se(d), g.mean(), se(g)))
    lines.append("A small model from random weights on 384 utterances: its attention is near uniform, so which tokens go is close to arbitrary. "
                 "This does not establish what a pretrained encoder loses.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
