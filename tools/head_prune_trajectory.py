#!/usr/bin/env python3
"""Held-out F1 of pruned models with and without a fine-tune under the mask, on the shipped text: the split and set-up of
tools/rdrop_trajectory.py (fixed batch order, 8 initialisation seeds, valid[:384] for training, valid[384:512] held out and never
trained on; shapes, seeds and learning rates from tests/golden/case_traj.npz's meta; dropout on: heads 0.3, encoder 0.1).

Per seed: one randomly initialised bert of --layers layers is trained 6 epochs (144 BertAdam steps), its heads are scored on the
TRAINING split (trainer.head_importance) and trainer.prune_lowest prunes 25 / 50 / 75 % of them.  Reported, on the held-out split:
  unpruned            the trained model
  pruned              the same weights under the pruned mask (--testing --head_mask)
  pruned + fine-tune  2 more epochs (48 steps, a fresh BertAdam) under the mask (--train_head_mask), evaluated under it
  unpruned + 2 epochs the same 2 epochs without a mask: what the extra steps alone are worth
All legs of a seed start from the same trained weights, so the differences are paired per seed.  The split is small and the model
starts from random weights: this records a trajectory, it does not establish what pruning costs a pretrained model.

    python tools/head_prune_trajectory.py [--fractions 25,50,75] [--layers 2] [--dtype bf16] [--out profiles/head_prune_trajectory.txt]"""
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
    ap.add_argument("--fractions", default="25,50,75")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--finetune_epochs", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.3)
    ap.add_argument("--bert_dropout", type=float, default=0.1)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fractions = [int(t) for t in args.fractions.split(",")]
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
    n_heads = cfg.num_hidden_layers * cfg.num_attention_heads
    steps_per_epoch = nt // meta["batch"]
    opt = types.SimpleNamespace(batchSize=meta["batch"], tokenizer=inputs.WordPieceTokenizer(vocab), pre_trained_model="bert",
                                tod_pre_trained_model=None, without_system_act=False, add_l2_loss=False, add_segment_ids=True)
    split_tr, split_he = trainer.EncodedSplit(tr, opt, memory), trainer.EncodedSplit(he, opt, memory)

    def held_out(model):
        return trainer.eval_epoch(model, split_he, opt, memory)[1][2]

    def train(model, epochs, t_total):
        opt.optimizer = HipBertAdam(model, lr=meta["lr"], bert_lr=meta["bert_lr"], warmup=0.1, t_total=t_total)
        for _ in range(epochs):
            trainer.train_epoch(model, split_tr, opt, memory, shuffle=False)

    def clone(model, seed):
        """a model with the weights and the dropout position of ``model``, no mask, no optimizer state"""
        m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=cd, dropout=args.dropout, seed=seed)
        m.load_reference_state({k: v.detach().cpu() for k, v in model.state_dict().items()})
        m.step_counter = model.step_counter
        return m

    legs = ["unpruned", "unpruned + %d epochs" % args.finetune_epochs]
    for f in fractions:
        legs += ["pruned %d %%" % f, "pruned %d %% + fine-tune" % f]
    lines = ["%d seeds, %d epochs over valid[:%d] then %d epochs of fine-tuning, held-out valid[%d:%d], %d-layer bert (%d heads) from random "
             "weights, %s, dropout %g (heads) / %g (encoder), batch %d, BertAdam lr %g / %g; heads scored on the training split"
             % (len(meta["seeds"]), meta["epochs"], nt, args.finetune_epochs, nt, nt + nh, args.layers, n_heads, args.dtype, args.dropout,
                args.bert_dropout, meta["batch"], meta["lr"], meta["bert_lr"])]
    res = {leg: [] for leg in legs}
    for seed in meta["seeds"]:
        base = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=cd, dropout=args.dropout, seed=seed)
        base.load_reference_state(synth.model_state(cfg, labels, seed=seed))
        train(base, meta["epochs"], meta["t_total"])
        res["unpruned"].append(held_out(base))
        base.eval()
        imp = trainer.head_importance(base, split_tr, opt, memory)["importance"]
        more = clone(base, seed)
        train(more, args.finetune_epochs, args.finetune_epochs * steps_per_epoch)
        res[legs[1]].append(held_out(more))
        for f in fractions:
            mask = trainer.prune_lowest(imp, None, n_heads * f // 100)
            base.set_head_mask(mask)
            res["pruned %d %%" % f].append(held_out(base))
            base.set_head_mask(None)
            fine = clone(base, seed)
            fine.set_head_mask(mask, trainable=True)
            train(fine, args.finetune_epochs, args.finetune_epochs * steps_per_epoch)
            res["pruned %d %% + fine-tune" % f].append(held_out(fine))
        lines.append("seed %d  held-out F1: %s" % (seed, "  ".join("%s %.1f" % (leg, res[leg][-1]) for leg in legs)))
        print(lines[-1], flush=True)
    r = {leg: np.asarray(v) for leg, v in res.items()}
    for leg in legs:
        lines.append("%-28s MEAN over %d seeds: held-out F1 %.2f, seed std %.2f" % (leg, len(r[leg]), r[leg].mean(), r[leg].std(ddof=1)))

    def paired(a, b):
        d = r[a] - r[b]
        lines.append("%-28s - %-20s paired per seed: mean %+.2f pt, standard error %.2f" % (a, b, d.mean(), d.std(ddof=1) / np.sqrt(len(d))))
    paired(legs[1], "unpruned")
    for f in fractions:
        paired("pruned %d %%" % f, "unpruned")
        paired("pruned %d %% + fine-tune" % f, "pruned %d %%" % f)
        paired("pruned %d %% + fine-tune" % f, "unpruned")
        paired("pruned %d %% + fine-tune" % f, legs[1])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
