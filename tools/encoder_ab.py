#!/usr/bin/env python3
"""Bit-level A/B of the encoder entry points between two builds of the library, through the model.

    NBEST_LIB=/path/to/other/libnbest_hip.so python tools/encoder_ab.py dump --out A.npz
    python tools/encoder_ab.py dump --out B.npz
    python tools/encoder_ab.py compare A.npz B.npz

``dump`` runs ``forward_backward`` on seeded models at B 4, S 128 and saves, for every case, the loss parts and the scores in full and two
64-bit digests of the bits of every parameter's gradient (the sum of its 32-bit words, and their sum weighted by position: a hundred-odd
cases of 30 M gradients each do not fit a file).  The grid: 768 / 3072 / 12 heads with L 3 (odd: one layer without a partner) and L 4,
and 256 / 1024 / 4 heads with L 10 (a window cut at the 16-entry table, a flush for want of a free buffer set); every ``wgrad_group``
mode; ``cls_top`` on and off; bf16, fp32 (mode plan only: it has no other) and fp8w (the calibration step and the fp8 step after it;
without ``cls_top``, which it does not run); hidden dropout 0 and 0.1.  On top of the bf16 cases: the backward in
2-layer chunks, two accumulated micro-batches, the transcript pass (``add_l2_loss``), frozen embeddings + layer 0 (``first_trainable``,
``no_input_grad``), single frozen matrices (``wgrad_skip_host``), a trainable head mask (``head_gate_stash``), ``head_gate_grad``
(``no_param_grad`` under gates), FGM (``emb_delta``) and ``attribute`` (interpolated embeddings, ``no_param_grad``).  ``compare`` exits
non-zero unless both files hold the same arrays with the same bytes, and names the first array and index (for the gradients: the case
and the parameter) that differ.  ``dump --only TEXT`` keeps the cases whose tag contains TEXT."""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S = 4, 128
MODES = ("plan", "never", "always", "window")


def dump(out_path, only=""):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, hipabi as hb, synth
    from nbest_amd.model import NBestSTCModel
    labels = ncfg.LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
    modes = dict(plan=hb.WGRAD_GROUP_PLAN, never=hb.WGRAD_GROUP_NEVER, always=hb.WGRAD_GROUP_ALWAYS, window=hb.WGRAD_GROUP_WINDOW)
    out = {}

    states = {}

    def keep(tag, m, res):
        dig = []
        for s in m.arena.slots:                   # the bits of every gradient tensor: sum of the words, sum weighted by position
            w = m.arena.view(m.arena.g, s.name).contiguous().view(torch.int32).flatten().to(torch.int64)
            dig += [w.sum(), (w * (torch.arange(w.numel(), device=w.device) % 65521 + 1)).sum()]
        torch.cuda.synchronize()
        out[tag + "/grad_digest"] = torch.stack(dig).view(-1, 2).cpu().numpy().copy()
        out[tag.split("/")[0] + "/" + tag.split("/")[1] + "/slots"] = np.array([s.name for s in m.arena.slots])
        for k in ("top", "final", "loss_parts"):
            out["%s/%s" % (tag, k)] = res[k].detach().float().cpu().numpy().copy()

    def model(width, L, dtype, mode, cls_top, hdrop):
        H, F, heads = width
        cfg = ncfg.bert_base(num_hidden_layers=L, hidden_size=H, intermediate_size=F, num_attention_heads=heads, vocab_size=2048,
                             hidden_dropout_prob=hdrop, attention_probs_dropout_prob=0.1 if hdrop else 0.0)
        fp8 = dtype == "fp8w"
        m = NBestSTCModel(cfg, labels, device="cuda:0", compute_dtype=torch.bfloat16 if fp8 else dtype, dropout=0.1 if hdrop else 0.0,
                          fp8_forward=fp8, wgrad_group=modes[mode])
        if (width, L) not in states:
            states.clear()
            states[(width, L)] = synth.model_state(cfg, labels, seed=11)
        m.load_reference_state(states[(width, L)])
        m.cls_top = cls_top
        m.train()
        bt = {k: torch.from_numpy(v).cuda() for k, v in synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=3, ragged=True, trans_len=32).items()}
        return m, bt

    def step(m, bt, **kw):
        return m.forward_backward(bt["ids"], bt["labels"], seg_ids=bt["seg"], **kw)

    shapes = [((768, 3072, 12), 3), ((768, 3072, 12), 4), ((256, 1024, 4), 10)]
    for (width, L), mode, cls_top, hdrop in itertools.product(shapes, MODES, (True, False), (0.0, 0.1)):
        base = "H%d/L%d/%s/cls%d/p%g" % (width[0], L, mode, cls_top, hdrop)
        if only not in base:
            continue
        print("encoder_ab dump: %s" % base, flush=True)
        for dtype in (torch.float32, torch.bfloat16, "fp8w"):
            # (fp32 has no grouped or window launches: every mode is "never"; an fp8w model runs no cls_top layer)
            if (dtype == torch.float32 and mode != "plan") or (dtype == "fp8w" and cls_top):
                continue
            m, bt = model(width, L, dtype, mode, cls_top, hdrop)
            tag = "%s/%s" % (base, dtype if dtype == "fp8w" else str(dtype)[6:])
            keep(tag + "/step1", m, step(m, bt))
            if dtype == "fp8w":                   # the step after the calibration step: the fp8 forward and backward
                keep(tag + "/step2", m, step(m, bt))
            if dtype != torch.bfloat16:
                continue
            chunks = [(lo, min(lo + 2, L)) for lo in range(0, L, 2)]
            keep(tag + "/chunks", m, step(m, bt, chunks=chunks))
            keep(tag + "/accumulate", m, step(m, bt, accumulate=True, chunks=chunks))
            keep(tag + "/l2", m, step(m, bt, trans_input_ids=bt["tids"], trans_seg_ids=bt["tseg"], add_l2_loss=True))
            keep(tag + "/adv", m, step(m, bt, adv=dict(epsilon=1.0)))
            if hdrop == 0.0:
                a = m.attribute(bt["ids"][:2], bt["seg"][:2], targets=[(0, 1), (1, 2)], steps=4)
                torch.cuda.synchronize()
                out[tag + "/attribute"] = a["attr"].cpu().numpy().copy()
            g = torch.Generator().manual_seed(5)
            mask = (torch.rand(L, width[2], generator=g) > 0.3).float()
            mask[0, 0] = 0.5
            m.set_head_mask(mask)
            hg = m.head_gate_grad(bt["ids"], bt["labels"], bt["seg"])
            torch.cuda.synchronize()
            out[tag + "/head_gate_grad"] = hg["grad"].cpu().numpy().copy()
            m.set_head_mask(mask, trainable=True)
            keep(tag + "/head_mask_train", m, step(m, bt))
            keep(tag + "/head_mask_train_chunks", m, step(m, bt, chunks=chunks))
            m.set_head_mask(None)
            # single frozen matrices (wgrad_skip_host), then embeddings + layer 0 frozen (first_trainable 1, no_input_grad)
            names = [n for n, _ in m.named_parameters() if n.endswith(".weight") and ".layer." in n and "LayerNorm" not in n]
            for n, p in m.named_parameters():
                p.requires_grad_(n not in names[1::3] and "pooler" not in n)
            keep(tag + "/skip", m, step(m, bt, chunks=chunks))
            for n, p in m.named_parameters():
                p.requires_grad_("pooler" not in n and "embeddings" not in n and ".layer.0." not in n)
            m.zero_grad()
            keep(tag + "/frozen", m, step(m, bt))
            keep(tag + "/frozen_chunks", m, step(m, bt, chunks=chunks))
            del m
    np.savez(out_path, **out)
    print("encoder_ab dump: %d arrays from %s -> %s" % (len(out), hb.LIB_PATH, out_path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print("encoder_ab compare: the files hold different arrays: %s" % sorted(set(a.files) ^ set(b.files))[:5])
        return 1
    nbytes = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            print("encoder_ab compare: %s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            return 1
        if x.tobytes() != y.tobytes():
            xb, yb = (np.ascontiguousarray(v).reshape(-1).view(np.uint32) for v in (x, y))
            i = int(np.flatnonzero(xb != yb)[0])
            if k.endswith("/grad_digest"):
                slots = a["/".join(k.split("/")[:2]) + "/slots"]
                print("encoder_ab compare: %s: the gradient of %s differs" % (k, slots[i // 4]))
                return 1
            print("encoder_ab compare: %s differs first at flat index %d (%s): %r against %r; %d of %d elements differ"
                  % (k, i, np.unravel_index(i, x.shape), x.reshape(-1)[i], y.reshape(-1)[i], int((xb != yb).sum()), xb.size))
            return 1
        nbytes += x.nbytes
    print("encoder_ab compare: %d arrays, %d bytes: every array byte-equal" % (len(a.files), nbytes))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("--out", required=True)
    d.add_argument("--only", default="")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.out, a.only)
        return 0
    return compare(a.a, a.b)


if __name__ == "__main__":
    sys.exit(main())
