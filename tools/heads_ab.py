#!/usr/bin/env python3
"""Bit-level A/B of the heads entry points between two builds of the library.

    NBEST_LIB=/path/to/other/libnbest_hip.so python tools/heads_ab.py dump --out A.npz
    python tools/heads_ab.py dump --out B.npz
    python tools/heads_ab.py compare A.npz B.npz

``dump`` runs stc_heads, stc_heads_kd, stc_heads_kd_t (T = 1 and 2), stc_heads_rdrop, stc_heads_logits and stc_heads_vjp (after a plain
call) on small seeded problems and saves every output (top, bott, final, loss_parts, dcls, dWh, dbh; logits).  The grid: the shipped
label space and the 75-row space whose 70-column head takes the strided nk > 64 path; B in {1, 5}, the last row of B = 5 saturated (two
top logits near +-115: scores exactly 1 and 0, the clamps); H 768 and H 80 (no multiple of 64: the tails of the mask words and of the
64-column tiles); fp32 and bf16 CLS rows; dropout 0 and 0.3; accumulate 0 and 1 on pre-filled dWh / dbh; alpha in {0, 0.3, 1}.  R-Drop
runs on the problem doubled (B2 in {2, 10}), the twins drawn independently.  ``compare`` exits non-zero unless both files hold the same
arrays with the same bytes, and names the first array and index that differ."""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("top", "bott", "final", "loss_parts", "dcls", "dWh", "dbh")
WIDE_SPACE = {0: [0], 1: [1, 2], 2: list(range(3, 73))}


def spaces():
    from nbest_amd.config import LabelSpace
    return {"shipped": LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json")),
            "wide": LabelSpace(WIDE_SPACE, ["s0", "a-x", "a-NONE"] + ["b-%d" % i for i in range(69)] + ["b-NONE"])}


def problem(ls, R, B, H, dtype, seed):
    """CLS rows at row stride 2 H, head matrix, labels with at most one bottom per top, a teacher's probabilities (random sigmoid /
    softmax draws, final = top x bottom) and logits; B > 1: the last row saturated"""
    gen = torch.Generator().manual_seed(seed)
    Wh, bh = torch.randn(R, H, generator=gen) * 0.05, torch.randn(R, generator=gen) * 0.05
    hidden = torch.randn(B, 2, H, generator=gen)
    if B > 1:
        hidden[B - 1, 0] += 60.0 * (768.0 / H) * (Wh[0] - Wh[1])
    y = torch.zeros(B, ls.n_bottom)
    for b in range(B):
        for t in torch.randperm(ls.n_top, generator=gen)[:2].tolist():
            bs = ls.top2bottom[t]
            y[b, bs[int(torch.randint(0, len(bs), (1,), generator=gen))]] = 1
    t_logits = torch.randn(B, R, generator=gen) * 2.0
    t_top = torch.sigmoid(t_logits[:, :ls.n_top])
    t_fin, bott, col = torch.zeros(B, ls.n_bottom), [], ls.n_top
    for t in range(ls.n_top):
        bs = ls.top2bottom[t]
        if len(bs) < 2:
            t_fin[:, bs[0]] = t_top[:, t]
            continue
        s = torch.softmax(t_logits[:, col:col + len(bs)], dim=1)
        bott.append(s)
        t_fin[:, bs] = t_top[:, t:t + 1] * s
        col += len(bs)
    t_bott = torch.cat(bott, dim=1)
    if B > 1:                                   # fractional targets on the two saturated tops: clamped logs carry weight in the soft loss
        t_top[B - 1, 0] = t_top[B - 1, 1] = 0.3
    dev = lambda x: x.cuda().contiguous()
    return dict(hidden=dev(hidden.to(dtype).reshape(B * 2, H)), Wh=dev(Wh), bh=dev(bh), y=dev(y), t_top=dev(t_top), t_bott=dev(t_bott),
                t_fin=dev(t_fin), t_logits=dev(t_logits))


def dump(out_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    out = {}

    def keep(tag, res):
        torch.cuda.synchronize()
        for k, v in zip(KEYS, res):
            if v is not None:
                out["%s/%s" % (tag, k)] = v.detach().cpu().numpy().copy()

    for (sname, ls), B, H, dtype in itertools.product(spaces().items(), (1, 5), (768, 80), (torch.float32, torch.bfloat16)):
        dls = hb.DeviceLabelSpace(ls, "cuda")
        R = dls.n_rows
        p = problem(ls, R, B, H, dtype, seed=1000 * B + H)
        p2 = problem(ls, R, 2 * B, H, dtype, seed=2000 * B + H)           # R-Drop: B2 = 2 B rows
        base = "%s/B%d/H%d/%s" % (sname, B, H, str(dtype)[6:])
        logits = hb.stc_heads_logits(p["hidden"], 2 * H, p["Wh"], p["bh"], dls, B, H)
        torch.cuda.synchronize()
        out[base + "/logits"] = logits.cpu().numpy().copy()
        for drop_p, acc in itertools.product((0.0, 0.3), (0, 1)):
            def kw():                             # fresh pre-filled gradient buffers for every call
                g = torch.Generator().manual_seed(77)
                return dict(need_grad=True, accumulate=bool(acc), drop_p=drop_p, seed=4321, drop_stream=900,
                            dWh=torch.randn(R, H, generator=g).cuda(), dbh=torch.randn(R, generator=g).cuda())
            tag = "%s/p%g/acc%d" % (base, drop_p, acc)
            args = (p["hidden"], 2 * H, p["Wh"], p["bh"], dls, p["y"])
            ws = hb.heads_ws(B, R, H, "cuda")
            k = kw()
            res = hb.stc_heads(*args, B, H, ws=ws, **k)
            keep(tag + "/plain", res)
            g = torch.Generator().manual_seed(5)
            up = [torch.randn(x.shape, generator=g).cuda() for x in res[:3]]
            dcls = hb.stc_heads_vjp(p["Wh"], dls, res[0], res[1], up[0], up[1], up[2], B, H, k["dWh"], k["dbh"], ws, accumulate=bool(acc),
                                    drop_p=drop_p, seed=4321, drop_stream=900)
            keep(tag + "/vjp", (None, None, None, None, dcls, k["dWh"], k["dbh"]))
            keep(tag + "/plain_nograd", hb.stc_heads(*args, B, H, need_grad=False, drop_p=drop_p, seed=4321, drop_stream=900))
            for alpha in (0.0, 0.3, 1.0):
                keep("%s/kd/a%g" % (tag, alpha), hb.stc_heads_kd(*args, p["t_top"], p["t_bott"], p["t_fin"], alpha, B, H, **kw()))
                for T in (1.0, 2.0):
                    keep("%s/kd_t%g/a%g" % (tag, T, alpha), hb.stc_heads_kd_t(*args, p["t_logits"], alpha, T, B, H, **kw()))
                keep("%s/rdrop/a%g" % (tag, alpha),
                     hb.stc_heads_rdrop(p2["hidden"], 2 * H, p2["Wh"], p2["bh"], dls, p2["y"], alpha, 2 * B, H, **kw()))
            keep(tag + "/kd/a0_no_teacher", hb.stc_heads_kd(*args, None, None, None, 0.0, B, H, **kw()))
    np.savez(out_path, **out)
    print("heads_ab dump: %d arrays from %s -> %s" % (len(out), hb.LIB_PATH, out_path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print("heads_ab compare: the files hold different arrays: %s" % sorted(set(a.files) ^ set(b.files))[:5])
        return 1
    nbytes = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            print("heads_ab compare: %s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            return 1
        if x.tobytes() != y.tobytes():
            xb, yb = (np.ascontiguousarray(v).reshape(-1).view(np.uint32) for v in (x, y))
            i = int(np.flatnonzero(xb != yb)[0])
            print("heads_ab compare: %s differs first at flat index %d (%s): %r against %r; %d of %d elements differ"
                  % (k, i, np.unravel_index(i, x.shape), x.reshape(-1)[i], y.reshape(-1)[i], int((xb != yb).sum()), xb.size))
            return 1
        nbytes += x.nbytes
    print("heads_ab compare: %d arrays, %d bytes: every array byte-equal" % (len(a.files), nbytes))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.out)
        return 0
    return compare(a.a, a.b)


if __name__ == "__main__":
    sys.exit(main())
