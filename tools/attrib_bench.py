"""Integrated-gradients attribution (NBestSTCModel.attribute): pairs per second at bert-base bf16 (S = 128, m = 32) and xlm-roberta-large bf16
(S = 256, m = 32), and the no_param_grad backward against the full backward on the same stash and shape.

    python tools/attrib_bench.py                  # timings (HIP events), one MI355X
    python tools/attrib_bench.py --trace_only     # one attribute() call per shape, for a rocprofv3 --kernel-trace run of its own

The kernel times of nbest_embed_ln_fwd_interp / nbest_embed_attrib come from the kernel trace (tools/rocpd_stats.py); their bytes are
computed here from the shapes and printed next to the timings."""
import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(name, L, S, labels):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = {"bert-base": ncfg.bert_base, "xlm-roberta-large": ncfg.xlmr_large}[name](num_hidden_layers=L)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16)
    m.load_reference_state(synth.model_state(cfg, labels, seed=3))
    m.eval()
    bt = synth.nbest_batch(cfg, labels, 16, S, n_best=5, seed=4, ragged=True, trans_len=16)
    return m, cfg, {k: torch.from_numpy(v).cuda() for k, v in bt.items()}


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def bwd_pair(m, cfg, B, S):
    """ms of the full backward and of the no_param_grad backward on one stash (eval forward, no dropout)"""
    from nbest_amd import hipabi as hb
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1000, 20000, (B, S), generator=g).cuda()
    rec = m._encode(0, ids, None, train=False)
    d, H, L = rec.ps.desc, cfg.hidden_size, cfg.num_hidden_layers
    m._set_weights(d, "backward")
    i, s, p, k = rec.inputs
    act, ws = m._stash[0][:rec.ps.act_bytes], m._ws
    dcls = torch.randn(B, H, device="cuda")
    dh = hb.cls_grad_scatter(dcls, B, S, H, torch.bfloat16)
    grad = torch.zeros_like(m.arena.g)

    def run(npg):
        d.no_param_grad = npg
        hb.check(hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(m.arena.weights), hb.ptr(m.arena.w16t), hb.ptr(m.arena.p),
                                                 None if npg else hb.ptr(grad), hb.ptr(i), hb.ptr(s), hb.ptr(p), hb.ptr(k), hb.ptr(act),
                                                 act.numel(), hb.ptr(dh), hb.ptr(ws), ws.numel(), 0, 0, L, 0, hb.stream_ptr()), "bwd")
        d.no_param_grad = 0
    full, npg = [], []
    for _ in range(5):
        full.append(timed(lambda: run(0), 3))
        npg.append(timed(lambda: run(1), 3))
    return sorted(full)[2], sorted(npg)[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace_only", action="store_true")
    ap.add_argument("--steps", type=int, default=32)
    a = ap.parse_args()
    from nbest_amd.config import LabelSpace
    labels = LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
    for name, L, S in (("bert-base", 12, 128), ("xlm-roberta-large", 24, 256)):
        m, cfg, b = build(name, L, S, labels)
        seg = b["seg"] if cfg.family == "bert" else None
        B = b["ids"].shape[0]
        tg = [(r, c) for r in range(B) for c in (r % labels.n_bottom, (3 * r + 1) % labels.n_bottom)]
        if a.trace_only:
            m.attribute(b["ids"], seg, targets=tg, steps=a.steps)
            torch.cuda.synchronize()
            continue
        ms = [timed(lambda: m.attribute(b["ids"], seg, targets=tg, steps=a.steps), 1) for _ in range(5)]
        med = sorted(ms)[2]
        rows = len(tg) * a.steps + 2 * B
        H, esz = cfg.hidden_size, 2
        print("%s bf16 S=%d m=%d: %d pairs (%d path + %d end rows) in %.2f ms (median of 5, spread %.2f-%.2f) = %.1f pairs/s"
              % (name, S, a.steps, len(tg), len(tg) * a.steps, 2 * B, med, min(ms), max(ms), 1e3 * len(tg) / med))
        print("  bytes: interp forward ~%.1f MB (3 table rows + 1 output row per token), embed_attrib %.1f MB (m S H esz of dhidden per pair)"
              % (rows * S * 4 * H * esz / 1e6, len(tg) * a.steps * S * H * esz / 1e6))
        Bb = 64 if S == 128 else 32
        f, n = bwd_pair(m, cfg, Bb, S)
        print("  backward B=%d S=%d: full %.2f ms, no_param_grad %.2f ms (%.2f x)" % (Bb, S, f, n, n / f))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("done in %.1f s" % (time.time() - t0))
