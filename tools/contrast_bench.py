#!/usr/bin/env python3
"""What the contrastive term costs: nbest_cls_contrast beside nbest_cls_mse and the heads call, and the step with --add_l2_loss
beside the same step with --contrastive_weight on top.

Kernel: hipabi.cls_contrast (keys, both gradients: its four launches) against hipabi.cls_mse (one launch) and hipabi.stc_heads
(need_grad: two launches), all on the CLS rows of 256 utterances of H 768 (bf16, row stride S H as in the step), many calls between
two events, alternately, queued behind ~ 20 ms of GEMMs so that the events bracket device time.

Step: train_step at bert-base bf16, S 128, n-best 5, BertAdam, dropout on (hidden 0.1, attention 0.1, heads 0.3), 256 utterances:
add_l2_loss alone against add_l2_loss + contrast_weight 1 (temperature 0.1).  Both run the transcript pass, so the difference is the
new term: transcript_keys (a B x B x S comparison on the device) and the four launches.  Alternately in one process on the same
seeded batches, timed with device events: median over the rounds, min..max.

    python tools/contrast_bench.py [--rounds 9] [--iters 10] [--layers 12] [--out profiles/contrast_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb, synth
from nbest_amd.model import NBestSTCModel
from nbest_amd.optim import HipBertAdam
from nbest_amd.trainer import limit_host_threads, train_step, transcript_keys


def timed(fn, iters, blocker=None):
    """ms per call between two device events.  ``blocker``: enqueued ahead of the first event - device work long enough for the host
    to queue all ``iters`` calls behind it, so that the events bracket back-to-back device time and not the host's launch rate"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
    if blocker is not None:
        blocker()
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    limit_host_threads()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, S = a.utterances, a.seq_len
    cfg = ncfg.bert_base(num_hidden_layers=a.layers)
    model = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.3, seed=999)
    model.load_reference_state(synth.model_state(cfg, labels, seed=1))
    model.train()
    optim = HipBertAdam(model, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=100000)

    # ---- the kernels alone ---------------------------------------------------------------------------------------------------------
    H = cfg.hidden_size
    gen = torch.Generator(device="cuda").manual_seed(3)
    dls = model.dls
    R, nb = dls.n_rows, labels.n_bottom
    St = 32                                                        # the transcript pass is shorter
    ha = torch.randn(B * S, H, generator=gen, device="cuda").bfloat16()
    ht = (0.5 * ha.view(B, S, H)[:, :St, :].float() + torch.randn(B, St, H, generator=gen, device="cuda")).bfloat16().reshape(B * St, H)
    keys = torch.arange(B, device="cuda")
    keys[1::7] = keys[0]                                           # repeated transcripts
    Wh, bh = model.arena.heads_wb()
    y = (torch.rand(B, nb, generator=gen, device="cuda") < 0.02).float()
    dWh, dbh = torch.zeros(R, H, device="cuda"), torch.zeros(R, device="cuda")
    da, dt = torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")
    cws = torch.empty(hb.cls_contrast_ws_bytes(B, H), dtype=torch.uint8, device="cuda")
    kw = dict(need_grad=True, drop_p=0.3, seed=5, drop_stream=900, dWh=dWh, dbh=dbh, ws=hb.heads_ws(B, R, H, "cuda"))
    klegs = {"stc_heads (2 launches)": lambda i: hb.stc_heads(ha, S * H, Wh, bh, dls, y, B, H, **kw),
             "cls_mse (1 launch)": lambda i: hb.cls_mse(ha, S * H, ht, St * H, B, H, da, dt),
             "cls_contrast (4 launches)": lambda i: hb.cls_contrast(ha, S * H, ht, St * H, B, H, 1.0, 0.1, keys=keys, da=da, dt=dt,
                                                                    accumulate_dt=True, ws=cws),
             "cls_contrast, loss only": lambda i: hb.cls_contrast(ha, S * H, ht, St * H, B, H, 1.0, 0.1, keys=keys, ws=cws)}
    for fn in klegs.values():
        for i in range(20):
            fn(i)
    torch.cuda.synchronize()
    big = torch.randn(8192, 8192, device="cuda").bfloat16()

    def blocker():                             # ~ 20 ms of GEMMs: 200 calls take the host less than that to enqueue
        for _ in range(12):
            torch.mm(big, big)
    ktimes = {leg: [] for leg in klegs}
    for _ in range(a.rounds):
        for leg, fn in klegs.items():
            ktimes[leg].append(timed(fn, 200, blocker) * 1e3)
    say("%d utterances, H %d, R %d, bf16 CLS rows at row stride S H (S %d / %d), queued behind ~ 20 ms of GEMMs so that the events "
        "bracket device time; %d rounds x 200 calls, alternating" % (B, H, R, S, St, a.rounds))
    say("%-34s %10s %20s" % ("call", "us/call", "spread us"))
    for leg in klegs:
        say("%-34s %10.2f %9.2f..%-10.2f" % (leg, statistics.median(ktimes[leg]), min(ktimes[leg]), max(ktimes[leg])))
    k_heads, k_mse, k_con, _ = (statistics.median(ktimes[k]) for k in klegs)
    say("cls_contrast is %.2f x the heads call and %.2f x cls_mse" % (k_con / k_heads, k_con / k_mse))
    del big

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    batches = []
    for s in range(2):
        bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True, trans_len=St)
        bt = {k: torch.from_numpy(v).cuda() for k, v in bt.items()}
        bt["tids"][1::7], bt["tseg"][1::7] = bt["tids"][0], bt["tseg"][0]          # repeated transcripts, as in the real batches
        batches.append(bt)
    tk = transcript_keys(batches[0]["tids"])
    legs = {"add_l2_loss": lambda i: train_step(model, optim, batches[i % 2], add_l2_loss=True),
            "add_l2_loss + contrast_weight 1": lambda i: train_step(model, optim, batches[i % 2], add_l2_loss=True, contrast_weight=1.0),
            "plain (one pass)": lambda i: train_step(model, optim, batches[i % 2])}
    for fn in legs.values():                   # warm-up: buffers sized, kernels loaded, clocks up
        for i in range(4):
            fn(i)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, a.iters))
    say("")
    say("bert-base bf16, %d layers, %d utterances, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating; %d distinct "
        "transcript keys in batch 0" % (a.layers, B, S, a.rounds, a.iters, tk.unique().numel()))
    say("%-34s %10s %20s" % ("train_step", "ms/step", "spread ms"))
    for leg in legs:
        say("%-34s %10.3f %9.3f..%-10.3f" % (leg, statistics.median(times[leg]), min(times[leg]), max(times[leg])))
    m0, m1, _ = (statistics.median(times[k]) for k in legs)
    say("the contrastive term on top of the two-pass step: %+.3f ms (%+.2f %%)" % (m1 - m0, 100 * (m1 - m0) / m0))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
