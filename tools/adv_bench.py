#!/usr/bin/env python3
"""What FGM (--adv_epsilon) costs: the three new launches per call, and the FGM step beside the plain step.

Kernels: hipabi.embed_adv_delta (its two launches), hipabi.embed_ln_fwd with and without delta, hipabi.embed_ln_bwd with and without
delta, on B x S token rows of H 768 (bf16 tables), dropout 0.1; many calls between two events, alternately, queued behind ~ 20 ms of
GEMMs so that the events bracket device time.

Step: train_step at bert-base bf16, S 128, n-best 5, BertAdam, dropout on (hidden 0.1, attention 0.1, heads 0.3): the FGM step
(adv_epsilon 1) against the plain step on the same seeded batches, alternately in one process, timed with device events: median over
the rounds, min..max.

    python tools/adv_bench.py [--rounds 9] [--iters 10] [--layers 12] [--out profiles/adv_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb, synth
from nbest_amd.model import NBestSTCModel, position_ids_for
from nbest_amd.optim import HipBertAdam
from nbest_amd.trainer import limit_host_threads, train_step


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

    def batches():
        out = []
        for s in range(2):
            bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
            out.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
        return out
    data = batches()

    # ---- the embedding kernels alone ---------------------------------------------------------------------------------------------
    H, ar = cfg.hidden_size, model.arena
    pre = "bert_encoder.embeddings."
    word, ttab, ptab = (ar.view(ar.weights, pre + n) for n in ("word_embeddings.weight", "token_type_embeddings.weight", "position_embeddings.weight"))
    gamma, beta = ar.view(ar.p, pre + "LayerNorm.weight"), ar.view(ar.p, pre + "LayerNorm.bias")
    ids, seg = data[0]["ids"].contiguous(), data[0]["seg"].contiguous()
    pos, mask = position_ids_for(cfg, ids), (ids > 0).to(torch.uint8)
    perm = hb.word_perm(ids)
    gen = torch.Generator(device="cuda").manual_seed(3)
    dout = (torch.randn(B * S, H, generator=gen, device="cuda") * 1e-3).bfloat16()
    delta = torch.empty(B * S, H, device="cuda")
    norm = torch.empty(B, device="cuda")
    ws = torch.empty(hb.lib().nbest_embed_adv_ws_bytes(B, S), dtype=torch.uint8, device="cuda")
    kw = dict(drop_p=0.1, seed=5, drop_stream=0)
    eps = cfg.layer_norm_eps
    hb.embed_adv_delta(ids, seg, pos, mask, word, ttab, ptab, gamma, dout, B, S, eps, 1.0, out=delta, norm=norm, ws=ws, **kw)
    _, stats = hb.embed_ln_fwd(ids, seg, pos, word, ttab, ptab, gamma, beta, eps, delta=delta, **kw)
    acc = tuple(torch.zeros_like(t, dtype=torch.float32) for t in (word, ttab, ptab, gamma, beta))
    bw = dict(word_pad_id=cfg.pad_token_id, perm=perm, accumulate_into=acc, **kw)
    klegs = {"embed_adv_delta (2 launches)": lambda i: hb.embed_adv_delta(ids, seg, pos, mask, word, ttab, ptab, gamma, dout, B, S, eps, 1.0,
                                                                        out=delta, norm=norm, ws=ws, **kw),
             "embed_ln_fwd": lambda i: hb.embed_ln_fwd(ids, seg, pos, word, ttab, ptab, gamma, beta, eps, **kw),
             "embed_ln_fwd, delta": lambda i: hb.embed_ln_fwd(ids, seg, pos, word, ttab, ptab, gamma, beta, eps, delta=delta, **kw),
             "embed_ln_bwd": lambda i: hb.embed_ln_bwd(ids, seg, pos, word, ttab, ptab, gamma, stats, dout, B, S, **bw),
             "embed_ln_bwd, delta": lambda i: hb.embed_ln_bwd(ids, seg, pos, word, ttab, ptab, gamma, stats, dout, B, S, delta=delta, **bw)}
    for fn in klegs.values():
        for i in range(10):
            fn(i)
    torch.cuda.synchronize()
    big = torch.randn(8192, 8192, device="cuda").bfloat16()

    def blocker():                             # ~ 20 ms of GEMMs: the calls take the host less than that to enqueue
        for _ in range(12):
            torch.mm(big, big)
    ktimes = {leg: [] for leg in klegs}
    for _ in range(a.rounds):
        for leg, fn in klegs.items():
            ktimes[leg].append(timed(fn, 50, blocker) * 1e3)
    say("embedding kernels, %d x %d token rows, H %d, bf16 tables (delta: %.0f MB fp32), dropout 0.1, queued behind ~ 20 ms of GEMMs so "
        "that the events bracket device time; %d rounds x 50 calls, alternating" % (B, S, H, B * S * H * 4 / 1e6, a.rounds))
    say("(the wrappers of embed_ln_fwd allocate their outputs per call and embed_ln_bwd's its workspace: the same on both sides)")
    say("%-34s %10s %20s" % ("call", "us/call", "spread us"))
    med = {}
    for leg in klegs:
        med[leg] = statistics.median(ktimes[leg])
        say("%-34s %10.2f %9.2f..%-10.2f" % (leg, med[leg], min(ktimes[leg]), max(ktimes[leg])))
    say("forward: delta costs %+.2f us; backward: %+.2f us" % (med["embed_ln_fwd, delta"] - med["embed_ln_fwd"],
                                                               med["embed_ln_bwd, delta"] - med["embed_ln_bwd"]))
    del big, acc

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    legs = {"plain": lambda i: train_step(model, optim, data[i % 2]),
            "adv_epsilon 1": lambda i: train_step(model, optim, data[i % 2], adv_epsilon=1.0)}
    for fn in legs.values():                   # warm-up: buffers sized, kernels loaded, clocks up
        for i in range(4):
            fn(i)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, a.iters))
    say("")
    say("bert-base bf16, %d layers, B %d, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating" % (a.layers, B, S, a.rounds, a.iters))
    say("%-34s %10s %20s" % ("train_step", "ms/step", "spread ms"))
    for leg in legs:
        say("%-34s %10.3f %9.3f..%-10.3f" % (leg, statistics.median(times[leg]), min(times[leg]), max(times[leg])))
    m0, m1 = (statistics.median(times[k]) for k in legs)
    say("the FGM step is %.3f x the plain step (%+.3f ms over twice the plain step)" % (m1 / m0, m1 - 2 * m0))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
