#!/usr/bin/env python3
"""What SAM (--sam_rho) costs: the K9s kernels next to nbest_ema_exchange (K9e) on the arena of the model, and the SAM step beside
the plain step.

Kernels: nbest_sam_perturb (plain and adaptive), nbest_sam_restore, nbest_sam_norms and nbest_bertadam_norms, each over both descriptor
tables as the optimizer launches them, next to nbest_ema_exchange in the same run, alternately, with device events.  Bytes come from
the shapes, per trainable parameter: perturb 18 B (reads p and g, writes the backup, p and the bf16 copy), restore 10 B (reads the
backup, writes p and the bf16 copy), the adaptive norms 8 B (reads p and g), the plain norms 4 B, the exchange 18 B (over every
tensor, the pooler included).  Share of HBM peak against 8 TB/s (MI355X).  A perturb that is not undone would walk the weights
away, so a round times perturb + restore pairs and restore alone, and perturb is the difference; the weights end on their bits.

Step: train_step at bert-base bf16, S 128, n-best 5, BertAdam, dropout on (hidden 0.1, attention 0.1, heads 0.3): SAM (rho 0.05) and
ASAM (rho 0.5, eta 0.01) against the plain step on the same seeded batches, alternately in one process: median over the rounds,
min..max.

    python tools/sam_bench.py [--rounds 9] [--iters 10] [--layers 12] [--out profiles/sam_bench.txt]"""
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
from nbest_amd.trainer import limit_host_threads, train_step

HBM_PEAK = 8.0e12


def timed(fn, iters):
    """ms per call between two device events (every call here is far longer on the device than its enqueue on the host)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0)
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
    data = []
    for s in range(2):
        bt = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
        data.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})

    # ---- the kernels alone, on the model's arenas and the optimizer's descriptor tables ------------------------------------------------
    ar, L, P, st = model.arena, hb.lib(), hb.ptr, hb.stream_ptr
    train_step(model, optim, data[0])                       # a real gradient in arena.g
    torch.cuda.synchronize()
    p0 = ar.p.clone()
    backup, ema = torch.zeros_like(ar.p), ar.p.clone()
    partial = torch.zeros(optim.parts[0][2] + optim.parts[1][2], device="cuda")
    clip = torch.zeros(2, device="cuda")
    n_param = sum(x.numel for x in ar.slots if "pooler" not in x.name)
    n_all = sum(x.numel for x in ar.slots)

    def norms(eta):
        base = 0
        for d, n_t, n_b, _ in optim.parts:
            if eta is None:
                hb.check(L.nbest_bertadam_norms(P(ar.g), P(d), n_t, n_b, 0, n_b, P(partial[base:]), st()), "bertadam_norms")
            else:
                hb.check(L.nbest_sam_norms(P(ar.p), P(ar.g), P(d), n_t, n_b, eta, P(partial[base:]), st()), "sam_norms")
            base += n_b

    def perturb(rho, eta):
        for d, n_t, n_b, _ in optim.parts:
            hb.check(L.nbest_sam_perturb(P(ar.p), P(ar.g), P(backup), P(ar.w16), P(d), n_t, n_b, P(clip[1:2]), rho, eta, st()), "sam_perturb")

    def restore():
        for d, n_t, n_b, _ in optim.parts:
            hb.check(L.nbest_sam_restore(P(ar.p), P(backup), P(ar.w16), P(d), n_t, n_b, st()), "sam_restore")

    def exchange():
        for d, n_t, n_b, _ in optim.parts:
            hb.check(L.nbest_ema_exchange(P(ar.p), P(ema), P(ar.w16), P(d), n_t, n_b, st()), "ema_exchange")

    def pair(rho, eta):
        perturb(rho, eta)
        restore()

    norms(None)
    hb.check(L.nbest_adam_clip_coef(P(partial), partial.numel(), 0.0, P(clip), st()), "adam_clip_coef")
    pair(0.05, -1.0)                                        # the backup holds w from here on: a restore alone is a no-op move
    klegs = [("ema_exchange", lambda i: exchange(), 18 * n_all), ("sam_restore", lambda i: restore(), 10 * n_param),
             ("sam_perturb + sam_restore", lambda i: pair(0.05, -1.0), 28 * n_param),
             ("sam_perturb adaptive + sam_restore", lambda i: pair(0.5, 0.01), 28 * n_param),
             ("sam_norms (adaptive)", lambda i: norms(0.01), 8 * n_param), ("bertadam_norms (plain)", lambda i: norms(None), 4 * n_param)]
    # (ema starts as a clone of p and every perturb is undone, so p and ema hold the same bits throughout: any number of exchanges
    # leaves the weights where they were, which the check after the timed rounds confirms)
    for _, fn, _ in klegs:
        for i in range(4):
            fn(i)
    torch.cuda.synchronize()
    ktimes = {k: [] for k, _, _ in klegs}
    for _ in range(a.rounds):
        for k, fn, _ in klegs:
            ktimes[k].append(timed(fn, a.iters) * 1e3)
    torch.cuda.synchronize()
    assert torch.equal(ar.p.view(torch.int32), p0.view(torch.int32)), "the timed kernels moved the weights"
    say("arena of bert-base (%d layers): %.1f M trainable parameters (pooler excluded), bf16 compute copy, HBM peak %.1f TB/s; %d rounds x "
        "%d calls, alternating, device events; both descriptor tables per call" % (a.layers, n_param / 1e6, HBM_PEAK / 1e12, a.rounds, a.iters))
    say("%-36s %9s %9s %9s %9s %8s %16s" % ("kernel", "median us", "min us", "MB", "TB/s", "% peak", "vs ema_exchange"))
    med = {k: statistics.median(v) for k, v in ktimes.items()}
    rows = [(k, med[k], min(ktimes[k]), nb) for k, _, nb in klegs]
    for name, pk in (("sam_perturb (pair - restore)", "sam_perturb + sam_restore"),
                     ("sam_perturb adaptive (pair - restore)", "sam_perturb adaptive + sam_restore")):
        rows.append((name, med[pk] - med["sam_restore"], min(ktimes[pk]) - min(ktimes["sam_restore"]), 18 * n_param))
    for k, m_us, lo, nbytes in rows:
        tbs = nbytes / (m_us * 1e-6) / 1e12
        say("%-36s %9.1f %9.1f %9.0f %9.2f %7.0f %% %16.3f" % (k, m_us, lo, nbytes / 1e6, tbs, 100 * tbs * 1e12 / HBM_PEAK, m_us / med["ema_exchange"]))
    say("by bytes: perturb 18 / 18 = 1.000 and restore 10 / 18 = 0.556 of ema_exchange (which also moves the pooler's 0.6 M elements).  The "
        "plan for this kernel counted 14 B (8 read, 6 written) and expected 14 / 18 = 0.778: it left out one of the two fp32 stores - "
        "backup and p are both written, 4 + 4 + 2 = 10 B")

    # ---- the step ------------------------------------------------------------------------------------------------------------------------
    legs = {"plain": lambda i: train_step(model, optim, data[i % 2]),
            "sam_rho 0.05": lambda i: train_step(model, optim, data[i % 2], sam_rho=0.05),
            "sam_rho 0.5 adaptive": lambda i: train_step(model, optim, data[i % 2], sam_rho=0.5, sam_adaptive=True, sam_eta=0.01)}
    for fn in legs.values():                   # warm-up: buffers sized, kernels loaded, clocks up
        for i in range(4):
            fn(i)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, a.iters))
    assert torch.isfinite(ar.p).all()
    say("")
    say("bert-base bf16, %d layers, B %d, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating" % (a.layers, B, S, a.rounds, a.iters))
    say("%-34s %10s %20s" % ("train_step", "ms/step", "spread ms"))
    for leg in legs:
        say("%-34s %10.3f %9.3f..%-10.3f" % (leg, statistics.median(times[leg]), min(times[leg]), max(times[leg])))
    m0 = statistics.median(times["plain"])
    for leg in list(legs)[1:]:
        m1 = statistics.median(times[leg])
        say("the %s step is %.3f x the plain step (%+.3f ms against twice the plain step)" % (leg, m1 / m0, m1 - 2 * m0))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
