#!/usr/bin/env python3
"""What distillation costs per step, and what the kd instantiation of the heads kernel costs beside the plain one.

Step: train_step at the bench shape (bert-base student of 6 layers, bf16, B 256, S 128, n-best 5, BertAdam, dropout on: hidden 0.1,
attention 0.1, heads 0.3) without a teacher, with a 12-layer bf16 teacher (teacher.predict ahead of every step) and with that
teacher at temperature 2 (its logits: one more launch in predict, the kd_t heads kernel in the step), alternately in one process on
the same seeded batches, timed with device events: median over the rounds, min..max as the spread.

Kernel: hipabi.stc_heads against hipabi.stc_heads_kd (alpha 0.5) and hipabi.stc_heads_kd_t (alpha 0.5, T 2) on B 256 CLS rows of
H 768, dropout 0.3, need_grad: the two launches of each (forward + backward), many calls between two events, alternately; and
hipabi.stc_heads_logits (one launch) in the same protocol.

    python tools/distill_bench.py [--rounds 9] [--iters 10] [--out profiles/distill_bench.txt]"""
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
from nbest_amd.trainer import limit_host_threads, student_state_from_teacher, train_step


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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--student_layers", type=int, default=6)
    ap.add_argument("--teacher_layers", type=int, default=12)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    limit_host_threads()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = ncfg.LabelSpace.from_json(os.path.join(root, "tests", "golden", "label_space.json"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, S = a.batch, a.seq_len
    tcfg = ncfg.bert_base(num_hidden_layers=a.teacher_layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    teacher = NBestSTCModel(tcfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, seed=999)
    tsd = synth.model_state(tcfg, labels, seed=1)
    teacher.load_reference_state(tsd)
    teacher.eval()
    scfg = ncfg.bert_base(num_hidden_layers=a.student_layers)
    student = NBestSTCModel(scfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.3, seed=999)
    step = max(1, a.teacher_layers // a.student_layers)
    student.load_reference_state(student_state_from_teacher({k: torch.as_tensor(v) for k, v in tsd.items()},
                                                            [min(step * (k + 1) - 1, a.teacher_layers - 1) for k in range(a.student_layers)]))
    student.train()
    optim = HipBertAdam(student, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=100000)
    batches = []
    for s in range(2):
        bt = synth.nbest_batch(scfg, labels, B, S, n_best=5, seed=11 + s, ragged=True)
        batches.append({k: torch.from_numpy(v).cuda() for k, v in bt.items()})
    legs = {"no teacher": lambda i: train_step(student, optim, batches[i % 2]),
            "teacher": lambda i: train_step(student, optim, batches[i % 2], teacher=teacher, distill_alpha=0.5),
            "teacher, T = 2": lambda i: train_step(student, optim, batches[i % 2], teacher=teacher, distill_alpha=0.5, distill_temperature=2.0),
            "teacher.predict": lambda i: teacher.predict(batches[i % 2]["ids"], seg_ids=batches[i % 2]["seg"])}
    for fn in legs.values():                   # warm-up: buffers sized, kernels loaded, clocks up
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, a.iters))
    say("bert-base bf16, student %d layers, teacher %d layers, B %d, S %d, dropout on, BertAdam; %d rounds x %d steps, alternating"
        % (a.student_layers, a.teacher_layers, B, S, a.rounds, a.iters))
    say("%-34s %10s %20s %12s" % ("leg", "ms/step", "spread ms", "utt/s"))
    for leg in legs:
        med = statistics.median(times[leg])
        say("%-34s %10.3f %9.3f..%-10.3f %12.0f" % ("train_step, " + leg if leg != "teacher.predict" else leg, med, min(times[leg]),
                                                     max(times[leg]), B / med * 1e3))
    m0, m1, mp = (statistics.median(times[k]) for k in ("no teacher", "teacher", "teacher.predict"))
    say("the teacher adds %.3f ms per step (%.1f %%); its predict alone takes %.3f ms" % (m1 - m0, 100 * (m1 - m0) / m0, mp))
    mt = statistics.median(times["teacher, T = 2"])
    say("the temperature adds %.3f ms to the step with a teacher (%.2f %%)" % (mt - m1, 100 * (mt - m1) / m1))

    # ---- the heads kernel alone ----------------------------------------------------------------------------------------------------
    H = scfg.hidden_size
    gen = torch.Generator(device="cuda").manual_seed(3)
    dls = student.dls
    R, nt, nb = dls.n_rows, labels.n_top, labels.n_bottom
    hidden = torch.randn(B, H, generator=gen, device="cuda").bfloat16()
    Wh, bh = student.arena.heads_wb()
    y = (torch.rand(B, nb, generator=gen, device="cuda") < 0.02).float()
    with torch.no_grad():
        t = teacher.predict(batches[0]["ids"], seg_ids=batches[0]["seg"], return_logits=True)
    dWh, dbh = torch.zeros(R, H, device="cuda"), torch.zeros(R, device="cuda")
    kw = dict(need_grad=True, drop_p=0.3, seed=5, drop_stream=900, dWh=dWh, dbh=dbh, ws=hb.heads_ws(B, R, H, "cuda"))
    klegs = {"stc_heads": lambda i: hb.stc_heads(hidden, H, Wh, bh, dls, y, B, H, **kw),
             "stc_heads_kd": lambda i: hb.stc_heads_kd(hidden, H, Wh, bh, dls, y, t["top"], t["bott"], t["final"], 0.5, B, H, **kw),
             "stc_heads_kd_t (T = 2)": lambda i: hb.stc_heads_kd_t(hidden, H, Wh, bh, dls, y, t["logits"], 0.5, 2.0, B, H, **kw),
             "stc_heads_logits (one launch)": lambda i: hb.stc_heads_logits(hidden, H, Wh, bh, dls, B, H)}
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
    say("")
    say("K7, B %d, H %d, R %d, bf16 CLS rows, dropout 0.3, forward + backward launches (stc_heads_logits: its one launch, no dropout), queued behind ~ 20 ms of GEMMs so that the "
        "events bracket device time; %d rounds x 200 calls, alternating" % (B, H, R, a.rounds))
    say("%-34s %10s %20s" % ("call", "us/call", "spread us"))
    for leg in klegs:
        say("%-34s %10.2f %9.2f..%-10.2f" % (leg, statistics.median(ktimes[leg]), min(ktimes[leg]), max(ktimes[leg])))
    k0, k1, k2 = (statistics.median(ktimes[k]) for k in ("stc_heads", "stc_heads_kd", "stc_heads_kd_t (T = 2)"))
    say("stc_heads_kd - stc_heads %+.2f us; stc_heads_kd_t - stc_heads_kd %+.2f us" % (k1 - k0, k2 - k1))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
