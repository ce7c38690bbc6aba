#!/usr/bin/env python3
"""Headline benchmark: fine-tuning throughput (utterances/s) of the HIP hot path on synthetic n-best
sequences - BASELINE.json configs[1]: bert-base-uncased shape, bf16, n_best=5, seq_len=128, batch 256 per
GPU; one process per GPU (torchrun), data-parallel over RCCL, weak scaling.

A step = forward (embeddings, 12 layers, STC heads + losses) + backward + gradient all-reduce +
BertAdam (per-tensor clip) with dropout ON (hidden 0.1, attention 0.1, heads 0.3, the shipped script's
values).  Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def _self_launch():
    """`python bench.py --gpus N` with N > 1 and no RANK in the environment: this process (which has imported nothing
    that could touch a GPU) starts one child per GPU through torch.distributed.run on 127.0.0.1, relays their output
    (rank 0 prints the JSON line) and exits with the launcher's code.  Nothing is exec'd."""
    if "RANK" in os.environ:
        return
    n = 1
    for i, tok in enumerate(sys.argv):
        if tok == "--gpus" and i + 1 < len(sys.argv):
            n = int(sys.argv[i + 1])
        elif tok.startswith("--gpus="):
            n = int(tok.split("=", 1)[1])
    if n <= 1:
        return
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.run(cmd, env=env).returncode)


if __name__ == "__main__":
    _self_launch()

import numpy as np
import torch
import torch.distributed as dist

import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, synth, hipabi as hb
from nbest_amd.model import NBestSTCModel
from nbest_amd.optim import HipBertAdam
from nbest_amd.trainer import GradReducer, broadcast_parameters, init_distributed, train_step

PEAK_BF16_TFLOPS = 2500.0      # dense MFMA peak, MI355X (MI355X_MICROARCH.md)
PEAK_FP8_TFLOPS = 5000.0       # dense fp8 MFMA peak (same guide); the fp8w mode's GEMMs are priced against this one


def wgrad_traffic_from_profiles(fp8=False):
    """HBM bytes per weight-gradient launch (the GEMM plus its split-K reduce) from the newest tracked PMC table
    profiles/rNN_pmc.csv (tools/profile_step.sh: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this very
    command, gfx950 corrections applied by tools/pmc_table.py).  Returns (bytes or None, provenance string)."""
    import csv
    import glob
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.csv")) if ("fp8w" in os.path.basename(f)) == fp8)
    if not files:
        return None, "no profiles/r*_%spmc.csv" % ("fp8w_" if fp8 else "")
    total, launches = 0.0, 0.0
    with open(files[-1]) as f:
        for row in csv.DictReader(f):
            k = row["kernel"]
            if fp8:
                is_gemm = "gemm8tt_kernel" in k
            else:
                kk = k.replace(", false>", ">").replace(", true>", ">") if "gemm2_kernel" in k else k    # trailing experiment flag of gemm2_kernel
                is_gemm = ("gemm2_kernel" in k or "gemm_bf16_kernel" in k) and kk.rstrip(">").endswith(", 6")   # EPI = F32_SPLITK
            if not (is_gemm or ("splitk_reduce8" in k if fp8 else ("splitk_reduce" in k and "reduce8" not in k))):
                continue
            n, tb = float(row["launches_per_step"]), float(row["traffic_bytes_per_launch"])
            if tb != tb:
                continue
            total += n * tb
            if is_gemm:
                launches += n
    if not launches:
        return None, "no weight-gradient rows in %s" % os.path.basename(files[-1])
    return total / launches, "profiles/%s (rocprofv3 --pmc, FETCH_SIZE x2 x1024 + WRITE_SIZE x1024, GEMM + split-K reduce)" % os.path.basename(files[-1])


def flops_per_utt(cfg, S, St=0):
    """3 x L*S*(24 H^2 + 4 S H) (+ the transcript pass when --add_l2_loss)"""
    H, L = cfg.hidden_size, cfg.num_hidden_layers
    f = lambda s: L * s * (24 * H * H + 4 * s * H)
    return 3.0 * (f(S) + (f(St) if St else 0))


def cpu_baseline(labels, seconds_budget=25.0):
    """the oracle (CPU restatement, kind "port") timed on this box's host cores at BASELINE configs[0]'s
    shape: bert-base fp32, B=8, S=128, n_best=5: forward + losses + backward + BertAdam."""
    from oracle.encoder import EncoderConfig as OCfg
    from oracle.model import OracleModel
    from oracle.bertadam import OracleBertAdam
    from oracle.step import train_step as oracle_step
    from oracle import stc
    # the GPU box reports the host's cores but grants a 16-core share per GPU: more threads than that thrash
    cores = max(1, min(len(os.sched_getaffinity(0)), os.cpu_count() or 1, 16))
    torch.set_num_threads(cores)
    cfg = ncfg.bert_base()
    ocfg = OCfg(**{k: v for k, v in cfg.to_dict().items() if k in OCfg.__dataclass_fields__})
    torch.manual_seed(999)
    om = OracleModel(ocfg, labels.top2bottom, labels.n_bottom, 0.3)
    om.train()
    b = synth.nbest_batch(cfg, labels, 8, 128, n_best=5, seed=999, trans_len=32)
    t = {k: torch.from_numpy(v) for k, v in b.items()}
    opt = OracleBertAdam(list(om.named_parameters()), lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=1000)
    b2t = stc.bottom2top_matrix(labels.top2bottom)
    # What the reference's loop does per step (n_best_asr_bert.py:250-255 -> models/model.py:51-58): BOTH encoder passes - the
    # transcript pass runs and is discarded unless --add_l2_loss (quirk Q4).  `value` times exactly that; the variant that skips
    # the unused pass (what this build's GPU path does) is reported next to it.
    def rate(skip, budget):
        oracle_step(om, opt, t, labels.top2bottom, b2t, skip_unused_transcript=skip)      # warm-up
        n, t0 = 0, time.time()
        while n < 3 or (time.time() - t0 < budget and n < 12):
            oracle_step(om, opt, t, labels.top2bottom, b2t, skip_unused_transcript=skip)
            n += 1
        return 8 * n / (time.time() - t0), n
    full, n_full = rate(False, seconds_budget * 0.45)
    lean, n_lean = rate(True, seconds_budget * 0.3)
    return dict(value=round(full, 3), unit="utterances/s", cores=torch.get_num_threads(), kind="port",
                sample="%d steps of bert-base fp32 B=8 S=128 S_t=32 n_best=5 (ASR pass + the transcript pass the reference always runs, "
                       "losses, backward, BertAdam), oracle on CPU" % n_full,
                without_unused_transcript_pass=round(lean, 3), sample_without="%d steps" % n_lean)


def time_wgrad_in_step(model, step, B, S, n_steps=3, operand_bytes=2.0):
    """The kernel with the largest share of the step (profiles/): the weight-gradient GEMM dW = dY^T . X over the
    M = B*S token rows (split-K, fp32 out), launched four times per layer (FFN-down, FFN-up, attention-out, QKV).
    Timed IN the training step, on the launch stream, with HIP events the library records around each of the 4 L
    launches (nbest_encoder_desc::wgrad_events; a launch = the GEMM kernel + its split-K reduce): `n_steps` further
    steps right after the timed region, same cache / clock / power state as the step itself.
    Returns (avg ms per launch, avg algorithmic flops per launch, avg algorithmic bytes per launch = both operands (bf16, or
    e4m3 in the fp8w mode: `operand_bytes`) read once + the fp32 gradient written once)."""
    import ctypes as C
    cfg = model.cfg
    H, F, L, M = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, B * S
    n_ev = 8 * L
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
    for e in evs:
        e.record()                                  # torch creates the hipEvent_t lazily, at the first record
    torch.cuda.synchronize()
    arr = (C.c_void_p * n_ev)(*[e.cuda_event for e in evs])
    desc = model._pass(B, S, 0).desc
    from nbest_amd import hipabi as hb
    per_layer = hb.lib().nbest_encoder_wgrad_launches_per_layer(C.byref(desc))   # 3: QKV + attention-out share a launch (bf16)
    desc.wgrad_events, desc.wgrad_events_n = C.cast(arr, C.POINTER(C.c_void_p)), n_ev
    tot, n = 0.0, 0
    try:
        for _ in range(n_steps):
            step()
            torch.cuda.synchronize()
            for i in range(per_layer * L):
                tot += evs[2 * i].elapsed_time(evs[2 * i + 1])
                n += 1
    finally:
        desc.wgrad_events, desc.wgrad_events_n = None, 0
    shapes = [(H, F), (F, H), (H, H), (3 * H, H)]
    flops = sum(2.0 * M * a * b for a, b in shapes) / per_layer
    byts = sum(operand_bytes * M * (a + b) + 4.0 * a * b for a, b in shapes) / per_layer
    return tot / n, flops, byts, per_layer


def note(msg):
    print("[bench] " + msg, file=sys.stderr, flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out, model, d, per_tensor=4096, seed=1234):
    """--dump-outputs: what the timed path computed in its LAST step, as float32 DIR/<name>.npy - the arrays train_step returns
    (top, bott, final, loss_parts, asr_cls[, trans_cls]) and, for every parameter tensor in slot order, the same fixed seeded sample
    of min(numel, per_tensor) elements of the fp32 master weights the step updated (params_sample) and of the gradients it left in
    the arena (grads_sample).  Called right after the timed region, before anything else runs a step."""
    os.makedirs(d, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in out.items() if v is not None}
    rng = np.random.default_rng(seed)
    idx = np.concatenate([s.offset + np.sort(rng.choice(s.numel, min(s.numel, per_tensor), replace=False)) for s in model.arena.slots])
    idx = torch.from_numpy(idx).to(model.arena.p.device)
    host["params_sample"] = model.arena.p[idx].cpu().numpy()
    host["grads_sample"] = model.arena.g[idx].cpu().numpy()
    total = sum(v.nbytes for v in host.values())
    assert total <= DUMP_LIMIT_BYTES, "dump of %d bytes exceeds the %d-byte limit" % (total, DUMP_LIMIT_BYTES)
    for k, v in host.items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(v, dtype=np.float32))
    note("dumped %s (%.1f MB) to %s" % (", ".join(sorted(host)), total / 1e6, d))


def real_data_throughput(model, optim, labels, batch_size, n_best, epochs=2, min_utts=16384):
    """VERDICT r3 item 8 / SURVEY 8f-1: the REAL-data loop - the shipped `valid` split (tests/golden/valid_512.txt: 512 lines of
    the reference's dstc2 valid file) tiled to >= 16 k utterances, through trainer.EncodedSplit (tokenised once) + Prefetcher
    (pinned host batches, side-stream H2D) + trainer.train_epoch (the step, the device decode and the host F1 bookkeeping of
    /root/reference/n_best_asr_bert.py:232-294).  Batches pad to their own longest row, so the comparable quantity is PADDED
    TOKENS per second.  Returns a dict for the JSON line; epoch 0 warms the shape cache, the last epoch is the one reported."""
    import types
    from nbest_amd import inputs, trainer
    vocab = json.load(open(os.path.join(ROOT, "tests", "golden", "text_vocab.json")))
    z = np.load(os.path.join(ROOT, "tests", "golden", "case_text.npz"))
    memory = dict(label2idx=json.loads(str(z["label2idx"])), idx2label=labels.idx2label)
    data = trainer.read_wcn_data(os.path.join(ROOT, "tests", "golden", "valid_512.txt"))
    reps = (min_utts + len(data[0]) - 1) // len(data[0])
    data = tuple(list(x) * reps for x in data)
    opt = types.SimpleNamespace(batchSize=batch_size, tokenizer=inputs.WordPieceTokenizer(vocab), pre_trained_model="bert",
                                tod_pre_trained_model=None, without_system_act=False, add_l2_loss=False, add_segment_ids=True,
                                n_best=n_best, max_seq_len=None, random_seed=999, optimizer=optim)
    t0 = time.time()
    split = trainer.EncodedSplit(data, opt, memory)
    t_tok = time.time() - t0
    lens = np.array([len(r[0]) for r in split.rows])
    res = {}
    for ep in range(epochs):
        lists = trainer.batch_indices(len(split), batch_size, shuffle=True, seed=999 + ep)
        padded = int(sum(len(ix) * lens[ix].max() for ix in lists))
        torch.cuda.synchronize()
        t0 = time.time()
        loss, (p, r, f), acc = trainer.train_epoch(model, split, opt, memory, epoch=ep)
        torch.cuda.synchronize()
        dt = time.time() - t0
        res = dict(utterances=len(split), epochs=epochs, reported_epoch=ep, batch=batch_size, n_best=n_best, steps=len(lists),
                   seconds=round(dt, 3), utterances_per_s=round(len(split) / dt, 1), padded_tokens=padded,
                   padded_tokens_per_s=round(padded / dt, 0), mean_padded_len=round(padded / len(split), 1),
                   max_len=int(lens.max()), tokenise_once_s=round(t_tok, 2), loss=round(float(loss), 3), f1=round(float(f), 2),
                   includes="EncodedSplit batches from pinned memory (Prefetcher, side-stream H2D), train_step, device decode + host F1 "
                            "bookkeeping one step behind (MetricsPipe), no host synchronisation inside the epoch")
        note("real data epoch %d: %.2f s, %.0f utt/s, %.0f padded tokens/s (mean padded length %.1f)" % (
            ep, dt, len(split) / dt, padded / dt, padded / len(split)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="utterances per GPU per step")
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--n_best", type=int, default=5)
    ap.add_argument("--model", default="bert", choices=["bert", "xlm-roberta", "xlm-roberta-large"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "fp8w"],
                    help="fp8w: forward GEMMs on the block-scaled fp8 MFMA from an e4m3 weight copy (reported separately, never the headline)")
    ap.add_argument("--add_l2_loss", action="store_true")
    ap.add_argument("--no_dropout", action="store_true")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--no_roofline", action="store_true", help="skip the in-step event timing (profiler passes)")
    ap.add_argument("--shard_optimizer", default="off", choices=["auto", "on", "off"],
                    help="data parallel: BertAdam sharded over the ranks (auto: models over 200 M parameters - see DESIGN 6)")
    ap.add_argument("--no_packed_weights", action="store_true", help="A/B diagnostic: the GEMMs read the weight matrices row by row (round-2 behaviour)")
    ap.add_argument("--real", action="store_true", help="after the synthetic measurement: the real-data loop (shipped valid split tiled to 16 k utterances "
                    "through EncodedSplit + Prefetcher + train_epoch, decode and F1 included) as a second JSON key `real_data` (N = 1 only)")
    ap.add_argument("--epochs", type=int, default=2, help="--real: epochs over the tiled split (the last one is reported)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps: write what the last timed step computed (its outputs, a fixed sample of the updated "
                         "weights and of the gradients) as float32 DIR/<name>.npy (rank 0; not with the sharded optimizer)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    from nbest_amd import trainer as _trainer
    _trainer.limit_host_threads()            # the container's CPU quota, not the machine's core count (trainer.limit_host_threads)

    # NBEST_BENCH_REHEARSAL=1: the N ranks share cuda:0 and talk through gloo - the whole multi-rank code path (sharded optimizer,
    # reduce-to-owner buckets, sparse row exchange, tear-down, rank 0's extra measurements) on a ONE-GPU box; its timings mean nothing
    rehearsal = os.environ.get("NBEST_BENCH_REHEARSAL") == "1"
    rank, world, local = init_distributed("gloo" if rehearsal else None)
    if rehearsal:
        local = 0
    assert world == a.gpus, "launch with torchrun --nproc-per-node %d (WORLD_SIZE=%d)" % (a.gpus, world)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    labels = ncfg.LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
    cfg = ncfg.NAMED[a.model]()
    if a.no_dropout:
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    dtype = torch.float32 if a.dtype == "f32" else torch.bfloat16
    model = NBestSTCModel(cfg, labels, device=dev, compute_dtype=dtype, dropout=0.0 if a.no_dropout else 0.3, seed=999,
                          fp8_forward=(a.dtype == "fp8w"))
    if a.no_packed_weights:
        model.arena.wpk = model.arena.wpkt = model.arena.w8p = model.arena.w8tp = None
    model.load_reference_state(synth.model_state(cfg, labels, seed=999))     # random init of the named architecture
    broadcast_parameters(model)
    model.train()
    St = a.seq_len // 4 if a.add_l2_loss else 0
    b = synth.nbest_batch(cfg, labels, a.batch, a.seq_len, n_best=a.n_best, seed=999 + rank, trans_len=St or None)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    # rows of the word-embedding table this shard touches, built on the host like trainer.EncodedSplit does: under data
    # parallelism a 250 002-row table (XLM-R) exchanges these rows instead of all-reducing 768 MB (trainer.GradReducer)
    batch["word_rows"] = torch.from_numpy(np.unique(np.concatenate([b[k].ravel() for k in ("ids", "tids") if k in b]))).to(dev)
    # ... and the tokens sorted by word id (stable): the index of the deterministic embedding backward, built by the data loader next
    # to ids (trainer.EncodedSplit.host_batch does the same for real data); a pure function of ids, resident like them
    for k, pk in (("ids", "tok_perm"), ("tids", "ttok_perm")):
        if k in b:
            batch[pk] = torch.from_numpy(np.argsort(b[k].ravel(), kind="stable").astype(np.int32)).to(dev)
    t_total = 100000
    distributed = dist.is_available() and dist.is_initialized()
    dist_backend = dist.get_backend() if distributed else None     # "nccl" = RCCL; recorded in the JSON line
    # data parallel: the optimizer sharded over the ranks (gradients reduced to the owner of each arena range, owners broadcast the bf16
    # compute copy: 0.75 x the bytes of the all-reduce, 1/N of the BertAdam traffic per GPU) where the replicated update is the larger
    # cost - models over 200 M parameters (XLM-R); at bert-base the N sequential owner broadcasts after the update (21 MB each, not
    # overlappable with anything) cost about what the 0.57 ms replicated update does, so the plain all-reduce path stays
    n_params = sum(s.numel for s in model.arena.slots)
    shard = distributed and (a.shard_optimizer == "on" or (a.shard_optimizer == "auto" and n_params > 200e6))
    if shard and a.dump_outputs:
        sys.exit("--dump-outputs: the sharded optimizer leaves rank 0 with part of the weights and gradients only")
    optim = HipBertAdam(model, lr=3e-5, bert_lr=3e-5, warmup=0.1, t_total=t_total, shard=shard)
    reducer = GradReducer(model.arena, owner_ranges=optim.owner_ranges) if distributed else None

    def step():
        return train_step(model, optim, batch, add_l2_loss=a.add_l2_loss, add_segment_ids=True, reducer=reducer)

    if rank == 0:
        note("model + batch resident on %s; warm-up %d steps" % (dev, a.warmup))
    for i in range(a.warmup):
        step()
        if i == 0:
            torch.cuda.synchronize()
            if rank == 0:
                note("first step done")
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    if rank == 0:
        note("timing %d steps" % a.steps)
    t0 = time.time()
    for _ in range(a.steps):
        out = step()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.time() - t0
    if distributed:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = tt.item()
    loss = float(out["loss_parts"].sum().item())
    assert np.isfinite(loss), "non-finite loss in the timed region"
    if a.dump_outputs and rank == 0:
        dump_outputs(out, model, a.dump_outputs)
    if distributed:
        # every rank leaves the process group together, right after the timed region: rank 0's extra measurements
        # below (dominant-kernel timing) must not keep its peers waiting inside a communicator tear-down
        dist.barrier()
        dist.destroy_process_group()
        reducer = None            # rank 0's in-step kernel timing below runs its extra steps without a gradient exchange
        optim.sharded = False     # ... and without the sharded optimizer's collectives (a replicated update of its stale copy: timing only)

    if rank == 0:
        note("timed region: %.3f s, %.1f utt/s" % (dt, a.batch * world * a.steps / dt))
        utt = a.batch * world * a.steps / dt
        fpu = flops_per_utt(cfg, a.seq_len, St)
        if a.model == "bert" and a.seq_len == 128 and a.n_best == 5 and a.batch == 256 and not a.add_l2_loss:
            cfg_label = "BASELINE configs[1]"
        elif a.model == "xlm-roberta" and a.seq_len == 128 and a.n_best == 5:
            cfg_label = "BASELINE configs[2] per-GPU shard (global 256 / DP 8 = 32)" if a.batch == 32 else "BASELINE configs[2] shape"
        elif a.model == "bert" and a.add_l2_loss and a.seq_len == 256 and a.n_best == 10:
            cfg_label = "BASELINE configs[3] shape"
        elif a.model == "xlm-roberta-large" and a.seq_len == 256:
            cfg_label = "BASELINE configs[4] shape" + ("" if a.dtype == "fp8w" else " in bf16 (configs[4] itself is --dtype fp8w)")
        else:
            cfg_label = "custom shape"
        res = {
            "metric": "utterances/sec fine-tune (bert-base, seq128, n_best=5)" if a.model == "bert" else "utterances/sec fine-tune (%s)" % a.model,
            "value": round(utt, 2), "unit": "utterances/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(1000 * dt / a.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": "%s: %s shape (random init), %s, synthetic n_best=%d seq_len=%d, batch %d per GPU, "
                                   "fwd+losses+bwd+allreduce+BertAdam%s%s, dropout %s" % (
                                       cfg_label, {"bert": "bert-base-uncased", "xlm-roberta": "xlm-roberta-base"}.get(a.model, a.model), a.dtype,
                                       a.n_best, a.seq_len, a.batch, " + transcript pass and CLS-MSE (--add_l2_loss)" if a.add_l2_loss else "",
                                       "; fp8w = forward, dgrad and weight-gradient GEMMs on the block-scaled fp8 MFMA (e4m3 weight copy, "
                                       "e4m3 activation / gradient copies), everything else bf16, fp32 master weights" if a.dtype == "fp8w" else "",
                                       "off" if a.no_dropout else "on (0.1/0.1/0.3)"),
                       "global_batch": a.batch * world, "seq_len": a.seq_len, "n_best": a.n_best, "parallelism": "dp%d" % world,
                       "add_l2_loss": bool(a.add_l2_loss)},
            **({"rehearsal": "N ranks on ONE GPU over gloo: code-path check, not a measurement"} if rehearsal else {}),
            "dist_backend": dist_backend,
            "flops_per_utterance": fpu,
            "step_mfma_frac": round(utt * fpu / 1e12 / ((PEAK_FP8_TFLOPS if a.dtype == "fp8w" else PEAK_BF16_TFLOPS) * world), 4),
            "last_loss_per_utt": round(loss / a.batch, 4),
        }
        if a.dtype in ("bf16", "fp8w") and not a.no_roofline:
            f8 = a.dtype == "fp8w"
            peak = PEAK_FP8_TFLOPS if f8 else PEAK_BF16_TFLOPS
            ms, fl, by, wpl = time_wgrad_in_step(model, step, a.batch, a.seq_len, operand_bytes=1.0 if f8 else 2.0)
            ach = fl / (ms * 1e-3) / 1e12
            traffic, src = wgrad_traffic_from_profiles(f8) if (a.model == "bert" and a.batch == 256 and a.seq_len == 128) else (None, "not measured for this shape")
            H_, F_ = cfg.hidden_size, cfg.intermediate_size
            kern = ("gemm8tt_kernel (e4m3 x e4m3 on v_mfma_scale_f32_32x32x64_f8f6f4, ds_read_b64_tr_b8 transposed reads) + splitk_reduce8_kernel" if f8 else
                    "gemm2_kernel<256,256,...,true,true,F32_SPLITK> + splitk_reduce2_kernel; the QKV and attention-output gradients of a layer "
                    "share one launch (nbest_wgrad_pair: 27 + 9 output tiles)" if wpl == 3 else
                    "gemm2_kernel<256,256,...,true,true,F32_SPLITK> for QKV/FFN, gemm_bf16_kernel<true,true,F32_SPLITK> for the attention "
                    "output, each followed by its split-K reduce")
            res["roofline"] = {"bound": "mfma", "achieved": round(ach, 1), "peak": peak, "unit": "TFLOP/s",
                               "frac": round(ach / peak, 4), "traffic": traffic, "traffic_source": src,
                               "kernel": "weight-gradient GEMM dW = dY^T.X (both operands token-major, transposed LDS reads, split-K, fp32 "
                                         "out; %s), K = %d token rows; avg over the %d launches of a layer: %dx%d, %dx%d, %s" % (
                                             kern, a.batch * a.seq_len, wpl, H_, F_, F_, H_,
                                             "%dx%d + %dx%d" % (3 * H_, H_, H_, H_) if wpl == 3 else "%dx%d, %dx%d" % (H_, H_, 3 * H_, H_)),
                               "timing": "HIP events recorded by the library around each of the %d launches per step, on the launch "
                                         "stream, inside 3 training steps run right after the timed region" % (wpl * cfg.num_hidden_layers),
                               "avg_launch_ms": round(ms, 4), "flops_per_launch": fl, "algorithmic_bytes_per_launch": by}
        if a.real and world == 1:
            rd = real_data_throughput(model, optim, labels, a.batch, a.n_best, epochs=a.epochs)
            syn_tok = a.batch * a.seq_len * a.steps / dt
            rd["synthetic_padded_tokens_per_s"] = round(syn_tok, 0)
            rd["real_over_synthetic_at_equal_padded_tokens"] = round(rd["padded_tokens_per_s"] / syn_tok, 3)
            res["real_data"] = rd
        if world == 1 and not a.no_cpu_baseline:
            note("cpu baseline (oracle on host cores) ...")
            res["cpu_baseline"] = cpu_baseline(labels)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
