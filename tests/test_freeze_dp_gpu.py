"""GPU, two ranks on cuda:0 over gloo: a frozen set that changes mid-run under the SHARDED optimizer (the plan balances by
active elements, so its cut points move) gives the replicated optimizer's parameters and moments bit for bit."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import nbest_amd  # noqa: F401
        from nbest_amd import config as ncfg, synth
        from nbest_amd.model import NBestSTCModel
        from nbest_amd.optim import HipAdam, HipBertAdam
        from nbest_amd.trainer import GradReducer, broadcast_parameters, shard_bounds, train_step
        labels = ncfg.LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
        cfg = ncfg.bert_base(num_hidden_layers=4, vocab_size=3000, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
        B, S, STEPS = 6, 48, 4
        batches = []
        for s in range(STEPS):
            b = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=300 + s, ragged=True, trans_len=16)
            batches.append({k: torch.from_numpy(v).cuda() for k, v in b.items()})
        lo, hi = shard_bounds(B, rank, world)
        shard = lambda b: {k: v[lo:hi].contiguous() for k, v in b.items()}
        res = {}
        for kind in ("bertadam", "adamw"):
            for sharded in (False, True):
                m = NBestSTCModel(cfg, labels, device="cuda:0", compute_dtype=torch.bfloat16, dropout=0.3)
                m.load_reference_state(synth.model_state(cfg, labels, seed=11))
                m.train()
                for n, p in m.named_parameters():
                    if n.startswith(("bert_encoder.embeddings.", "bert_encoder.encoder.layer.0.", "bert_encoder.encoder.layer.1.")):
                        p.requires_grad_(False)
                if kind == "bertadam":
                    opt = HipBertAdam(m, lr=1e-3, bert_lr=1e-3, warmup=0.1, t_total=10, shard=sharded)
                else:
                    opt = HipAdam(m, kind="adamw", lr=1e-3, bert_lr=1e-3, warmup=0.1, t_total=10, max_grad_norm=1.0, shard=sharded)
                assert opt.sharded == sharded
                broadcast_parameters(m)
                red = GradReducer(m.arena, n_chunks=2, owner_ranges=opt.owner_ranges)
                cuts = []
                for k, b in enumerate(batches):
                    if k == 2:                                       # gradual unfreezing: layer 1 and the embeddings
                        for n, p in m.named_parameters():
                            if n.startswith(("bert_encoder.embeddings.", "bert_encoder.encoder.layer.1.")):
                                p.requires_grad_(True)
                    train_step(m, opt, shard(b), add_l2_loss=True, add_segment_ids=True, reducer=red, global_batch=B)
                    if sharded:
                        cuts.append([list(r) for r in opt.owner_ranges[rank]])
                opt.gather_master()
                torch.cuda.synchronize()
                a = m.arena
                res[(kind, sharded)] = (a.p.clone(), a.m.clone(), a.v.clone(), a.weights.clone(), cuts)
            (p0, m0, v0, w0, _), (p1, m1, v1, w1, cuts) = res[(kind, False)], res[(kind, True)]
            ok = torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(w0, w1)
            moved = cuts[1] != cuts[2]                               # the unfreezing moved this rank's range
            q.put((rank, kind, bool(ok), bool(moved), (p0 - p1).abs().max().item()))
        dist.destroy_process_group()
    except BaseException as e:                                       # noqa: BLE001 - reported to the parent
        q.put((rank, "error", repr(e), False, 0.0))
        raise


def test_sharded_optimizer_follows_a_changing_frozen_set():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29741
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    for _ in range(4):
        res.append(q.get(timeout=600))
        if res[-1][1] == "error":
            break
    for p in procs:
        p.join(120)
    assert all(r[1] != "error" for r in res), res
    assert sorted((r[0], r[1]) for r in res) == [(0, "adamw"), (0, "bertadam"), (1, "adamw"), (1, "bertadam")], res
    assert all(r[2] for r in res), res                               # sharded == replicated, bit for bit
    assert any(r[3] for r in res), res                               # and the shard plan did move
