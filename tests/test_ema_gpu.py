"""GPU: the device-side weight average of --ema_decay.  The two kernels (nbest_ema_update, nbest_ema_exchange) over a hand-built
descriptor table in a guard-filled buffer, the optimizers' recurrence against fp64, the ``ema_weights()`` swap with every derived
weight image, the optimizer state, two replicated data-parallel ranks, and the CLI end to end (model.pt holds the weights the
evaluation ran on)."""
import os
import re
import shutil
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT
from test_optim_adam_gpu import BERT_LR, LR, _batch, _grads, _model

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GUARD = 12345.678
NUMELS = (1, 3, 4, 255, 16383, 16384, 16385, 40000)
UNALIGNED = (255, 40000)          # offset % 4 != 0: the scalar path, as arena.py's unaligned bias / head slots (one of them multi-block)
INACTIVE = 16385                  # two blocks, both must return


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16)


def _table():
    """[(offset, numel, active)], device descriptor array, n_tensors, n_blocks, buffer length: at least 4 guard elements before,
    between and after the tensors"""
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    chunk = hb.lib().nbest_bertadam_chunk()
    assert chunk == 16384
    arr = (hb.TensorDesc * len(NUMELS))()
    off, blk, layout = 64, 0, []
    for i, n in enumerate(NUMELS):
        off = (off + 3) // 4 * 4 + 4
        if n in UNALIGNED:
            off += 1 + (i % 2)
        d = arr[i]
        d.offset, d.numel, d.lr, d.wd, d.active, d.block_start = off, n, 1.0, 0.0, int(n != INACTIVE), blk
        layout.append((off, n, int(n != INACTIVE)))
        blk += (n + chunk - 1) // chunk
        off += n
    total = off + 64
    assert {o % 4 for o, n, _ in layout if n in UNALIGNED} - {0} and all(o % 4 == 0 for o, n, _ in layout if n not in UNALIGNED)
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return layout, dev, len(NUMELS), blk, total


def _inputs(layout, total, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ema = torch.full((total,), GUARD, device="cuda")
    p = torch.full((total,), -GUARD, device="cuda")
    covered = torch.zeros(total, dtype=torch.bool, device="cuda")
    for off, n, _ in layout:
        ema[off:off + n] = torch.randn(n, generator=gen, device="cuda")
        p[off:off + n] = torch.randn(n, generator=gen, device="cuda") * 3.0
        p[off:off + n:7] = ema[off:off + n:7]                    # elements with ema == p
        covered[off:off + n] = True
    return ema, p, covered


@pytest.mark.parametrize("w", [0.0, 0.01, 1.0])
def test_ema_update_kernel(w):
    """ema = fma(w, p - ema, ema) on the active tensors against fp64, within 5 * 2^-24 * max(|ema|, |p|): one rounding each of
    p - ema, of the fma and of w.  The inactive tensor and every guard element keep their bits; so does everything at w = 0, and
    every element with ema == p; a second run from the same inputs gives the same bits."""
    from nbest_amd import hipabi as hb
    layout, descs, n_t, n_b, total = _table()
    ema0, p, covered = _inputs(layout, total)
    runs = []
    for _ in range(2):
        ema = ema0.clone()
        hb.check(hb.lib().nbest_ema_update(hb.ptr(ema), hb.ptr(p), hb.ptr(descs), n_t, n_b, w, hb.stream_ptr()), "ema_update")
        torch.cuda.synchronize()
        runs.append(ema)
    ema = runs[0]
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    assert torch.equal(_bits(p[~covered]), _bits(torch.full_like(p[~covered], -GUARD)))
    assert torch.equal(_bits(ema[~covered]), _bits(ema0[~covered])), "guard elements written"
    worst = 0.0
    for off, n, active in layout:
        got, e0, pp = ema[off:off + n], ema0[off:off + n], p[off:off + n]
        if not active:
            assert torch.equal(_bits(got), _bits(e0)), "inactive tensor written"
            continue
        want = e0.double() + w * (pp.double() - e0.double())
        bound = 5 * EPS * torch.maximum(e0.abs(), pp.abs()).double()
        err = (got.double() - want).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= bound).all(), (n, w, err.max().item())
        same = e0 == pp
        assert same.any() and torch.equal(_bits(got[same]), _bits(e0[same])), n
        if w == 0.0:
            assert torch.equal(_bits(got), _bits(e0)), n
        if w > 0 and n > 8:
            assert not torch.equal(got, e0), n
    print("ema_update w=%g: worst error / bound %.3f" % (w, worst))


def test_ema_update_keeps_negative_zero():
    """the bit-identity promises hold for -0.0 too (fma(w, +0, -0) alone would give +0)"""
    from nbest_amd import hipabi as hb
    layout, descs, n_t, n_b, total = _table()
    ema0 = torch.full((total,), -0.0, device="cuda")
    for w, p in ((0.0, torch.ones(total, device="cuda")), (0.3, torch.full((total,), -0.0, device="cuda")),
                 (0.3, torch.zeros(total, device="cuda"))):
        ema = ema0.clone()
        hb.check(hb.lib().nbest_ema_update(hb.ptr(ema), hb.ptr(p), hb.ptr(descs), n_t, n_b, w, hb.stream_ptr()), "ema_update")
        torch.cuda.synchronize()
        assert torch.equal(_bits(ema), _bits(ema0)), w


@pytest.mark.parametrize("lowp", [True, False])
def test_ema_exchange_kernel(lowp):
    """p <-> ema for every tensor, the inactive one included; p_lowp = bf16(new p) on the covered elements; guards untouched in all
    three buffers; two calls restore every bit"""
    from nbest_amd import hipabi as hb
    layout, descs, n_t, n_b, total = _table()
    ema0, p0, covered = _inputs(layout, total)
    ema, p = ema0.clone(), p0.clone()
    low0 = torch.full((total,), 7.0, dtype=torch.bfloat16, device="cuda")
    low = low0.clone() if lowp else None
    call = lambda: hb.check(hb.lib().nbest_ema_exchange(hb.ptr(p), hb.ptr(ema), hb.ptr(low), hb.ptr(descs), n_t, n_b, hb.stream_ptr()),
                            "ema_exchange")
    call()
    torch.cuda.synchronize()
    assert torch.equal(_bits(p[covered]), _bits(ema0[covered])) and torch.equal(_bits(ema[covered]), _bits(p0[covered]))
    assert torch.equal(_bits(p[~covered]), _bits(p0[~covered])) and torch.equal(_bits(ema[~covered]), _bits(ema0[~covered]))
    for off, n, _ in layout:
        assert torch.equal(_bits(p[off:off + n]), _bits(ema0[off:off + n])), n
    if lowp:
        assert torch.equal(_bits(low[covered]), _bits(p.to(torch.bfloat16)[covered]))
        assert torch.equal(_bits(low[~covered]), _bits(low0[~covered]))
    call()
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(ema), _bits(ema0))
    if lowp:
        assert torch.equal(_bits(low[covered]), _bits(p0.to(torch.bfloat16)[covered]))


def _optimizer(m, kind, **kw):
    from nbest_amd.optim import HipAdam, HipBertAdam
    if kind == "bertadam":
        return HipBertAdam(m, lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=40, **kw)
    return HipAdam(m, kind=kind, lr=LR, bert_lr=BERT_LR, l2=1e-4, warmup=0.1, t_total=40, max_grad_norm=5.0, **kw)


FROZEN = "bert_encoder.encoder.layer.0."


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["bertadam", "adam", "adamw"])
def test_optimizer_ema_follows_the_recurrence(kind, dtype, labels):
    """four steps on synthetic gradients with ema_decay = 0.9: arena.ema against the fp64 recurrence over the parameters after every
    step, with ema_decay_at, within 4 x the per-step bound of the kernel test; p, m, v and w16 bit-equal to a twin without EMA; a
    tensor frozen from the start has ema bit-equal to p"""
    from nbest_amd.optim import ema_decay_at
    models = []
    for ema_decay in (0.9, None):
        m = _model(labels, dtype)
        for n, p in m.named_parameters():
            if n.startswith(FROZEN):
                p.requires_grad_(False)
        models.append((m, _optimizer(m, kind, ema_decay=ema_decay)))
    (m, opt), (tm, topt) = models
    a, ta = m.arena, tm.arena
    assert ta.ema is None and a.ema is not None and a.ema.dtype == torch.float32 and torch.equal(a.ema, a.p)
    assert a.ema.data_ptr() != a.p.data_ptr()
    ref = a.p.double()
    scale = torch.maximum(a.p.abs(), a.ema.abs())
    for k in range(4):
        for mm in (m, tm):
            _grads(mm.arena, 500 + k, 0.05)
        opt.step()
        topt.step()
        if getattr(opt, "scheduler", None) is not None:
            opt.scheduler.step()
            topt.scheduler.step()
        torch.cuda.synchronize()
        ref += (1.0 - ema_decay_at(k + 1, 0.9)) * (a.p.double() - ref)
        scale = torch.maximum(scale, a.p.abs())
    assert opt.step_count == 4
    for s in a.slots:
        got, want = a.view(a.ema, s.name), a.view(ref, s.name)
        if s.name.startswith(FROZEN) or "pooler" in s.name:
            assert torch.equal(_bits(got.contiguous()), _bits(a.view(a.p, s.name).contiguous())), s.name
            continue
        bound = 4 * 5 * EPS * a.view(scale, s.name).double()
        assert ((got.double() - want).abs() <= bound).all(), (s.name, (got.double() - want).abs().max().item())
        assert not torch.equal(got, a.view(a.p, s.name)), s.name
    for name in ("p", "m", "v", "w16"):
        x, y = getattr(a, name), getattr(ta, name)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), name


def _fwd(m, b):
    """the evaluation pass of trainer.eval_epoch"""
    m.eval()
    out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)
    torch.cuda.synchronize()
    m.train()
    return {k: out[k].clone() for k in ("top", "final", "loss_parts")}


def _train(m, opt, b):
    from nbest_amd.trainer import train_step
    out = train_step(m, opt, b, add_l2_loss=True)
    torch.cuda.synchronize()
    return out["loss_parts"].clone()


IMAGES = ("p", "w16", "w16t", "wpk", "wpkt")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ema_weights_swaps_in_the_average_and_back(dtype, labels):
    """inside ``ema_weights()`` the model scores exactly as a second model loaded from the state_dict() taken inside; after the exit
    every weight image is back to the bit and the next training step equals that of a twin that never entered"""
    m, twin = _model(labels, dtype), _model(labels, dtype)
    opt, topt = _optimizer(m, "bertadam", ema_decay=0.9), _optimizer(twin, "bertadam", ema_decay=0.9)
    batches = [_batch(m, labels, seed=60 + i) for i in range(3)]
    for b in batches[:2]:
        _train(m, opt, b)
        _train(twin, topt, b)
    a = m.arena
    before = {n: getattr(a, n).clone() for n in IMAGES if getattr(a, n) is not None}
    assert ("w16t" in before) == (dtype == torch.bfloat16)
    ema0 = a.ema.clone()
    assert not torch.equal(ema0, a.p)
    raw = _fwd(m, batches[2])
    with opt.ema_weights() as got:
        assert got is opt
        assert torch.equal(a.p, ema0) and torch.equal(a.ema, before["p"])
        inside = _fwd(m, batches[2])
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        with pytest.raises(RuntimeError, match="nest"):
            with opt.ema_weights():
                pass
        for step in (opt.step, opt.step_main, opt.step_embeddings):
            with pytest.raises(RuntimeError, match="ema_weights"):
                step()
        assert torch.equal(a.p, ema0), "a refused call moved the weights"
    fresh = _model(labels, dtype)
    fresh.load_reference_state(sd)
    want = _fwd(fresh, batches[2])
    for k in want:
        assert torch.equal(inside[k], want[k]), k
    assert not torch.equal(inside["top"], raw["top"])
    for n, x in before.items():
        assert torch.equal(_bits(getattr(a, n)), _bits(x)), n
    assert torch.equal(a.ema, ema0) and opt.step_count == 2
    again = _fwd(m, batches[2])
    for k in raw:
        assert torch.equal(again[k], raw[k]), k
    l1, l2 = _train(m, opt, batches[2]), _train(twin, topt, batches[2])
    assert torch.equal(l1, l2)
    for n in ("p", "m", "ema"):
        assert torch.equal(getattr(a, n), getattr(twin.arena, n)), n
    # an exception inside still restores the raw weights
    p_now = a.p.clone()
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("x")
    assert torch.equal(a.p, p_now)
    with opt.ema_weights():
        pass


def test_ema_weights_round_trip_of_the_fp8_images(labels):
    """fp8w: the e4m3 copies, their transposes, packed forms and per-matrix scales are requantised from the averaged weights on
    entry and are back to the bit after the exit"""
    m = _model(labels, torch.bfloat16, fp8=True)
    opt = _optimizer(m, "bertadam", ema_decay=0.5)
    for i in range(3):                                  # the first pass is the calibration pass
        _train(m, opt, _batch(m, labels, seed=70 + i))
    a = m.arena
    names = [n for n in ("p", "w16", "w8", "w8t", "w8_inv_scale", "w8p", "w8tp") if getattr(a, n) is not None]
    assert {"w8", "w8t", "w8_inv_scale"} <= set(names)
    before = {n: getattr(a, n).clone() for n in names}
    with opt.ema_weights():
        torch.cuda.synchronize()
        assert not torch.equal(a.w8, before["w8"]) and not torch.equal(a.w16, before["w16"])
    torch.cuda.synchronize()
    for n, x in before.items():
        y = getattr(a, n)
        assert torch.equal(y.view(torch.uint8), x.view(torch.uint8)), n


@pytest.mark.parametrize("kind", ["bertadam", "adamw"])
def test_ema_state_round_trip_and_mismatch(kind, labels):
    m = _model(labels)
    opt = _optimizer(m, kind, ema_decay=0.9)
    for k in range(2):
        _grads(m.arena, 600 + k, 0.05)
        opt.step()
    torch.cuda.synchronize()
    sd = opt.state_dict()
    assert sd["ema_decay"] == 0.9 and set(sd["ema"]) == {s.name for s in m.arena.slots}
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd["ema"].values())
    m2 = _model(labels, seed=22)
    opt2 = _optimizer(m2, kind, ema_decay=0.9)
    assert not torch.equal(m2.arena.ema, m.arena.ema)
    opt2.load_state_dict(sd)
    for s in m.arena.slots:
        assert torch.equal(_bits(m2.arena.view(m2.arena.ema, s.name).contiguous()), _bits(m.arena.view(m.arena.ema, s.name).contiguous())), s.name
    assert opt2.step_count == 2
    # reset_ema: the average starts over from the weights loaded after construction
    m2.load_reference_state({k: v.detach().cpu() for k, v in m.state_dict().items()})
    opt2.reset_ema()
    assert torch.equal(m2.arena.ema, m2.arena.p) and m2.arena.ema.data_ptr() != m2.arena.p.data_ptr()
    # exactly one side with an average: refused, in the words of the kind mismatch
    plain = _optimizer(_model(labels), kind)
    assert "ema" not in plain.state_dict() and "ema_decay" not in plain.state_dict()
    with pytest.raises(ValueError, match=r"optimizer state with a weight average cannot be loaded into .* \(--ema_decay must match the run"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match=r"optimizer state without a weight average cannot be loaded into .* \(--ema_decay must match"):
        opt2.load_state_dict(plain.state_dict())
    with pytest.raises(RuntimeError):
        plain.reset_ema()
    with pytest.raises(RuntimeError):
        with plain.ema_weights():
            pass


@pytest.mark.parametrize("kind", ["bertadam", "adam"])
def test_sharded_optimizer_refuses_ema(kind, labels):
    m = _model(labels)
    with pytest.raises(ValueError, match="shard"):
        _optimizer(m, kind, shard=True, ema_decay=0.9)
    assert m.arena.ema is None


# ---- replicated data parallel: two ranks on cuda:0 over gloo, the rehearsal set-up of test_dp_gpu.py ---------------------------------
def _dp_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import nbest_amd  # noqa: F401
        from nbest_amd import config as ncfg, synth
        from nbest_amd.model import NBestSTCModel
        from nbest_amd.optim import HipBertAdam
        from nbest_amd.trainer import GradReducer, broadcast_parameters, shard_bounds, train_step
        labels = ncfg.LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
        cfg = ncfg.bert_base(num_hidden_layers=2, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        B, S, STEPS = 5, 48, 3

        def build(seed):
            m = NBestSTCModel(cfg, labels, device="cuda:0", compute_dtype=torch.float32, dropout=0.0)
            m.load_reference_state(synth.model_state(cfg, labels, seed=seed))
            m.train()
            return m

        batches = []
        for s in range(STEPS):
            b = synth.nbest_batch(cfg, labels, B, S, n_best=5, seed=100 + s, ragged=True, trans_len=16)
            batches.append({k: torch.from_numpy(v).cuda() for k, v in b.items()})
        lo, hi = shard_bounds(B, rank, world)
        m = build(5 + rank)
        broadcast_parameters(m)                         # rank 0's parameters win: the optimizer (and its average) is built afterwards
        opt = HipBertAdam(m, lr=1e-3, bert_lr=1e-3, warmup=0.1, t_total=10, ema_decay=0.9)
        red = GradReducer(m.arena, n_chunks=2)
        for b in batches:
            train_step(m, opt, {k: v[lo:hi].contiguous() for k, v in b.items()}, add_l2_loss=True, add_segment_ids=True, reducer=red,
                       global_batch=B)
        torch.cuda.synchronize()
        mine = m.arena.ema.cpu()
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        ms = build(5)
        opts = HipBertAdam(ms, lr=1e-3, bert_lr=1e-3, warmup=0.1, t_total=10, ema_decay=0.9)
        for b in batches:
            train_step(ms, opts, b, add_l2_loss=True, add_segment_ids=True)
        torch.cuda.synchronize()
        d = (m.arena.ema - ms.arena.ema).abs()
        dist.destroy_process_group()
        q.put((rank, dict(same=all(torch.equal(every[0], x) for x in every), mean_err=d.mean().item(), max_err=d.max().item(),
                          moved=not torch.equal(m.arena.ema, m.arena.p), p_err=(m.arena.p - ms.arena.p).abs().mean().item())))
    except BaseException as e:                      # surface the failure in the parent instead of a queue timeout
        import traceback
        q.put((rank, dict(error=traceback.format_exc() + repr(e))))


def test_replicated_ranks_hold_the_same_average():
    """after three data-parallel steps the two ranks' arena.ema are bit-identical and equal the single-process run's to the bar
    test_dp_gpu.py sets for the parameters (mean |DP - single| <= 2e-6: the gradient's summation order differs)"""
    import test_dp_gpu  # noqa: F401  (the rehearsal it describes: N spawned processes on cuda:0 over gloo)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, 29751, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(120)
    for r in range(2):
        assert "error" not in res[r], res[r]["error"]
        assert res[r]["same"], "replicas' averages diverged"
        assert res[r]["moved"]
        assert res[r]["mean_err"] <= 2e-6, res[r]


# ---- CLI end to end --------------------------------------------------------------------------------------------------------------
def test_cli_model_pt_holds_the_weights_the_evaluation_ran_on(tmp_path):
    """two epochs with --ema_decay 0.5 --resume, then --testing without the flag on the model.pt of that run: the Valid F1 / Acc of
    log.test are those of the last NEW BEST line of log.train.  last.pt carries the average in the optimizer state and the raw
    weights under ``model``"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--optim_choice", "bertadam", "--lr", "1e-3", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
              "--batchSize", "16", "--max_epoch", "2", "--experiment", str(tmp_path / "exp"), "--pre_trained_model", "bert",
              "--add_segment_ids", "--add_l2_loss", "--label_space", os.path.join(GOLDEN, "label_space.json"),
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "5", "--resume"]
    train_args = common + ["--ema_decay", "0.5"]
    assert cli.main(train_args) == 0
    d = cli.exp_dir(cli.parse_arguments(train_args))
    assert d.endswith("__ema_0.5")
    log = open(os.path.join(d, "log.train")).read().split("\n")
    assert log[0].startswith("Training starts") and log[1].startswith("Weight EMA: decay 0.5")
    best = [l for l in log if l.startswith("NEW BEST:")]
    assert best, "no epoch reached a valid F1 above 0: the comparison below would be empty"
    f1, acc = re.search(r"valid F1/Acc: ([0-9.]+)/([0-9.]+)", best[-1]).groups()
    ck = torch.load(os.path.join(d, "last.pt"), weights_only=True)
    saved = torch.load(os.path.join(d, "model.pt"), weights_only=True)
    assert ck["optimizer"]["ema_decay"] == 0.5 and set(ck["optimizer"]["ema"]) == set(ck["model"])
    assert any(not torch.equal(ck["model"][k], saved[k]) for k in saved), "last.pt holds the averaged weights under `model`"
    if best[-1].startswith("NEW BEST:\tEpoch: 01"):                    # model.pt written after the last epoch: it IS the average
        w = "bert_encoder.encoder.layer.1.output.dense.weight"
        assert torch.equal(saved[w], ck["optimizer"]["ema"][w])
    # --testing is refused with the flag, and without it the directory name has no ema_ part: evaluate a copy of model.pt there
    d_test = cli.exp_dir(cli.parse_arguments(common))
    os.makedirs(d_test)
    shutil.copy(os.path.join(d, "model.pt"), os.path.join(d_test, "model.pt"))
    assert cli.main(common + ["--testing"]) == 0
    line = [l for l in open(os.path.join(d_test, "log.test")).read().split("\n") if l.startswith("[Valid]")][0]
    tf1, tacc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", line).groups()
    assert (tf1, tacc) == (f1, acc), (line, best[-1])
