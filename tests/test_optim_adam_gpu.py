"""GPU: --optim_choice adam | adamw (nbest_adam_*: one global-norm clip + torch Adam / HF AdamW over the arena) against
torch.optim.Adam + clip_grad_norm_ and a restatement of HF AdamW(correct_bias=False) driven by the real
transformers.get_linear_schedule_with_warmup; compute-copy refresh, determinism, the reference's loop body, the sharded
optimizer and --resume."""
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LR, BERT_LR = 1e-3, 1e-4


def _model(labels, dtype=torch.float32, fp8=False, dropout=0.0, seed=21, layers=2):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    cfg = ncfg.bert_base(num_hidden_layers=layers, vocab_size=3000, hidden_dropout_prob=0.1 if dropout else 0.0,
                         attention_probs_dropout_prob=0.1 if dropout else 0.0)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=dtype, dropout=dropout, seed=4, fp8_forward=fp8)
    m.load_reference_state(synth.model_state(cfg, labels, seed=seed))
    m.train()
    return m


def _batch(m, labels, seed=9, B=5, S=40):
    from nbest_amd import synth
    b = synth.nbest_batch(m.cfg, labels, B, S, n_best=5, seed=seed, ragged=True, trans_len=12)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


def _ulp(x):
    return (torch.nextafter(x, torch.full_like(x, math.inf)) - x).abs()


def _grads(a, seed, scale):
    """seeded gradient in every element of the arena - the pooler's included: the optimizer must ignore it there.  Magnitudes
    are kept >= scale / 2: Adam divides by sqrt(v) + eps, so an element whose gradient is near eps (or cancels against the L2
    term) amplifies a one-ulp difference of the clip coefficient beyond any per-element bar, in torch's own kernels as well"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(a.total, generator=gen, device="cuda")
    a.g.copy_(torch.sign(x) * (x.abs() + 0.5) * scale)


def _trainable(a):
    return [s for s in a.slots if "pooler" not in s.name]


def _check_step(a, ref, before, lr_of):
    """per-element parameter deltas of the HIP step against the reference's within 1e-5 lr + 2 ulp(p)"""
    for s in _trainable(a):
        lr = lr_of(s.name)
        d_hip = a.view(a.p, s.name) - before[s.name]
        d_ref = ref[s.name].detach() - before[s.name]
        tol = 1e-5 * lr + 2 * _ulp(before[s.name])
        bad = ((d_hip - d_ref).abs() > tol)
        assert not bad.any(), (s.name, (d_hip - d_ref).abs().max().item(), int(bad.sum()))


def _check_moments(a, m_ref, v_ref):
    for s in _trainable(a):
        for hip, ref in ((a.view(a.m, s.name), m_ref[s.name]), (a.view(a.v, s.name), v_ref[s.name])):
            scale = ref.abs().max().item()
            assert (hip - ref).abs().max().item() <= 1e-5 * max(scale, 1e-30), s.name


def test_adam_matches_torch_adam_with_global_clip(labels):
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=l2) after clip_grad_norm_(params, max_norm), three steps:
    clip active, inactive, active; one lr for every tensor; the pooler (no gradient) untouched and outside the norm"""
    from nbest_amd.optim import HipAdam
    m = _model(labels)
    a = m.arena
    max_norm, l2 = 5.0, 1e-4
    opt = HipAdam(m, kind="adam", lr=LR, bert_lr=BERT_LR, l2=l2, max_grad_norm=max_norm)
    assert opt.scheduler is None
    ref = {s.name: a.view(a.p, s.name).clone().requires_grad_(True) for s in _trainable(a)}
    topt = torch.optim.Adam(list(ref.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=l2)
    pool = {s.name: a.view(a.p, s.name).clone() for s in a.slots if "pooler" in s.name}
    n_el = sum(s.numel for s in _trainable(a))
    for k, (scale, clipped) in enumerate(((0.05, True), (0.1 * max_norm / math.sqrt(n_el), False), (1.0, True))):
        _grads(a, 100 + k, scale)
        before = {n: a.view(a.p, n).clone() for n in ref}
        with torch.no_grad():
            for n, t in ref.items():
                t.copy_(before[n])                      # both take the step from the same parameters
                t.grad = a.view(a.g, n).clone()
        total = torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm).item()
        assert (total > max_norm) == clipped, (k, total)
        topt.step()
        opt.step()
        torch.cuda.synchronize()
        _check_step(a, ref, before, lambda n: LR)
        _check_moments(a, {n: topt.state[t]["exp_avg"] for n, t in ref.items()}, {n: topt.state[t]["exp_avg_sq"] for n, t in ref.items()})
        assert abs(opt.clip[1].item() - total) <= 1e-5 * total
    assert opt.step_count == 3
    for n, p0 in pool.items():
        assert torch.equal(a.view(a.p, n), p0) and not a.view(a.m, n).any() and not a.view(a.v, n).any(), n


def _adamw_ref(p, g, m, v, lr, wd, eps=1e-6):
    """HF AdamW(correct_bias=False).step for one tensor (transformers <= 4.x optimization.py)"""
    m.mul_(0.9).add_(g, alpha=0.1)
    v.mul_(0.999).addcmul_(g, g, value=0.001)
    p.addcdiv_(m, v.sqrt().add_(eps), value=-lr)
    if wd > 0.0:
        p.add_(p, alpha=-lr * wd)


def test_adamw_matches_restated_rule_and_transformers_schedule(labels):
    """BertAdam's groups (bert_lr for the encoder, decay 0.01 except bias / LayerNorm), global clip, no bias correction, lr from
    the real get_linear_schedule_with_warmup: the first step has lr 0 (warm-up) and leaves every parameter bit-identical"""
    from transformers import get_linear_schedule_with_warmup
    from nbest_amd.arena import NO_DECAY
    from nbest_amd.optim import HipAdam
    m = _model(labels)
    a = m.arena
    T, warmup, max_norm = 10, 0.2, 5.0
    opt = HipAdam(m, kind="adamw", lr=LR, bert_lr=BERT_LR, warmup=warmup, t_total=T, max_grad_norm=max_norm)
    lr_g = lambda n: BERT_LR if "bert_encoder" in n else LR
    wd_g = lambda n: 0.0 if any(nd in n for nd in NO_DECAY) else 0.01
    ref = {s.name: a.view(a.p, s.name).clone().requires_grad_(True) for s in _trainable(a)}
    names = list(ref)
    dummy = torch.optim.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=lr_g(n)) for n in names], lr=1.0)
    sched = get_linear_schedule_with_warmup(dummy, num_warmup_steps=int(warmup * T), num_training_steps=T)
    mom = {n: torch.zeros_like(t) for n, t in ref.items()}
    vel = {n: torch.zeros_like(t) for n, t in ref.items()}
    p0 = a.p.clone()
    for k, scale in enumerate((1.0, 1e-4, 0.05, 1.0)):
        _grads(a, 200 + k, scale)
        before = {n: a.view(a.p, n).clone() for n in names}
        with torch.no_grad():
            for n, t in ref.items():
                t.copy_(before[n])
                t.grad = a.view(a.g, n).clone()
            torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm)
            for i, n in enumerate(names):
                _adamw_ref(ref[n], ref[n].grad, mom[n], vel[n], dummy.param_groups[i]["lr"], wd_g(n))
        opt.step()
        opt.scheduler.step()
        dummy.step()
        sched.step()
        torch.cuda.synchronize()
        if k == 0:
            assert torch.equal(a.p, p0), "lr 0 at the first (warm-up) step must leave every parameter as it was"
        _check_step(a, ref, before, lr_g)
        _check_moments(a, mom, vel)
    # the later steps moved every group: encoder / head learning rate x decay / no decay
    moved = {(lr_g(s.name), wd_g(s.name)) for s in _trainable(a) if not torch.equal(a.view(a.p, s.name), a.view(p0, s.name))}
    assert moved == {(LR, 0.0), (LR, 0.01), (BERT_LR, 0.0), (BERT_LR, 0.01)}, moved
    assert opt.step_count == 4 and opt.scheduler.last_epoch == 4


@pytest.mark.parametrize("mode", ["bf16", "fp8w"])
@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_compute_copies_are_refreshed(mode, kind, labels):
    """after a step: w16 == bf16(p) bit for bit, and the model computes exactly what a fresh model loaded from its updated
    state_dict computes - the packed, transposed and e4m3 weight images were all rebuilt from the new master"""
    from nbest_amd.optim import HipAdam
    fp8 = mode == "fp8w"
    m = _model(labels, torch.bfloat16, fp8=fp8)
    b = _batch(m, labels)

    def run(model):
        outs = []
        for _ in range(2):      # fp8w: the first pass after new weights is the calibration pass, the second the fp8 one
            outs.append(model.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                               add_l2_loss=True))
        return outs[-1]

    run(m)
    opt = HipAdam(m, kind=kind, lr=LR, bert_lr=BERT_LR, warmup=0.0, t_total=10, l2=1e-3)
    p0 = m.arena.p.clone()
    opt.step()
    torch.cuda.synchronize()
    a = m.arena
    assert not torch.equal(a.p, p0)
    assert torch.equal(a.w16, a.p.to(torch.bfloat16))
    m._drop_fp8_history()                           # both models start from the same (no) amax history
    fresh = _model(labels, torch.bfloat16, fp8=fp8)
    fresh.load_reference_state({k: v.detach().cpu() for k, v in m.state_dict().items()})
    fa = fresh.arena
    names = ("w8", "w8t", "w8_inv_scale", "w8p", "w8tp") if fp8 else ("w16", "w16t", "wpk", "wpkt")
    for n in names:
        x, y = getattr(a, n), getattr(fa, n)
        assert (x is None) == (y is None), n
        if x is not None:
            assert torch.equal(x, y), n
    o1, o2 = run(m), run(fresh)
    torch.cuda.synchronize()
    for k in ("top", "final", "loss_parts"):
        assert torch.equal(o1[k], o2[k]), k


def test_adamw_train_steps_are_deterministic(labels):
    """two runs of three fused train_steps (bf16, dropout on, adamw + schedule): the same p, m and v to the bit"""
    from nbest_amd.optim import HipAdam
    from nbest_amd.trainer import train_step

    def run():
        m = _model(labels, torch.bfloat16, dropout=0.3)
        opt = HipAdam(m, kind="adamw", lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=10)
        for i in range(3):
            train_step(m, opt, _batch(m, labels, seed=30 + i), add_l2_loss=True)
            opt.scheduler.step()
        torch.cuda.synchronize()
        return m.arena.p.clone(), m.arena.m.clone(), m.arena.v.clone()

    r1, r2 = run(), run()
    for x, y, n in zip(r1, r2, "pmv"):
        assert torch.equal(x, y), n


def test_reference_loop_body_matches_fused_path(labels):
    """n_best_asr_bert.py:264-277 verbatim on the autograd bridge - total_loss.backward(); clip_grad_norm_(params, max_norm);
    optimizer.step(); scheduler.step(); optimizer.zero_grad() - with the optimizer's own clip off (max_grad_norm=0), against the
    fused train_step with the clip inside.  Bars of test_model_gpu.py::test_autograd_bridge_runs_the_reference_loop_body: the two
    gradients agree to fp32 rounding; an element whose gradient is rounding noise may move by an order-dependent +-lr, so the
    parameters are compared by their mean difference"""
    from nbest_amd.optim import HipAdam
    from nbest_amd.trainer import train_step
    from oracle import stc
    b2t = stc.bottom2top_matrix(labels.top2bottom).cuda()
    max_norm, T = 1.0, 10
    mf, mb = _model(labels), _model(labels)
    of = HipAdam(mf, kind="adamw", lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=T, max_grad_norm=max_norm)
    ob = HipAdam(mb, kind="adamw", lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=T, max_grad_norm=0)
    opt = type("Opt", (), dict(optimizer=ob, scheduler=ob.scheduler, max_norm=max_norm))()
    p0 = mf.arena.p.clone()
    params = list(filter(lambda p: p.requires_grad, list(mb.parameters())))
    for i in range(3):
        b = _batch(mf, labels, seed=40 + i)
        mf.zero_grad()
        train_step(mf, of, b, add_l2_loss=True)
        of.scheduler.step()
        g_fused = mf.arena.g.clone()
        top, bottoms, final, asr_cls, trans_cls = mb(None, b["ids"], b["tids"], seg_ids=b["seg"], trans_seg_ids=b["tseg"],
                                                     classifier_input_type="asr")
        _, total_loss, _ = stc.total_loss(top, bottoms, final, b["labels"], labels.top2bottom, b2t, asr_cls, trans_cls, True)
        total_loss.backward()
        g_bridge = mb.arena.g.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, opt.max_norm).item()
        assert abs(of.clip[1].item() - norm) <= 1e-5 * norm, (of.clip[1].item(), norm)     # the fused step's global norm
        opt.optimizer.step()
        opt.scheduler.step()
        opt.optimizer.zero_grad()
        torch.cuda.synchronize()
        a = mf.arena
        for s in _trainable(a):
            if s.name.endswith("attention.self.key.bias"):      # its gradient is rounding noise (softmax is shift-invariant)
                continue
            x, y = a.view(g_bridge, s.name), a.view(g_fused, s.name)
            assert (x - y).abs().max().item() <= 2e-5 * max(y.abs().max().item(), 1e-20), s.name
        if i == 0:
            assert torch.equal(mf.arena.p, p0) and torch.equal(mb.arena.p, p0)    # lr 0 at the warm-up's first step
        dp = (mb.arena.p - mf.arena.p).abs()
        assert dp.mean().item() <= 1e-7, (i, dp.mean().item(), dp.max().item())
    assert not mb.arena.g.any()
    assert ob.step_count == of.step_count == 3 and ob.scheduler.last_epoch == of.scheduler.last_epoch == 3


def _cli_args(root, exp, extra, optim="adamw"):
    return ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
            "--bert_dropout", "0.1", "--optim_choice", optim, "--lr", "1e-3", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
            "--max_norm", "1.0", "--batchSize", "16", "--experiment", exp, "--add_segment_ids", "--n_best", "3",
            "--label_space", os.path.join(GOLDEN, "label_space.json"), "--vocab", os.path.join(GOLDEN, "text_vocab.json"),
            "--encoder_layers", "2", "--resume"] + (["--restated_adamw"] if optim == "adamw" else []) + extra


def test_sharded_adamw_equals_replicated(tmp_path):
    """two ranks on cuda:0 over gloo (NBEST_DP_REHEARSAL) with --optim_choice adamw: --shard_optimizer on gives the parameters and
    moments of the replicated optimizer bit for bit (the global clip's partials are SUM-all-reduced: x + 0 is exact)"""
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    env = dict(os.environ, NBEST_DP_REHEARSAL="1", OMP_NUM_THREADS="4")
    env.pop("RANK", None)
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    cks = []
    for port, shard in ((29721, "on"), (29722, "off")):
        args = _cli_args(root, str(tmp_path / shard), ["--max_epoch", "2", "--shard_optimizer", shard])
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "n_best_asr_bert.py")] + args
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
        cks.append(torch.load(os.path.join(cli.exp_dir(cli.parse_arguments(args)), "last.pt"), weights_only=True))
    on, off = cks
    assert on["optimizer"]["kind"] == "adamw" and on["optimizer"]["step"] == off["optimizer"]["step"] > 0
    assert on["optimizer"]["sched_step"] == off["optimizer"]["sched_step"] == on["optimizer"]["step"]
    for k in off["model"]:
        assert torch.equal(on["model"][k], off["model"][k]), k
    for k in off["optimizer"]["state"]:
        for f in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(on["optimizer"]["state"][k][f], off["optimizer"]["state"][k][f]), (k, f)


def test_cli_resume_adamw_and_refuse_another_kind(tmp_path):
    """--optim_choice adamw: stop after epoch 0 + --resume == two epochs in one go, to the bit (model, exp_avg, exp_avg_sq, step,
    schedule position); a last.pt written by BertAdam is refused with a message naming the kind"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    f32 = ["--dtype", "f32", "--max_epoch", "2"]
    assert cli.main(_cli_args(root, a, f32)) == 0
    assert cli.main(_cli_args(root, b, f32 + ["--stop_after_epoch", "0"])) == 0
    assert cli.main(_cli_args(root, b, f32)) == 0
    da, db = (cli.exp_dir(cli.parse_arguments(_cli_args(root, x, f32))) for x in (a, b))
    ca = torch.load(os.path.join(da, "last.pt"), weights_only=True)
    cb = torch.load(os.path.join(db, "last.pt"), weights_only=True)
    assert ca["epoch"] == cb["epoch"] == 1 and ca["optimizer"]["step"] == cb["optimizer"]["step"] == 4
    assert ca["optimizer"]["sched_step"] == cb["optimizer"]["sched_step"] == 4
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for k in ca["optimizer"]["state"]:
        for f in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(ca["optimizer"]["state"][k][f], cb["optimizer"]["state"][k][f]), (k, f)
    assert "Resumed after epoch 00 (optimizer step 2)" in open(os.path.join(db, "log.train")).read()
    # a BertAdam checkpoint in the adamw run's directory
    c = str(tmp_path / "c")
    one = ["--dtype", "f32", "--max_epoch", "1"]
    assert cli.main(_cli_args(root, c, one, optim="bertadam")) == 0
    dc_bert = cli.exp_dir(cli.parse_arguments(_cli_args(root, c, one, optim="bertadam")))
    dc_adamw = cli.exp_dir(cli.parse_arguments(_cli_args(root, c, one)))
    os.makedirs(dc_adamw, exist_ok=True)
    shutil.copy(os.path.join(dc_bert, "last.pt"), os.path.join(dc_adamw, "last.pt"))
    with pytest.raises(SystemExit, match="kind 'bertadam'"):
        cli.main(_cli_args(root, c, one))
