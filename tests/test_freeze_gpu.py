"""GPU: training with frozen parameters (requires_grad False): frozen tensors keep their values and have no gradient,
trainable tensors get the gradients of the unfrozen model bit for bit, the optimizers skip frozen tensors and start a tensor
that becomes trainable from zero moments, the frozen layers' activations are not stashed, the fp8w mode, and the CLI flags."""
import os
import re
import shutil

import pytest
import torch

from conftest import GOLDEN
from test_infer_gpu import _batch, _model

pytestmark = pytest.mark.gpu

EMB = "bert_encoder.embeddings."
LAY = "bert_encoder.encoder.layer.%d."


def _freeze(m, emb=False, layers=(), names=()):
    pre = ([EMB] if emb else []) + [LAY % l for l in layers]
    for n, p in m.named_parameters():
        if (pre and n.startswith(tuple(pre))) or n in names:
            p.requires_grad_(False)
    return {n for n, p in m.named_parameters() if not p.requires_grad and "pooler" not in n}


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _step(m, b):
    return m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                              add_l2_loss=True)


# ---- 1. the reference loop body on the autograd bridge ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_loop_leaves_frozen_tensors_alone(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, L=4, dtype=dtype)
    m.train()
    frozen = _freeze(m, emb=True, layers=(0, 1))
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    b = _batch(cfg, labels, 4, 48)
    before = _params(m)
    for _ in range(2):
        m.zero_grad()
        top, bottoms, fin, asr_cls, _ = m(None, b["ids"], seg_ids=b["seg"])
        (fin.sum() + 0.5 * top.sum() + 0.1 * asr_cls.sum()).backward()
        opt.step()
    torch.cuda.synchronize()
    after = dict(m.named_parameters())
    for n in frozen:
        assert torch.equal(after[n].detach(), before[n]), "frozen %s changed" % n
        assert after[n].grad is None, n
    moved = [n for n in after if n not in frozen and "pooler" not in n and not torch.equal(after[n].detach(), before[n])]
    assert any(n.startswith(LAY % 3) for n in moved) and any(n.startswith("clf.") for n in moved)


# ---- 2. trainable gradients are the unfrozen model's, bit for bit ----------------------------------------------------------------
QKV2 = tuple(LAY % 2 + "attention.self.%s.weight" % q for q in ("query", "key", "value"))
WO1 = (LAY % 1 + "attention.output.dense.weight",)
# (the last two freeze one half of the QKV + attention-out weight-gradient pair: the other half runs as a single launch)
CASES = {"emb+0..1": (True, (0, 1)), "emb": (True, ()), "layer2": (False, (2,)), "all_layers": (True, (0, 1, 2, 3)),
         "qkv_w_l2": (False, (), QKV2), "attn_out_w_l1": (False, (), WO1)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trainable_gradients_bit_identical(case, dtype, labels):
    b = None
    grads = []
    for freeze in (False, True):
        m, cfg, _ = _model(labels, L=4, dtype=dtype)
        m.train()
        b = b or _batch(cfg, labels, 4, 48)
        frozen = _freeze(m, *CASES[case]) if freeze else set()
        before = _params(m)
        _step(m, b)
        torch.cuda.synchronize()
        grads.append({n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()})
        for n in frozen:
            assert grads[-1][n] is None, n
            assert torch.equal(dict(m.named_parameters())[n].detach(), before[n])
    full, part = grads
    checked = 0
    for n, g in part.items():
        if g is not None and "pooler" not in n:
            assert torch.equal(g, full[n]), "gradient of %s differs from the unfrozen model's" % n
            checked += 1
    assert checked > 0


# ---- 3. optimizers ---------------------------------------------------------------------------------------------------------------
def test_bertadam_step_equals_unfrozen_run_on_trainable(labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for freeze in (False, True):
        m, cfg, _ = _model(labels, L=4, dtype=torch.bfloat16)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        frozen = _freeze(m, emb=True, layers=(0,)) if freeze else set()
        before = _params(m)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        _step(m, b)
        opt.step()
        torch.cuda.synchronize()
        res.append((_params(m), frozen, before))
    (full, _, _), (part, frozen, before) = res
    for n in part:
        if n in frozen:
            assert torch.equal(part[n], before[n]), n
        else:
            assert torch.equal(part[n], full[n]), "%s differs from the unfrozen run" % n


def test_adam_clips_over_trainable_tensors_only(labels):
    """torch.optim.Adam + clip_grad_norm_ over the trainable parameters (n_best_asr_bert.py:269 filters on requires_grad), with
    the bar of test_optim_adam_gpu: seeded gradients in EVERY arena element, the frozen ones included - the optimizer must leave
    them out of the norm and the update"""
    from nbest_amd.optim import HipAdam
    from test_optim_adam_gpu import _grads, _ulp
    LR, l2, max_norm = 1e-3, 1e-4, 0.5
    m, cfg, _ = _model(labels, L=4, dtype=torch.float32)
    m.train()
    b = _batch(cfg, labels, 4, 48)
    frozen = _freeze(m, emb=True, layers=(0, 1))
    opt = HipAdam(m, kind="adam", lr=LR, l2=l2, max_grad_norm=max_norm)
    a = m.arena
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters() if p.requires_grad and "pooler" not in n}
    topt = torch.optim.Adam(list(ref.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=l2)
    for k in range(2):
        _step(m, b)                                      # sets .grad (None for the frozen tensors)
        _grads(a, 200 + k, 0.05)
        before = _params(m)
        with torch.no_grad():
            for n, t in ref.items():
                t.copy_(before[n])
                t.grad = a.view(a.g, n).clone()
        total = torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm).item()
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert total > max_norm and abs(opt.clip[1].item() - total) <= 1e-5 * total, (opt.clip[1].item(), total)
        now = dict(m.named_parameters())
        for n in frozen:
            assert torch.equal(now[n].detach(), before[n]) and not a.view(a.m, n).any(), n
        for n, r in ref.items():
            d_hip, d_ref = now[n].detach() - before[n], r.detach() - before[n]
            assert not ((d_hip - d_ref).abs() > 1e-5 * LR + 2 * _ulp(before[n])).any(), n


# ---- 4. unfreezing mid-run -------------------------------------------------------------------------------------------------------
def test_unfrozen_tensor_starts_from_zero_moments(labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, L=4, dtype=torch.float32)
    m.train()
    b = _batch(cfg, labels, 4, 48)
    _freeze(m, emb=True, layers=(0,))
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=-1, t_total=-1)
    for _ in range(2):
        _step(m, b)
        opt.step()
    name = LAY % 0 + "output.dense.weight"
    p = m.get_parameter(name)
    p.requires_grad_(True)                                   # gradual unfreezing: one matrix of layer 0
    _step(m, b)
    assert p.grad is not None and p.grad.data_ptr() == m.arena.view(m.arena.g, name).data_ptr()
    g, w = p.grad.clone(), p.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    # BertAdam's first step from m = v = 0: clip to norm 1, m = 0.1 g, v = 0.001 g^2, p -= lr (m / (sqrt v + e) + 0.01 p)
    g = g * min(1.0, 1.0 / (g.norm().item() + 1e-6))
    mm, vv = 0.1 * g, 0.001 * g * g
    want = w - 3e-5 * (mm / (vv.sqrt() + 1e-6) + 0.01 * w)
    assert torch.allclose(p.detach(), want, rtol=0, atol=1e-7 + 1e-6 * 3e-5)
    assert torch.allclose(m.arena.view(m.arena.m, name), mm, rtol=1e-5, atol=0)


# ---- 5. memory -------------------------------------------------------------------------------------------------------------------
def test_frozen_layers_are_not_stashed(labels):
    import ctypes as C
    from nbest_amd import hipabi as hb
    from nbest_amd.optim import HipBertAdam
    peaks = []
    for K in (0, 2):
        torch.cuda.empty_cache()
        m, cfg, _ = _model(labels, L=4, dtype=torch.bfloat16)
        m.train()
        b = _batch(cfg, labels, 32, 128)
        _freeze(m, emb=K > 0, layers=range(K))
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
        opt.step()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        (ps,) = m._passes.values()
        d = ps.desc
        assert d.first_trainable == K
        assert m._stash[0].numel() == hb.lib().nbest_encoder_act_bytes(C.byref(d))
        del m, opt
    assert peaks[1] < peaks[0], peaks


# ---- 6. fp8w ---------------------------------------------------------------------------------------------------------------------
def test_fp8w_freezing_keeps_frozen_copies(labels):
    from nbest_amd.optim import HipBertAdam
    grads = []
    for freeze in (False, True):
        m, cfg, _ = _model(labels, L=4, dtype=torch.bfloat16, fp8=True)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        frozen = _freeze(m, emb=True, layers=(0, 1)) if freeze else set()
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        a = m.arena
        w8, sc = a.w8.clone(), a.w8_inv_scale.clone()
        _step(m, b)                                          # calibration pass (bf16 GEMMs): the unfrozen model's gradients
        grads.append({n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()})
        for _ in range(3):
            opt.step()
            _step(m, b)
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(a.p).all()
        if freeze:
            for n in frozen:
                if n.startswith(LAY % 0) or n.startswith(LAY % 1):
                    s = a.by_name[n]
                    assert torch.equal(a.w8[s.offset:s.offset + s.numel], w8[s.offset:s.offset + s.numel]), n
            assert torch.equal(a.w8_inv_scale[:8], sc[:8])   # the QKV / attention-out / FFN matrices of layers 0 and 1
    for n, g in grads[1].items():
        if g is not None and "pooler" not in n:
            assert torch.equal(g, grads[0][n]), n


@pytest.mark.parametrize("case", ["emb+0..1", "qkv_w_l2", "attn_out_w_l1"])
def test_fp8w_backward_gradients_bit_identical(case, labels):
    """the second pass of an fp8w model runs the fp8 forward and the fp8 dgrads / weight gradients (the first one calibrated):
    with the weights unchanged in between, the trainable gradients equal the unfrozen model's bit for bit"""
    grads = []
    for freeze in (False, True):
        m, cfg, _ = _model(labels, L=4, dtype=torch.bfloat16, fp8=True)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        if freeze:
            _freeze(m, *CASES[case])
        _step(m, b)                                          # calibration pass
        assert m._gamax_valid and m._aamax_valid
        _step(m, b)                                          # fp8 pass
        torch.cuda.synchronize()
        assert m._gamax_valid
        grads.append({n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()})
    checked = 0
    for n, g in grads[1].items():
        if g is not None and "pooler" not in n:
            assert torch.equal(g, grads[0][n]), n
            checked += 1
    assert checked > 0


# ---- 7. CLI --------------------------------------------------------------------------------------------------------------------
def _cli_args(root, exp, extra):
    return ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
            "--bert_dropout", "0.1", "--lr", "3e-5", "--bert_lr", "3e-5", "--batchSize", "16", "--max_epoch", "2", "--experiment", exp,
            "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", "f32",
            "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "3", "--n_best", "3", "--resume",
            "--freeze_embeddings", "--freeze_layers", "2"] + extra


def test_cli_freeze_flags_train_and_resume(tmp_path, capsys):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    a_exp, b_exp = str(tmp_path / "a"), str(tmp_path / "b")
    assert cli.main(_cli_args(root, a_exp, ["--stop_after_epoch", "0"])) == 0
    out = capsys.readouterr().out
    da = cli.exp_dir(cli.parse_arguments(_cli_args(root, a_exp, [])))
    assert da.endswith("__fz_emb_2")
    e0 = torch.load(os.path.join(da, "last.pt"), weights_only=True)["model"]
    frozen = [n for n in e0 if n.startswith((EMB, LAY % 0, LAY % 1))]
    assert frozen and len(frozen) < len(e0)
    n_params = int(re.search(r"num params: (\d+)", out).group(1))
    assert n_params == sum(v.numel() for n, v in e0.items() if n not in frozen)
    assert cli.main(_cli_args(root, a_exp, [])) == 0                  # resume: epoch 1
    a1 = torch.load(os.path.join(da, "last.pt"), weights_only=True)
    assert cli.main(_cli_args(root, b_exp, [])) == 0                  # both epochs in one run
    db = cli.exp_dir(cli.parse_arguments(_cli_args(root, b_exp, [])))
    b1 = torch.load(os.path.join(db, "last.pt"), weights_only=True)
    for n, v in a1["model"].items():
        assert torch.equal(v, b1["model"][n]), "resumed run differs from the uninterrupted one: %s" % n
        if n in frozen:
            assert torch.equal(v, e0[n]), "frozen %s changed" % n
    assert any(not torch.equal(a1["model"][n], e0[n]) for n in a1["model"] if n.startswith(LAY % 2))
    if os.path.exists(os.path.join(da, "model.pt")):
        best = torch.load(os.path.join(da, "model.pt"), weights_only=True)
        for n in frozen:
            assert torch.equal(best[n], e0[n]), n
