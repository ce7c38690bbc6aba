"""GPU: the in-batch contrastive term.  nbest_cls_contrast against the fp64 restatement of tests/test_contrast_cpu.py on the
unsaturated draw (loss, hits, both gradients, strided rows, pre-filled / overwritten / accumulated gradient buffers), its identities and
refusals, forward_backward(contrast=) on a whole fp32 model against the oracle under torch autograd, the untouched path without it,
the combinations with R-Drop and distillation, train_step(contrast_weight=) and --contrastive_weight through the CLI."""
import os
import re
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_contrast_cpu import BAR_GRAD, BAR_LOSS, contrast_reference, unsaturated_draw

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERR_ARG, ERR_WORKSPACE = -1, -6
W = 1.3


def _rows(x, stride_rows, dtype):
    """``x`` [B, H] as row 0 of every group of ``stride_rows`` rows of a [B * stride_rows, H] tensor (the other rows NaN)"""
    B, H = x.shape
    buf = torch.full((B, stride_rows, H), float("nan"), dtype=dtype, device=DEV)
    buf[:, 0, :] = x.to(DEV).to(dtype)
    return buf.reshape(B * stride_rows, H)


def _call(a, t, key, weight, T, dtype=torch.float32, da=None, dt=None, accumulate_dt=False, ws=None):
    """hidden_a at row stride 3 H, hidden_t at row stride 2 H"""
    from nbest_amd import hipabi as hb
    B, H = a.shape
    out = hb.cls_contrast(_rows(a, 3, dtype), 3 * H, _rows(t, 2, dtype), 2 * H, B, H, weight, T,
                          keys=None if key is None else key.to(DEV), da=da, dt=dt, accumulate_dt=accumulate_dt, ws=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("keyed", [False, True], ids=["nokey", "keys"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [0.05, 0.1])
@pytest.mark.parametrize("B,H", [(1, 768), (2, 64), (3, 768), (5, 768), (64, 768), (65, 1024), (257, 768)])
def test_kernel_matches_the_fp64_restatement(B, H, T, dtype, keyed):
    """out[0..3], da (pre-filled: the result is pre-fill + reference) and dt (overwrite and accumulate mode) against the restatement in
    fp64 on the same bf16-representable rows, at the project's bars for these quantities: L 1e-5 relative, hits equal, a gradient
    within 1e-4 of the tensor's largest reference element"""
    a, t, key = unsaturated_draw(B, H, T)
    key = key if keyed else None
    ref = contrast_reference(a.double(), t.double(), key, W, T)
    g = torch.Generator().manual_seed(B + H)
    fill_a, fill_t = (0.01 * torch.randn(B, H, generator=g)).to(DEV), (0.01 * torch.randn(B, H, generator=g)).to(DEV)
    da, dt_over, dt_acc = fill_a.clone(), torch.full((B, H), float("nan"), device=DEV), fill_t.clone()
    out = _call(a, t, key, W, T, dtype, da=da, dt=dt_over)
    out2 = _call(a, t, key, W, T, dtype, da=None, dt=dt_acc, accumulate_dt=True)
    worst = {}
    o = out.double().cpu()
    e_l = abs(o[0].item() - ref["L"].item()) / max(ref["L"].item(), 1e-30) if B > 1 else abs(o[0].item())
    worst["L"] = e_l / BAR_LOSS
    print("cls_contrast B=%d H=%d T=%g %s %s: L %.6f (ref %.6f), hits %d (ref %d)" % (
        B, H, T, str(dtype)[6:], "keys" if keyed else "nokey", o[0], ref["L"], o[1], ref["hits"]))
    assert e_l <= BAR_LOSS, (o[0].item(), ref["L"].item())
    assert o[1].item() == ref["hits"] and o[2].item() == B and o[3].item() == 0.0
    assert torch.equal(out, out2)
    if B == 1:
        assert torch.equal(da, fill_a) and not dt_over.any() and torch.equal(dt_acc, fill_t) and o[0].item() == 0.0
    else:
        scale_a, scale_t = ref["da"].abs().max().item(), ref["dt"].abs().max().item()
        for name, got, want, scale in (("da", da, fill_a.double().cpu() + ref["da"], scale_a), ("dt", dt_over, ref["dt"], scale_t),
                                       ("dt+", dt_acc, fill_t.double().cpu() + ref["dt"], scale_t)):
            err = (got.double().cpu() - want).abs().max().item() / scale
            worst[name] = err / BAR_GRAD
            assert err == err and err <= BAR_GRAD, (name, err)
    print("cls_contrast B=%d H=%d T=%g %s %s: worst error / bar %s" % (
        B, H, T, str(dtype)[6:], "keys" if keyed else "nokey", ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_kernel_identities():
    """all keys equal: out[0] == 0.0, da bit-unchanged, dt all zero.  weight 0: da bit-unchanged, dt zero, out[0] the bits of W 1.3.
    Two identical calls give identical bits, also when the workspace is NaN-filled before the second"""
    from nbest_amd import hipabi as hb
    B, H, T = 65, 768, 0.1
    a, t, key = unsaturated_draw(B, H, T)
    fill = torch.randn(B, H, device=DEV)
    da, dt = fill.clone(), torch.full((B, H), float("nan"), device=DEV)
    out = _call(a, t, torch.full((B,), 9, dtype=torch.int64), W, T, da=da, dt=dt)
    assert out[0].item() == 0.0 and out[1].item() == B and torch.equal(da, fill) and not dt.any()
    da, dt = fill.clone(), torch.full((B, H), float("nan"), device=DEV)
    out0 = _call(a, t, key, 0.0, T, da=da, dt=dt)
    assert torch.equal(da, fill) and not dt.any()
    ws = torch.zeros(hb.cls_contrast_ws_bytes(B, H), dtype=torch.uint8, device=DEV)
    runs = []
    for i in range(3):
        if i == 2:
            ws.view(torch.float32).fill_(float("nan"))
        da, dt = fill.clone(), torch.empty(B, H, device=DEV)
        runs.append((_call(a, t, key, W, T, torch.bfloat16, da=da, dt=dt, ws=ws), da, dt))
    assert runs[0][0][0].item() > 0 and torch.equal(out0.view(torch.int32), _call(a, t, key, W, T).view(torch.int32))
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(runs[0][1], fill)


def test_kernel_refusals_touch_nothing():
    """a workspace one byte short, B = 4097 and temperature 0: the error code, with out, da and dt as they were"""
    from nbest_amd import hipabi as hb
    import ctypes as C
    B, H = 5, 64
    L = hb.lib()
    hid = torch.randn(4097, H, device=DEV)
    out, da, dt = torch.full((4,), 7.0, device=DEV), torch.full((4097, H), 3.0, device=DEV), torch.full((4097, H), 5.0, device=DEV)
    ws = torch.zeros(hb.cls_contrast_ws_bytes(4097, H), dtype=torch.uint8, device=DEV)

    def call(B=B, T=0.1, ws_bytes=None):
        n = hb.cls_contrast_ws_bytes(B, H) if ws_bytes is None else ws_bytes
        return L.nbest_cls_contrast(hb.ptr(hid), H, hb.ptr(hid), H, C.c_void_p(0), 1.0, T, hb.ptr(out), hb.ptr(da), hb.ptr(dt), 0, B, H,
                                    hb.F32, hb.ptr(ws), n, hb.stream_ptr())
    assert call(ws_bytes=hb.cls_contrast_ws_bytes(B, H) - 1) == ERR_WORKSPACE
    assert call(B=4097) == ERR_ARG
    assert call(T=0.0) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (da == 3.0).all() and (dt == 5.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert out[2].item() == B and (da[B:] == 3.0).all() and (dt[B:] == 5.0).all() and not (da[:B] == 3.0).all()


def test_whole_model_fp32_matches_the_oracle_under_autograd(labels):
    """bert_L2, weight 1, temperature 0.1, dropout 0, transcript row 1 set equal to row 0 (a duplicate key): the arena gradients of
    forward_backward(contrast=) against the oracle model with hard + MSE + W * the restatement on its CLS rows under torch autograd,
    at the fp32 gradient bars of tests/test_model_gpu.py (noise-to-signal 2e-3 per tensor, the STC heads as one fused matrix, key bias
    skipped); contrast[0] 1e-4 relative; two runs give the same bits; loss_parts has the bits of the step without the argument"""
    from test_contrast_cpu import contrast_loss
    from test_model_gpu import _build, _oracle_for
    from conftest import case_inputs
    from nbest_amd.trainer import transcript_keys
    from oracle import stc
    meta, _ = load_case("bert_L2")
    weight, T = 1.0, 0.1
    cfg, sd, batch = case_inputs(meta, labels)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v).clone() for k, v in batch.items()}
    t["tids"][1], t["tseg"][1] = t["tids"][0], t["tseg"][0]
    keys = transcript_keys(t["tids"])
    assert keys[1].item() == 0 and keys.unique().numel() == keys.numel() - 1
    top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"] if meta["seg"] else None, trans_seg_ids=t["tseg"])
    _, _, parts = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, stc.bottom2top_matrix(labels.top2bottom),
                                 asr, tr, meta["add_l2"])
    con = contrast_loss(asr, tr, keys, T)
    ref_con = contrast_reference(asr.detach().double(), tr.detach().double(), keys, weight, T)
    total = parts["bottom_bce"] + parts["top_bce"] + parts["ce"] + weight * con
    if meta["add_l2"]:
        total = total + parts["mse"]
    total.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    m, b = _build(meta, labels, torch.float32)
    b["tids"][1], b["tseg"][1] = b["tids"][0], b["tseg"][0]
    step = lambda mm, **kw: mm.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                                                trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"], **kw)
    runs = []
    for _ in range(2):
        out = step(m, contrast=dict(weight=weight, temperature=T, keys=keys.to(DEV)))
        torch.cuda.synchronize()
        runs.append(m.arena.g.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "the contrast step is not bit-reproducible"
    c = out["contrast"].double().cpu()
    print("forward_backward(contrast=) bert_L2 fp32: contrast %.6f vs %.6f (autograd expression %.6f), hits %d vs %d of %d" % (
        c[0], ref_con["L"], con.item(), c[1], ref_con["hits"], c[2]))
    assert abs(c[0].item() - ref_con["L"].item()) <= 1e-4 * ref_con["L"].item() and c[2].item() == keys.numel() and c[3].item() == 0.0
    named = dict(m.named_parameters())
    fused = lambda n: n.startswith("clf.") and (n.endswith(".weight") or n.endswith(".bias"))
    worst = (0.0, "")
    for kind in (".weight", ".bias"):
        names = [n for n in ref_g if fused(n) and n.endswith(kind)]
        num = sum((named[n].grad.float().cpu() - ref_g[n]).pow(2).sum().item() for n in names) ** 0.5
        den = sum(ref_g[n].pow(2).sum().item() for n in names) ** 0.5
        worst = max(worst, (num / den, "clf fused " + kind))
        assert num <= 2e-3 * den, (kind, num / den)
    for n, g_ref in ref_g.items():
        if n.endswith("attention.self.key.bias") or fused(n):          # (softmax is invariant to a key bias: both sides are noise)
            continue
        ns = ((named[n].grad.float().cpu() - g_ref).norm() / g_ref.norm().clamp_min(1e-30)).item()
        worst = max(worst, (ns, n))
        assert ns <= 2e-3, (n, ns)
    print("forward_backward(contrast=) bert_L2 fp32: worst gradient noise-to-signal %.3e (%s), bar 2e-3" % worst)
    plain, _ = _build(meta, labels, torch.float32)
    pout = step(plain)
    torch.cuda.synchronize()
    assert "contrast" not in pout and not torch.equal(plain.arena.g, m.arena.g)
    assert torch.equal(pout["loss_parts"].view(torch.int32), out["loss_parts"].view(torch.int32))


def test_without_contrast_nothing_changes(labels):
    """a plain step after a contrast step has the bits of a model that never saw one (dropout on); add_l2_loss + contrast(weight 0)
    leaves the gradients of add_l2_loss alone; need_grad=False computes the loss only; refused arguments raise before anything runs"""
    from test_optim_adam_gpu import _batch, _model
    a, twin = _model(labels, torch.bfloat16, dropout=0.3), _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(a, labels, B=6)
    tr = dict(seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"])
    con = dict(weight=0.7, temperature=0.1)
    out = a.forward_backward(b["ids"], b["labels"], contrast=con, **tr)
    tout = twin.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    assert out["contrast"][0].item() > 0 and "contrast" not in tout and not torch.equal(a.arena.g, twin.arena.g)
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(out[k], tout[k]), k
    assert out["trans_cls"] is not None and tout["trans_cls"] is None
    o1, o2 = a.forward_backward(b["ids"], b["labels"], **tr), twin.forward_backward(b["ids"], b["labels"], **tr)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.g.view(torch.int32), twin.arena.g.view(torch.int32))
    assert a.step_counter == twin.step_counter == 2
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(o1[k], o2[k]), k
    assert "contrast" not in o1
    # weight 0 next to the MSE: the MSE's gradients, bit for bit
    o3 = a.forward_backward(b["ids"], b["labels"], add_l2_loss=True, contrast=dict(weight=0.0, temperature=0.1), **tr)
    o4 = twin.forward_backward(b["ids"], b["labels"], add_l2_loss=True, **tr)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.g, twin.arena.g) and torch.equal(o3["loss_parts"], o4["loss_parts"]) and o3["contrast"][0].item() > 0
    # the loss only
    g0 = a.arena.g.clone()
    a.eval()
    ev = a.forward_backward(b["ids"], b["labels"], need_grad=False, contrast=con, **tr)
    torch.cuda.synchronize()
    want = contrast_reference(ev["asr_cls"].double().cpu(), ev["trans_cls"].double().cpu(), None, 0.7, 0.1)
    assert abs(ev["contrast"][0].item() - want["L"].item()) <= 1e-5 * want["L"].item()
    assert torch.equal(a.arena.g, g0)
    a.train()
    steps = a.step_counter
    for kwargs in (dict(contrast=dict(weight=-1.0, temperature=0.1)), dict(contrast=dict(weight=float("nan"), temperature=0.1)),
                   dict(contrast=dict(weight=1.0, temperature=0.0)), dict(contrast=dict(weight=1.0, temperature=float("inf"))),
                   dict(contrast=con, trans_input_ids=None), dict(contrast=con, adv=dict(epsilon=1.0)),
                   dict(contrast=dict(con, keys=torch.arange(5, device=DEV)))):
        with pytest.raises(ValueError, match="contrast"):
            a.forward_backward(b["ids"], b["labels"], **dict(tr, **kwargs))
    L, heads = a.cfg.num_hidden_layers, a.cfg.num_attention_heads
    for trainable in (False, True):
        a.set_head_mask(torch.ones(L, heads), trainable=trainable)
        with pytest.raises(RuntimeError, match="contrast"):
            a.forward_backward(b["ids"], b["labels"], contrast=con, **tr)
    a.set_head_mask(None)
    assert a.step_counter == steps and torch.equal(a.arena.g, g0)
    f8 = _model(labels, torch.bfloat16, fp8=True)
    with pytest.raises(RuntimeError, match="contrast"):
        f8.forward_backward(b["ids"], b["labels"], contrast=con, **tr)
    assert f8.step_counter == 0


@pytest.mark.parametrize("other", ["rdrop", "distill"])
def test_combinations_one_step(other, labels):
    """the small bf16 model, one step with the contrastive term next to R-Drop (2 P rows, doubled keys) or distillation, with the
    MSE: contrast[0] is the restatement on the returned CLS rows, the soft term stays in loss_parts[3] and the MSE comes back as mse"""
    from nbest_amd import trainer
    from test_optim_adam_gpu import _batch, _model
    m = _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(m, labels, B=6)
    b["tids"][4], b["tseg"][4] = b["tids"][1], b["tseg"][1]
    kw = {}
    if other == "rdrop":
        b = trainer.rdrop_batch(b)
        kw["rdrop"] = dict(alpha=0.7)
    else:
        teacher = _model(labels, torch.bfloat16, seed=22)
        kw["distill"] = trainer.teacher_scores(teacher, b["ids"], b["seg"], 0.5)
    keys = trainer.transcript_keys(b["tids"])
    rows = b["ids"].shape[0]
    assert keys[4].item() == 1 and (other != "rdrop" or (rows == 12 and torch.equal(keys[6:], keys[:6]) and keys[10].item() == 1))
    out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True,
                             tok_perm=b.get("tok_perm"), trans_tok_perm=b.get("ttok_perm"),
                             contrast=dict(weight=1.0, temperature=0.1, keys=keys), **kw)
    torch.cuda.synchronize()
    want = contrast_reference(out["asr_cls"].double().cpu(), out["trans_cls"].double().cpu(), keys.cpu(), 1.0, 0.1)
    c = out["contrast"].double().cpu()
    print("forward_backward(contrast=, %s=) bf16: contrast %.6f vs %.6f, hits %d vs %d" % (other, c[0], want["L"], c[1], want["hits"]))
    assert abs(c[0].item() - want["L"].item()) <= 1e-5 * want["L"].item() and c[2].item() == rows
    assert out["mse"].shape == (1,) and out["mse"].item() > 0 and out["loss_parts"][3].item() > 0
    assert torch.isfinite(m.arena.g).all()


def test_train_step_with_contrast(labels):
    """a 1-layer bf16 model, B 8, S 32, 21 steps on one batch at weight 1, temperature 0.1: the contrastive term and the hard loss
    fall and the optimizer stepped once per call; a teacher next to the flag works, adv_epsilon next to it raises"""
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import train_step
    from test_optim_adam_gpu import BERT_LR, LR, _batch, _model
    m = _model(labels, torch.bfloat16, layers=1, seed=34, dropout=0.3)
    opt = HipBertAdam(m, lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=40)
    b = _batch(m, labels, B=8, S=32)
    parts, con = [], []
    for _ in range(21):
        out = train_step(m, opt, b, contrast_weight=1.0, contrast_temperature=0.1)
        parts.append(out["loss_parts"].clone())
        con.append(out["contrast"].clone())
    torch.cuda.synchronize()
    parts, con = torch.stack(parts).double().cpu(), torch.stack(con).double().cpu()
    hard = parts[:, :3].sum(dim=1).tolist()
    print("train_step(contrast_weight=1): hard loss %.4f -> %.4f, contrast %.4f -> %.4f, hits %d -> %d of 8 over 20 steps" % (
        hard[0], hard[20], con[0, 0], con[20, 0], con[0, 1], con[20, 1]))
    assert con[20, 0].item() < con[0, 0].item() and hard[20] < hard[0], (hard, con[:, 0].tolist())
    assert opt.step_count == 21 and (parts[:, 3] == 0).all() and (con[:, 2] == 8).all()
    teacher = _model(labels, torch.bfloat16, layers=1, seed=35)
    out = train_step(m, opt, b, teacher=teacher, contrast_weight=1.0)
    assert opt.step_count == 22 and out["contrast"][0].item() > 0 and out["loss_parts"][3].item() > 0
    with pytest.raises(ValueError, match="contrast_weight"):
        train_step(m, opt, b, adv_epsilon=1.0, contrast_weight=1.0)
    assert opt.step_count == 22


@pytest.mark.parametrize("mode", ["ema", "freeze", "adam", "adamw"])
def test_train_step_with_what_the_flag_combines_with(mode, labels):
    """one train_step with contrast_weight=1 on the small bf16 model (2 layers, B 6) under --ema_decay, --freeze_embeddings
    --freeze_layers 1 and the two other optimizers: the term is returned, the optimizer stepped once, a trainable matrix moved and a
    frozen one did not"""
    from nbest_amd import cli
    from nbest_amd.optim import HipAdam, HipBertAdam
    from nbest_amd.trainer import train_step
    from test_optim_adam_gpu import BERT_LR, LR, _batch, _model
    m = _model(labels, torch.bfloat16, dropout=0.3)
    frozen = cli.freeze_parameters(m, embeddings=True, layers=1) if mode == "freeze" else []
    if mode in ("adam", "adamw"):
        opt = HipAdam(m, kind=mode, lr=LR, bert_lr=BERT_LR, warmup=0.0, t_total=40)
    else:
        opt = HipBertAdam(m, lr=LR, bert_lr=BERT_LR, ema_decay=0.9 if mode == "ema" else None)    # (no schedule: BertAdam's warm-up starts at lr 0)
    b = _batch(m, labels, B=6)
    named = dict(m.named_parameters())
    top, low = "bert_encoder.encoder.layer.1.output.dense.weight", "bert_encoder.encoder.layer.0.output.dense.weight"
    before = {n: named[n].detach().clone() for n in (top, low)}
    out = train_step(m, opt, b, contrast_weight=1.0, contrast_temperature=0.1)
    torch.cuda.synchronize()
    c = out["contrast"]
    assert torch.isfinite(c).all() and c[0].item() > 0 and c[2].item() == 6 and opt.step_count == 1
    assert not torch.equal(named[top].detach(), before[top])
    assert torch.equal(named[low].detach(), before[low]) == (mode == "freeze") and (low in frozen) == (mode == "freeze")
    if mode == "ema":
        with opt.ema_weights():
            ev = m.predict(b["ids"], b["seg"])
        assert torch.isfinite(ev["top"]).all()


def test_gradient_accumulation_uses_the_negatives_of_the_micro_batch(labels):
    """two micro-batches of 3 with ``accumulate``: contrast[2] is 3 in both calls (the negatives are the micro-batch's) and arena.g
    holds the sum of the two calls' gradients (dropout 0; 1e-3 of the sum's norm: the accumulating kernels add in fp32, a term lost or
    doubled would show at order 1)"""
    from test_optim_adam_gpu import _batch, _model
    m, twin = _model(labels, torch.bfloat16), _model(labels, torch.bfloat16)
    b = _batch(m, labels, B=6)
    con = dict(weight=1.0, temperature=0.1)
    call = lambda mm, lo, **kw: mm.forward_backward(b["ids"][lo:lo + 3], b["labels"][lo:lo + 3], seg_ids=b["seg"][lo:lo + 3],
                                                    trans_input_ids=b["tids"][lo:lo + 3], trans_seg_ids=b["tseg"][lo:lo + 3],
                                                    contrast=con, **kw)
    o1 = call(m, 0)
    g1 = m.arena.g.clone()
    o2 = call(m, 3, accumulate=True)
    call(twin, 3)
    torch.cuda.synchronize()
    assert o1["contrast"][2].item() == 3 and o2["contrast"][2].item() == 3 and o2["contrast"][0].item() > 0
    want = g1.double() + twin.arena.g.double()
    err = (m.arena.g.double() - want).norm().item() / want.norm().item()
    print("accumulate with contrast: |g - (g1 + g2)| / |g1 + g2| = %.2e" % err)
    assert err <= 1e-3 and not torch.equal(m.arena.g, g1)


def test_cli_contrastive_weight(tmp_path):
    """one epoch on valid_head.txt with --contrastive_weight 1.0: the __cl_1.0_0.1 directory, the naming line, the per-epoch contrast
    line and a parsable [Train] line exist; --testing is refused with the flag and, without it, reproduces the valid F1 line on a
    copy of model.pt in the plain-named directory"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    plain = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
             "--bert_dropout", "0.1", "--optim_choice", "bertadam", "--lr", "1e-2", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
             "--batchSize", "4", "--max_epoch", "1", "--experiment", str(tmp_path / "exp"), "--pre_trained_model", "bert",
             "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
             "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "1", "--n_best", "5"]
    args = plain + ["--contrastive_weight", "1.0", "--resume"]
    assert cli.main(args) == 0
    d = cli.exp_dir(cli.parse_arguments(args))
    assert d.endswith("__cl_1.0_0.1") and os.path.isdir(d)
    pt = os.path.join(d, "model.pt")
    if not os.path.isfile(pt):         # written on a NEW BEST valid F1 only: otherwise the epoch's weights
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], pt)
    log = open(os.path.join(d, "log.train")).read().split("\n")
    assert sum(l.startswith("Contrastive: weight 1.0, temperature 0.1;") for l in log) == 1
    train = [l for l in log if l.startswith("[Train]\tEpoch: 00")]
    assert len(train) == 1
    loss, f1 = re.search(r"Loss: ([0-9.]+)\t\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)", train[0]).groups()
    assert 0.0 < float(loss) < 1e4 and 0.0 <= float(f1) <= 100.0
    con = [l for l in log if l.startswith("[Contrast]\tEpoch: 00")]
    assert len(con) == 1 and log.index(con[0]) == log.index(train[0]) + 1
    closs, align = re.fullmatch(r"\[Contrast\]\tEpoch: 00\tLoss: ([0-9.]+)\tAlign: ([0-9.]+)", con[0]).groups()
    assert 0.0 < float(closs) < 10.0 and 0.0 <= float(align) <= 100.0
    valid = [l for l in log if l.startswith("[Valid]\tEpoch: 00")][0]
    f1, acc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", valid).groups()
    with pytest.raises(SystemExit):
        cli.main(args + ["--testing"])
    d_test = cli.exp_dir(cli.parse_arguments(plain))
    assert d_test != d and d == d_test + "__cl_1.0_0.1"
    os.makedirs(d_test)
    shutil.copy(pt, os.path.join(d_test, "model.pt"))
    assert cli.main(plain + ["--testing"]) == 0
    line = [l for l in open(os.path.join(d_test, "log.test")).read().split("\n") if l.startswith("[Valid]")][0]
    tf1, tacc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", line).groups()
    assert (tf1, tacc) == (f1, acc), (line, valid)
