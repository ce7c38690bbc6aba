"""GPU: distillation at a temperature.  nbest_stc_heads_logits against fp64 and against the scores of nbest_stc_heads;
nbest_stc_heads_kd_t against the fp64 restatement of tests/test_distill_temperature_cpu.py, against the probability kernel at T = 1
and against the plain kernel at alpha = 0; predict(return_logits=True); forward_backward(distill=dict(logits=, alpha=,
temperature=)) on a whole fp32 model against the oracle under torch autograd; train_step with a teacher and a temperature; and
--distill_temperature through the CLI.  The kernel tests use the shapes of tests/test_distill_gpu.py."""
import os
import re
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_distill_cpu import heads_scores, soft_loss
from test_distill_gpu import DEV, H, _kd, _problem, _ratio, _space
from test_distill_temperature_cpu import kd_t_reference, scores_from_logits

pytestmark = pytest.mark.gpu

NAMES = ("top", "bott", "final", "loss_parts", "dcls", "dWh", "dbh")


def _c(x):
    return None if x is None else x.to(DEV).contiguous()


def _logits(dls, hidden, Wh, bh):
    from nbest_amd import hipabi as hb
    B = hidden.shape[0]
    out = hb.stc_heads_logits(_c(hidden.reshape(B * 2, H)), 2 * H, _c(Wh), _c(bh), dls, B, H)
    torch.cuda.synchronize()
    return out


def _plain(dls, hidden, Wh, bh, y, **kw):
    from nbest_amd import hipabi as hb
    B = hidden.shape[0]
    out = hb.stc_heads(_c(hidden.reshape(B * 2, H)), 2 * H, _c(Wh), _c(bh), dls, _c(y), B, H, **kw)
    torch.cuda.synchronize()
    return dict(zip(NAMES, out))


def _kd_t(dls, hidden, Wh, bh, y, t_logits, alpha, T, **kw):
    from nbest_amd import hipabi as hb
    B = hidden.shape[0]
    out = hb.stc_heads_kd_t(_c(hidden.reshape(B * 2, H)), 2 * H, _c(Wh), _c(bh), dls, _c(y), _c(t_logits), alpha, T, B, H, **kw)
    torch.cuda.synchronize()
    return dict(zip(NAMES, out))


def _teacher_logits(hidden, Wh, bh, seed, saturate):
    """6 x randn; with ``saturate`` the last row's teacher logits are that row's own (fp64, rounded to fp32): about +115 / -115 on
    its first two tops, so the teacher's tempered scores saturate with the student's and clamped logs (-100, in fp32 and in fp64)
    enter the soft loss with the weights 0 and 1 - and not NaN - and the 1e-12 denominators enter its gradient"""
    gen = torch.Generator().manual_seed(seed)
    B, R = hidden.shape[0], Wh.shape[0]
    tz = 6.0 * torch.randn(B, R, generator=gen)
    if saturate:
        tz[B - 1] = (hidden[B - 1, 0].double() @ Wh.double().t() + bh.double()).float()
    return tz


def _soft_t(z_student, z_teacher, T, top2bottom):
    """fp64: T^2 x the soft loss of the tempered scores of two rows of logits"""
    d = lambda x: x.detach().double().cpu()
    return (T * T * soft_loss(*scores_from_logits(d(z_student) / T, top2bottom), *scores_from_logits(d(z_teacher) / T, top2bottom),
                              top2bottom)).item()


# ---- 1. the logits kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_logits_kernel(space, B, dtype, labels):
    """stc_heads_logits against cls @ Wh^T + bh in fp64 on the same (fp32 or bf16) CLS rows, and sigmoid / per-head softmax of the
    returned logits (fp64) against the top / bott stc_heads returns for the same inputs at dropout 0; 1e-5, K7's bar for scores"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, B, dtype, seed=7 + B, saturate=B > 1)
    got = _logits(dls, hidden, Wh, bh)
    assert got.shape == (B, dls.n_rows) and got.dtype == torch.float32
    ref = hidden[:, 0, :].double() @ Wh.double().t() + bh.double()
    worst = {}
    _ratio("logits", got, ref, 1e-5, worst)
    plain = _plain(dls, hidden, Wh, bh, y, need_grad=False)
    top, bott, final = scores_from_logits(got.double().cpu(), ls.top2bottom)
    _ratio("sigmoid(logits) vs top", top, plain["top"], 1e-5, worst)
    _ratio("softmax(logits) vs bott", bott, plain["bott"], 1e-5, worst)
    _ratio("final", final, plain["final"], 1e-5, worst)
    print("stc_heads_logits %s B=%d %s: worst error / bar %s" % (
        space, B, str(dtype)[6:], ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert torch.equal(_logits(dls, hidden, Wh, bh), got)


# ---- 2. the tempered kernel against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_kernel_matches_the_fp64_restatement(space, B, alpha, T, dtype, labels):
    """scores, loss_parts[0..3], dcls, dWh and dbh of nbest_stc_heads_kd_t against kd_t_reference in fp64 on the same CLS rows, at
    the bars of tests/test_distill_gpu.py's kernel test (scores and losses 1e-5, gradients 1e-4 of the tensor's largest element).
    B = 5 carries the saturated row."""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, B, dtype, seed=7 + B, saturate=B > 1)
    tz = _teacher_logits(hidden, Wh, bh, seed=70 + B, saturate=B > 1)
    got = _kd_t(dls, hidden, Wh, bh, y, tz, alpha, T)
    ref = kd_t_reference(hidden[:, 0, :].float(), Wh, bh, y, tz, alpha, T, ls.top2bottom)
    if B > 1:
        assert got["top"][B - 1, 0].item() == 1.0 and got["top"][B - 1, 1].item() == 0.0, "the saturated row does not reach the clamps"
    worst = {}
    for k in ("top", "bott", "final"):
        _ratio(k, got[k], ref[k], 1e-5, worst)
    _ratio("loss_parts", got["loss_parts"], ref["loss_parts"], 1e-5, worst)
    _ratio("soft loss", got["loss_parts"][3:], ref["loss_parts"][3:], 1e-5, worst)
    for k in ("dcls", "dWh", "dbh"):
        _ratio(k, got[k], ref[k], 1e-4, worst)
    print("stc_heads_kd_t %s B=%d alpha=%g T=%g %s: worst error / bar %s" % (
        space, B, alpha, T, str(dtype)[6:], ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# ---- 3. T = 1 against the probability kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_temperature_one_against_the_probability_kernel(space, alpha, labels):
    """the teacher is a second head matrix on other CLS rows (logits of sd ~ 6): stc_heads_kd_t(T = 1) fed its stc_heads_logits
    against stc_heads_kd fed its stc_heads scores - all seven outputs within the bars of the restatement test"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, 5, torch.float32, seed=12, saturate=True)
    _, t_hidden, Wt, bt, _, _, _, _ = _problem(ls, 5, torch.float32, seed=13, saturate=False)
    Wt = Wt * 4.0
    tz = _logits(dls, t_hidden, Wt, bt)
    t = _plain(dls, t_hidden, Wt, bt, y, need_grad=False)
    a = _kd_t(dls, hidden, Wh, bh, y, tz, alpha, 1.0)
    b = _kd(dls, hidden, Wh, bh, y, t["top"], t["bott"], t["final"], alpha)
    worst = {}
    for k in ("top", "bott", "final", "loss_parts"):
        _ratio(k, a[k], b[k], 1e-5, worst)
    _ratio("soft loss", a["loss_parts"][3:], b["loss_parts"][3:], 1e-5, worst)
    for k in ("dcls", "dWh", "dbh"):
        _ratio(k, a[k], b[k], 1e-4, worst)
    same = [k for k in NAMES if torch.equal(a[k], b[k])]
    print("stc_heads_kd_t(T = 1) vs stc_heads_kd %s alpha=%g: worst error / bar %s; bit-identical: %s" % (
        space, alpha, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), ", ".join(same) or "none"))


# ---- 4. alpha = 0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_alpha_zero_is_the_plain_kernel(space, labels):
    """dropout 0.3, the same seed: every output of stc_heads_kd_t(alpha = 0, T = 3) has the bits of stc_heads's; loss_parts[3] is
    the tempered soft loss of the scores the kernel returned - their logits recovered in fp64 as log(p / (1 - p)) and log(s), a
    head's logits being free by a constant; two calls give the same bits"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, 5, torch.float32, seed=3, saturate=False)
    tz = _teacher_logits(hidden, Wh, bh, seed=4, saturate=False)
    kw = dict(drop_p=0.3, seed=4321, drop_stream=900)
    T = 3.0
    got = _kd_t(dls, hidden, Wh, bh, y, tz, 0.0, T, **kw)
    again = _kd_t(dls, hidden, Wh, bh, y, tz, 0.0, T, **kw)
    plain = _plain(dls, hidden, Wh, bh, y, **kw)
    nodrop = _kd_t(dls, hidden, Wh, bh, y, tz, 0.0, T)
    assert not torch.equal(nodrop["top"], got["top"])                       # the dropout is on
    for k in ("top", "bott", "final", "dcls", "dWh", "dbh"):
        assert torch.equal(got[k], plain[k]), k
    assert torch.equal(got["loss_parts"][:3], plain["loss_parts"][:3]) and plain["loss_parts"][3].item() == 0.0
    for k in NAMES:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
    top, bott = got["top"].double().cpu(), got["bott"].double().cpu()
    z = torch.cat([torch.log(top) - torch.log1p(-top), torch.log(bott)], dim=1)
    want = _soft_t(z, tz, T, ls.top2bottom)
    assert want > 1.0 and abs(got["loss_parts"][3].item() - want) <= 1e-5 * want, (got["loss_parts"][3].item(), want)
    # alpha = 0 without a teacher is the plain kernel too
    none = _kd_t(dls, hidden, Wh, bh, y, None, 0.0, T, **kw)
    for k in NAMES:
        assert torch.equal(none[k], plain[k]), k
    with pytest.raises(RuntimeError, match="stc_heads_kd_t"):
        _kd_t(dls, hidden, Wh, bh, y, tz, 0.5, 0.0)
    with pytest.raises(ValueError, match="t_logits"):
        _kd_t(dls, hidden, Wh, bh, y, tz[:, :-1], 0.5, 2.0)


# ---- 5. predict(return_logits=True) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_predict_return_logits(dtype, labels):
    """bert_L2, B 4, S 48: the other outputs keep their bits, logits is fp32 [B, R] and agrees with the model's own CLS rows through
    the head matrix in fp64 at the kernel's bar"""
    from test_model_gpu import _build
    meta, _ = load_case("bert_L2")
    m, b = _build(meta, labels, dtype)
    seg = b["seg"] if meta["seg"] else None
    base = m.predict(b["ids"], seg_ids=seg)
    out = m.predict(b["ids"], seg_ids=seg, return_logits=True)
    torch.cuda.synchronize()
    assert "logits" not in base and set(out) == set(base) | {"logits"}
    for k in ("top", "bott", "final", "cls", "pred"):
        assert torch.equal(out[k], base[k]), k
    B = b["ids"].shape[0]
    assert out["logits"].shape == (B, m.dls.n_rows) and out["logits"].dtype == torch.float32
    Wh, bh = m.arena.heads_wb()
    ref = out["cls"].double() @ Wh.double().t() + bh.double()
    worst = {}
    _ratio("logits", out["logits"], ref, 1e-5, worst)
    top, bott, final = scores_from_logits(out["logits"].double().cpu(), labels.top2bottom)
    _ratio("top", top, out["top"], 1e-5, worst)
    _ratio("bott", bott, out["bott"], 1e-5, worst)
    print("predict(return_logits=True) bert_L2 %s: worst error / bar %s" % (
        str(dtype)[6:], ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_training_step_after_predict_return_logits_is_unchanged(labels):
    from nbest_amd.optim import HipBertAdam
    from test_model_gpu import _build
    meta, _ = load_case("bert_L2")
    res = []
    for with_logits in (False, True):
        m, b = _build(meta, labels, torch.bfloat16)
        seg = b["seg"] if meta["seg"] else None
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_logits:
            m.predict(b["ids"], seg_ids=seg, return_logits=True)
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=seg, trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after predict(return_logits=True) differs"


# ---- 6. the whole model --------------------------------------------------------------------------------------------------------------
def test_whole_model_fp32_matches_the_oracle_under_autograd(labels):
    """bert_L2, alpha 0.5, T 2: the arena gradients of forward_backward(distill=dict(logits=, alpha=, temperature=)) against the
    oracle model with (1 - alpha) * hard + alpha * soft_T (+ MSE) under torch autograd - soft_T built from the oracle's CLS row and
    head parameters (its tempered scores are its heads on Wh / T, bh / T) - at the fp32 gradient bars of tests/test_model_gpu.py;
    then the no-distill path, the probability form and the refusal of a mixed dict"""
    from test_model_gpu import _build, _oracle_for
    from conftest import case_inputs
    from oracle import stc
    meta, z = load_case("bert_L2")
    alpha, T = 0.5, 2.0
    cfg, sd, batch = case_inputs(meta, labels)
    B, R = batch["ids"].shape[0], labels.n_top + sum(len(labels.top2bottom[k]) for k in labels.multi)
    tz = 3.0 * torch.randn(B, R, generator=torch.Generator().manual_seed(17))
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"] if meta["seg"] else None, trans_seg_ids=t["tseg"])
    _, _, parts = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, stc.bottom2top_matrix(labels.top2bottom),
                                 asr, tr, meta["add_l2"])
    lins = [om.clf.top_linear_layer] + [om.clf.linear_layers["lin_%d" % k] for k in labels.multi]
    Wo, bo = torch.cat([l.weight for l in lins], dim=0), torch.cat([l.bias for l in lins], dim=0)
    assert Wo.shape[0] == R
    s_top, s_bott, s_fin = heads_scores(asr, Wo, bo, labels.top2bottom)
    assert torch.allclose(s_top, top, atol=1e-6) and torch.allclose(s_fin, final, atol=1e-6)         # the fused matrix is the oracle's heads
    soft = T * T * soft_loss(*heads_scores(asr, Wo / T, bo / T, labels.top2bottom), *scores_from_logits(tz / T, labels.top2bottom),
                             labels.top2bottom)
    total = (1.0 - alpha) * (parts["bottom_bce"] + parts["top_bce"] + parts["ce"]) + alpha * soft
    if meta["add_l2"]:
        total = total + parts["mse"]
    total.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    m, b = _build(meta, labels, torch.float32)
    twin, _ = _build(meta, labels, torch.float32)
    kw = dict(seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"])
    distill = dict(logits=tz.cuda(), alpha=alpha, temperature=T)
    runs = []
    for _ in range(2):
        out = m.forward_backward(b["ids"], b["labels"], distill=distill, **kw)
        twin.forward_backward(b["ids"], b["labels"], **kw)
        torch.cuda.synchronize()
        runs.append(m.arena.g.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "the distillation step is not bit-reproducible"
    assert not torch.equal(twin.arena.g, m.arena.g)
    lp = out["loss_parts"].double().cpu()
    hard = (parts["bottom_bce"] + parts["top_bce"] + parts["ce"]).item()
    print("forward_backward(distill=logits, T=2) bert_L2 fp32: hard loss %.6f vs %.6f, soft loss %.6f vs %.6f" % (lp[:3].sum(), hard, lp[3], soft.item()))
    assert abs(lp[:3].sum().item() - hard) <= 1e-4 * hard and abs(lp[3].item() - soft.item()) <= 1e-4 * soft.item()   # the fp32 loss bar
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
    print("forward_backward(distill=logits, T=2) bert_L2 fp32: worst gradient noise-to-signal %.3e (%s), bar 2e-3" % worst)
    # a forward_backward without distill has the bits of a model that never saw one
    o1 = m.forward_backward(b["ids"], b["labels"], **kw)
    o2 = twin.forward_backward(b["ids"], b["labels"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(m.arena.g.view(torch.int32), twin.arena.g.view(torch.int32)) and m.step_counter == twin.step_counter
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(o1[k], o2[k]), k
    assert torch.equal(o1["top"], out["top"]) and torch.equal(o1["loss_parts"][:3], out["loss_parts"][:3])
    # the probability form still works on the same model, and the two key sets do not mix
    t_top, t_bott, t_fin = (x.float().cuda() for x in scores_from_logits(tz.double(), labels.top2bottom))
    prob = dict(top=t_top, bott=t_bott, final=t_fin, alpha=alpha)
    o3 = m.forward_backward(b["ids"], b["labels"], distill=prob, **kw)
    o4 = m.forward_backward(b["ids"], b["labels"], distill=dict(distill, temperature=1.0), **kw)
    torch.cuda.synchronize()
    s3, s4 = o3["loss_parts"][3].item(), o4["loss_parts"][3].item()
    assert s3 > 0 and abs(s3 - s4) <= 1e-5 * s3, (s3, s4)
    g0 = m.arena.g.clone()
    for bad in (dict(distill, top=t_top), dict(prob, temperature=T), dict(logits=tz.cuda(), alpha=alpha), dict(distill, temperature=0.0),
                dict(distill, temperature=float("nan")), dict(distill, temperature=float("inf")), dict(distill, alpha=1.5),
                dict(distill, logits=tz.cuda().double()), dict(distill, logits=tz.cuda()[:, :-1]), dict(distill, logits=tz)):
        with pytest.raises(ValueError, match="distill"):
            m.forward_backward(b["ids"], b["labels"], distill=bad, **kw)
    with pytest.raises(RuntimeError, match="distill"):
        m(None, b["ids"], seg_ids=kw["seg_ids"], distill=distill)
    torch.cuda.synchronize()
    assert torch.equal(m.arena.g, g0), "a refused call must leave the gradients alone"


# ---- 7. train_step -------------------------------------------------------------------------------------------------------------------
def test_train_step_with_a_teacher_and_a_temperature(labels):
    """the set-up of tests/test_distill_gpu.py's train_step test (2-layer teacher, 1-layer student from its layer 1, B 8, S 32, no
    dropout, alpha 1) at T = 2: loss_parts[3] of the first step is T^2 x the restated soft loss of the two models'
    predict(return_logits=True), the soft loss falls over 20 steps, nothing of the teacher changes"""
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import student_state_from_teacher, teacher_scores, train_step
    from test_optim_adam_gpu import BERT_LR, LR, _batch, _model
    T = 2.0
    teacher = _model(labels, torch.bfloat16, layers=2, seed=33)
    student = _model(labels, torch.bfloat16, layers=1, seed=34)
    tsd = {k: v.detach().cpu() for k, v in teacher.state_dict().items()}
    student.load_reference_state(student_state_from_teacher(tsd, [1]))
    opt = HipBertAdam(student, lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=40)
    b = _batch(student, labels, B=8, S=32)
    form = teacher_scores(teacher, b["ids"], b["seg"], 1.0, T)
    assert set(form) == {"logits", "alpha", "temperature"} and form["temperature"] == T and form["alpha"] == 1.0
    assert set(teacher_scores(teacher, b["ids"], b["seg"], 1.0)) == {"top", "bott", "final", "alpha"}
    zs = student.predict(b["ids"], seg_ids=b["seg"], return_logits=True)["logits"]
    zt = teacher.predict(b["ids"], seg_ids=b["seg"], return_logits=True)["logits"]
    torch.cuda.synchronize()
    assert torch.equal(zt, form["logits"])
    want = _soft_t(zs, zt, T, labels.top2bottom)
    before = {n: getattr(teacher.arena, n).clone() for n in ("p", "w16", "g") if getattr(teacher.arena, n) is not None}
    soft = []
    for _ in range(21):
        out = train_step(student, opt, b, teacher=teacher, distill_alpha=1.0, distill_temperature=T)
        soft.append(out["loss_parts"][3:4])
    torch.cuda.synchronize()
    soft = torch.cat(soft).cpu().tolist()
    print("train_step with a teacher, T = 2: soft loss %.6f (restated from predict: %.6f, rel %.2e) -> %.4f over 20 steps"
          % (soft[0], want, abs(soft[0] - want) / want, soft[20]))
    assert abs(soft[0] - want) <= 1e-5 * want, (soft[0], want)
    assert soft[20] < soft[0], soft
    assert not teacher.training and teacher.step_counter == 0 and opt.step_count == 21
    for n, x in before.items():
        assert torch.equal(getattr(teacher.arena, n).view(torch.uint8), x.view(torch.uint8)), n


# ---- 8. the command line -------------------------------------------------------------------------------------------------------------
def test_cli_distill_temperature(tmp_path):
    """a 2-layer teacher for one epoch, then a 1-layer student with --distill_from / --distill_temperature 2 for one epoch: the run
    ends, exp_dir carries __kd_0.5__kdT_2.0, log.train names T, and model.pt loads for --testing from the directory named without
    the kd_ / kdT_ parts"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")

    def common(exp, layers):
        return ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
                "--bert_dropout", "0.1", "--optim_choice", "bertadam", "--lr", "1e-2", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
                "--batchSize", "2", "--max_epoch", "1", "--experiment", str(tmp_path / exp), "--pre_trained_model", "bert",
                "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
                "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", str(layers), "--n_best", "5"]
    t_args = common("teacher", 2) + ["--resume"]
    assert cli.main(t_args) == 0
    t_dir = cli.exp_dir(cli.parse_arguments(t_args))
    t_pt = os.path.join(t_dir, "model.pt")
    if not os.path.isfile(t_pt):       # written on a NEW BEST valid F1 only: otherwise the epoch's weights (tests/test_cli_gpu.py does the same)
        torch.save(torch.load(os.path.join(t_dir, "last.pt"), weights_only=True)["model"], t_pt)
    s_plain = common("student", 1)
    s_args = s_plain + ["--distill_from", t_pt, "--distill_teacher_layers", "2", "--distill_init_layers", "1", "--distill_alpha", "0.5",
                        "--distill_temperature", "2"]
    assert cli.main(s_args) == 0
    d = cli.exp_dir(cli.parse_arguments(s_args))
    assert d.endswith("__kd_0.5__kdT_2.0") and os.path.isdir(d)
    assert os.path.isfile(os.path.join(d, "model.pt")), "the student's epoch reached no valid F1 above 0"
    log = open(os.path.join(d, "log.train")).read().split("\n")
    assert log[1].startswith("Distillation: teacher %s (2 layers), alpha 0.5, temperature 2.0" % t_pt), log[1]
    assert log[1].endswith("Loss below is the hard loss")
    best = [l for l in log if l.startswith("NEW BEST:")]
    f1, acc = re.search(r"valid F1/Acc: ([0-9.]+)/([0-9.]+)", best[-1]).groups()
    # --testing refuses the flags; without them the directory has neither part: evaluate a copy of model.pt there
    d_test = cli.exp_dir(cli.parse_arguments(s_plain))
    assert "kd" not in os.path.basename(d_test)
    os.makedirs(d_test)
    shutil.copy(os.path.join(d, "model.pt"), os.path.join(d_test, "model.pt"))
    assert cli.main(s_plain + ["--testing"]) == 0
    line = [l for l in open(os.path.join(d_test, "log.test")).read().split("\n") if l.startswith("[Valid]")][0]
    tf1, tacc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", line).groups()
    assert (tf1, tacc) == (f1, acc), (line, best[-1])
