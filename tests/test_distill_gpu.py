"""GPU: knowledge distillation.  nbest_stc_heads_kd against the fp64 restatement of tests/test_distill_cpu.py (losses and the three
gradients), its alpha = 0 and one-hot-teacher identities, forward_backward(distill=) on a whole fp32 model against the oracle under
torch autograd, the untouched no-distill path, train_step with a teacher, and --distill_from through the CLI."""
import os
import re
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_distill_cpu import _teacher_draw, heads_scores, kd_reference, onehot_teacher, soft_loss

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = 768
# a single-bottom top, a 2-column head and a head of 70 columns (more than a wave: the strided nk > 64 path); R = 3 + 2 + 70
WIDE_SPACE = {0: [0], 1: [1, 2], 2: list(range(3, 73))}


def _space(name, labels):
    from nbest_amd.config import LabelSpace
    if name == "shipped":
        return labels
    return LabelSpace(WIDE_SPACE, ["s0", "a-x", "a-NONE"] + ["b-%d" % i for i in range(69)] + ["b-NONE"])


def _ratio(name, got, ref, tol, worst):
    """the bar of tests/test_kernels_gpu.py's ``close``: max |got - ref| <= tol x max |ref|; records error / bar"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item() / scale
    worst[name] = max(worst.get(name, 0.0), err / tol)
    assert err == err and err <= tol, "%s: rel err %.3e > %.1e (scale %.3e)" % (name, err, tol, scale)


def _problem(ls, B, dtype, seed, saturate):
    """CLS rows (row stride 2 H, as a [B, 2, H] hidden state), head matrix, labels with at most one bottom per top, and a teacher:
    random sigmoid / softmax draws.  ``saturate``: the last row's CLS features get 60 x (row 0 - row 1 of the head matrix) added, so
    its first two top logits are about +115 and -115: the fp32 scores are exactly 1 and 0 and their logs run into the -100 clamp
    (its other logits have sd ~ 6); its labels and teacher scores are exactly 0 / 1, on the side its scores fall - but for the
    teacher's values on the two saturated tops, set to 0.3, so that clamped terms enter the soft loss and its gradient (fp64 runs
    into the same clamps there: sigmoid(115) is 1 in fp64 too, and log(sigmoid(-115)) = -115 < -100)"""
    from nbest_amd import hipabi as hb
    gen = torch.Generator().manual_seed(seed)
    dls = hb.DeviceLabelSpace(ls, DEV)
    R = dls.n_rows
    Wh, bh = torch.randn(R, H, generator=gen) * 0.05, torch.randn(R, generator=gen) * 0.05
    hidden = torch.randn(B, 2, H, generator=gen)
    if saturate:
        hidden[B - 1, 0] += 60.0 * (Wh[0] - Wh[1])
    hidden = hidden.to(dtype)
    y = torch.zeros(B, ls.n_bottom)
    for b in range(B):
        for t in torch.randperm(ls.n_top, generator=gen)[:2].tolist():
            bs = ls.top2bottom[t]
            y[b, bs[int(torch.randint(0, len(bs), (1,), generator=gen))]] = 1
    t_top, t_bott, t_fin = (x.float() for x in _teacher_draw(B, ls.top2bottom, gen))
    if saturate:
        cls64 = hidden[B - 1:, 0, :].double()
        top, bott, _ = heads_scores(cls64, Wh.double(), bh.double(), ls.top2bottom)
        fire = (top > 0.5).float()
        hot, col = [], 0
        yb = torch.zeros(1, ls.n_bottom)
        for t in range(ls.n_top):
            bs = ls.top2bottom[t]
            if len(bs) >= 2:
                am = int(bott[0, col:col + len(bs)].argmax())
                hot.append(torch.nn.functional.one_hot(torch.tensor([am]), len(bs)).float())
                yb[0, bs[am]] = fire[0, t]
                col += len(bs)
            else:
                yb[0, bs[0]] = fire[0, t]
        t_top[B - 1:], t_bott[B - 1:], t_fin[B - 1:], y[B - 1:] = fire, torch.cat(hot, dim=1), yb, yb
        assert set(t_top[B - 1].tolist()) <= {0.0, 1.0} and set(t_fin[B - 1].tolist()) <= {0.0, 1.0}
        # ... except fractional teacher values on the two saturated tops and on the final scores under the second (all exactly 0):
        # there a clamped log (-100) carries weight in the soft loss (0.7 x 100 on top 0; 0.3 x 100 on top 1 and on each of its
        # final scores) and the 1e-12 denominator meets a non-zero numerator in the soft gradient
        t_top[B - 1, 0] = t_top[B - 1, 1] = 0.3
        t_fin[B - 1, ls.top2bottom[1]] = 0.3
    return dls, hidden, Wh, bh, y, t_top, t_bott, t_fin


def _kd(dls, hidden, Wh, bh, y, t_top, t_bott, t_fin, alpha, **kw):
    from nbest_amd import hipabi as hb
    B = hidden.shape[0]
    c = lambda x: None if x is None else x.to(DEV).contiguous()
    out = hb.stc_heads_kd(c(hidden.reshape(B * 2, H)), 2 * H, c(Wh), c(bh), dls, c(y), c(t_top), c(t_bott), c(t_fin), alpha, B, H, **kw)
    torch.cuda.synchronize()
    return dict(zip(("top", "bott", "final", "loss_parts", "dcls", "dWh", "dbh"), out))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_kernel_matches_the_fp64_restatement(space, B, alpha, dtype, labels):
    """loss_parts[0..3], dcls, dWh and dbh of nbest_stc_heads_kd against the restatement in fp64 on the same (fp32 or bf16) CLS rows,
    at the bars tests/test_kernels_gpu.py's heads test applies to the same quantities (scores and losses 1e-5, gradients 1e-4 of
    the tensor's largest element).  B = 5 carries the saturated row."""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, t_top, t_bott, t_fin = _problem(ls, B, dtype, seed=7 + B, saturate=B > 1)
    got = _kd(dls, hidden, Wh, bh, y, t_top, t_bott, t_fin, alpha)
    ref = kd_reference(hidden[:, 0, :].float(), Wh, bh, y, t_top, t_bott, t_fin, alpha, ls.top2bottom)
    if B > 1:
        assert got["top"][B - 1, 0].item() == 1.0 and got["top"][B - 1, 1].item() == 0.0, "the saturated row does not reach the clamps"
    worst = {}
    for k in ("top", "bott", "final"):
        _ratio(k, got[k], ref[k], 1e-5, worst)
    _ratio("loss_parts", got["loss_parts"], ref["loss_parts"], 1e-5, worst)
    _ratio("soft loss", got["loss_parts"][3:], ref["loss_parts"][3:], 1e-5, worst)
    for k in ("dcls", "dWh", "dbh"):
        _ratio(k, got[k], ref[k], 1e-4, worst)
    print("stc_heads_kd %s B=%d alpha=%g %s: worst error / bar %s" % (
        space, B, alpha, str(dtype)[6:], ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_alpha_zero_is_the_plain_kernel(space, labels):
    """dropout 0.3, the same seed: every output of stc_heads_kd(alpha = 0) has the bits of stc_heads's; loss_parts[3] is the soft
    loss of the scores the kernel returned (not 0)"""
    from nbest_amd import hipabi as hb
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, t_top, t_bott, t_fin = _problem(ls, 5, torch.float32, seed=3, saturate=False)
    kw = dict(drop_p=0.3, seed=4321, drop_stream=900)
    got = _kd(dls, hidden, Wh, bh, y, t_top, t_bott, t_fin, 0.0, **kw)
    plain = dict(zip(("top", "bott", "final", "loss_parts", "dcls", "dWh", "dbh"),
                     hb.stc_heads(hidden.reshape(10, H).to(DEV), 2 * H, Wh.to(DEV), bh.to(DEV), dls, y.to(DEV), 5, H, **kw)))
    torch.cuda.synchronize()
    nodrop = _kd(dls, hidden, Wh, bh, y, t_top, t_bott, t_fin, 0.0)
    assert not torch.equal(nodrop["top"], got["top"])                       # the dropout is on
    for k in ("top", "bott", "final", "dcls", "dWh", "dbh"):
        assert torch.equal(got[k], plain[k]), k
    assert torch.equal(got["loss_parts"][:3], plain["loss_parts"][:3]) and plain["loss_parts"][3].item() == 0.0
    d = lambda x: x.double().cpu()
    want = soft_loss(d(got["top"]), d(got["bott"]), d(got["final"]), d(t_top), d(t_bott), d(t_fin), ls.top2bottom).item()
    assert want > 1.0 and abs(got["loss_parts"][3].item() - want) <= 1e-5 * want, (got["loss_parts"][3].item(), want)
    # alpha = 0 without a teacher is the plain kernel too
    none = _kd(dls, hidden, Wh, bh, y, None, None, None, 0.0, **kw)
    for k in none:
        assert torch.equal(none[k], plain[k]), k


@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_one_hot_teacher_is_the_labels(space, labels):
    """t_final = y, t_top = y . B2T, t_bott = the one-hot class (NONE for an empty head): loss_parts[3] = [0] + [1] + [2] and the
    alpha = 1 gradients are the alpha = 0 gradients, to 1e-6 relative, fp32"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, 5, torch.float32, seed=11, saturate=False)
    t_top, t_bott, t_fin = onehot_teacher(y, ls.top2bottom)
    a0 = _kd(dls, hidden, Wh, bh, y, t_top, t_bott, t_fin, 0.0)
    a1 = _kd(dls, hidden, Wh, bh, y, t_top, t_bott, t_fin, 1.0)
    hard = a1["loss_parts"][:3].double().sum().item()
    assert abs(a1["loss_parts"][3].item() - hard) <= 1e-6 * hard, (a1["loss_parts"].tolist(), hard)
    assert torch.equal(a0["loss_parts"], a1["loss_parts"])
    for k in ("dcls", "dWh", "dbh"):
        scale = a0[k].abs().max().item()
        err = (a1[k] - a0[k]).abs().max().item()
        assert scale > 0 and err <= 1e-6 * scale, (k, err, scale)


def _model_teacher(meta, z, seed=17):
    """the golden case's own reference scores, perturbed by a fixed seed, as a teacher"""
    gen = torch.Generator().manual_seed(seed)
    pert = lambda a: (torch.from_numpy(a).float() + 0.2 * (torch.rand(a.shape, generator=gen) - 0.5)).clamp(0.0, 1.0)
    return pert(z["top"]), pert(z["bottoms"]), pert(z["final"])


def test_whole_model_fp32_matches_the_oracle_under_autograd(labels):
    """bert_L2, alpha 0.5: the arena gradients of forward_backward(distill=) against the oracle model with
    (1 - alpha) * hard + alpha * soft (+ MSE) under torch autograd, at the fp32 gradient bars of tests/test_model_gpu.py
    (noise-to-signal 2e-3 per tensor, the STC heads as one fused matrix); two runs give the same bits"""
    from test_model_gpu import _build, _oracle_for
    from conftest import case_inputs
    from oracle import stc
    meta, z = load_case("bert_L2")
    alpha = 0.5
    t_top, t_bott, t_fin = _model_teacher(meta, z)
    cfg, sd, batch = case_inputs(meta, labels)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"] if meta["seg"] else None, trans_seg_ids=t["tseg"])
    _, _, parts = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, stc.bottom2top_matrix(labels.top2bottom),
                                 asr, tr, meta["add_l2"])
    bott = torch.cat([bottoms["lin_%d" % k] for k in labels.multi], dim=1)
    soft = soft_loss(top, bott, final, t_top, t_bott, t_fin, labels.top2bottom)
    total = (1.0 - alpha) * (parts["bottom_bce"] + parts["top_bce"] + parts["ce"]) + alpha * soft
    if meta["add_l2"]:
        total = total + parts["mse"]
    total.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    m, b = _build(meta, labels, torch.float32)
    distill = dict(top=t_top.cuda(), bott=t_bott.cuda(), final=t_fin.cuda(), alpha=alpha)
    runs = []
    for _ in range(2):
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                                 trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"], distill=distill)
        torch.cuda.synchronize()
        runs.append(m.arena.g.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "the distillation step is not bit-reproducible"
    lp = out["loss_parts"].double().cpu()
    hard = (parts["bottom_bce"] + parts["top_bce"] + parts["ce"]).item()
    print("forward_backward(distill=) bert_L2 fp32: hard loss %.6f vs %.6f, soft loss %.6f vs %.6f" % (lp[:3].sum(), hard, lp[3], soft.item()))
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
    print("forward_backward(distill=) bert_L2 fp32: worst gradient noise-to-signal %.3e (%s), bar 2e-3" % worst)
    # the gradient is not the hard one
    plain, _ = _build(meta, labels, torch.float32)
    pout = plain.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                                  trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"])
    assert not torch.equal(plain.arena.g, m.arena.g) and torch.equal(pout["loss_parts"][:3], out["loss_parts"][:3])
    if meta["add_l2"]:                                                  # slot 3 carries the soft loss: the MSE comes back beside it
        assert torch.equal(out["mse"], pout["loss_parts"][3:4])


def test_without_distill_nothing_changes(labels):
    """a forward_backward without ``distill`` after one with it gives the bits of a model that never saw one (dropout on: the step
    seeds advance the same way); need_grad=False with ``distill`` computes the losses only; the forward refuses ``distill``"""
    from test_optim_adam_gpu import _batch, _model
    a, twin = _model(labels, torch.bfloat16, dropout=0.3), _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(a, labels)
    gen = torch.Generator().manual_seed(2)
    t_top, t_bott, t_fin = (x.float().cuda() for x in _teacher_draw(5, labels.top2bottom, gen))
    distill = dict(top=t_top, bott=t_bott, final=t_fin, alpha=0.7)
    out = a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], distill=distill)
    twin.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    assert out["loss_parts"][3].item() > 0 and not torch.equal(a.arena.g, twin.arena.g)
    o1 = a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    o2 = twin.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.g.view(torch.int32), twin.arena.g.view(torch.int32))
    assert a.step_counter == twin.step_counter == 2
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(o1[k], o2[k]), k
    assert "mse" not in o1
    # losses only
    g0 = a.arena.g.clone()
    a.eval()
    ev = a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False, distill=distill)
    torch.cuda.synchronize()
    d = lambda x: x.double().cpu()
    want = soft_loss(d(ev["top"]), d(ev["bott"]), d(ev["final"]), d(t_top), d(t_bott), d(t_fin), labels.top2bottom).item()
    assert abs(ev["loss_parts"][3].item() - want) <= 1e-5 * want and torch.equal(a.arena.g, g0)
    a.train()
    with pytest.raises(RuntimeError, match="distill"):
        a(None, b["ids"], seg_ids=b["seg"], distill=distill)
    for bad in (dict(distill, alpha=1.5), dict(top=t_top, bott=t_bott, alpha=0.5), dict(distill, top=t_top.double())):
        with pytest.raises(ValueError, match="distill"):
            a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], distill=bad)
    with pytest.raises(ValueError, match="distill"):
        a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], distill=dict(distill, top=t_top[:3]))


def test_train_step_with_a_teacher(labels):
    """a 2-layer teacher, a 1-layer student started from its layer 1 (student_state_from_teacher), B 8, S 32, no dropout, alpha 1,
    20 steps on one batch: the soft loss falls, the teacher's weights keep their bits and its mode is eval"""
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import student_state_from_teacher, train_step
    from test_optim_adam_gpu import BERT_LR, LR, _batch, _model
    teacher = _model(labels, torch.bfloat16, layers=2, seed=33)
    student = _model(labels, torch.bfloat16, layers=1, seed=34)
    tsd = {k: v.detach().cpu() for k, v in teacher.state_dict().items()}
    student.load_reference_state(student_state_from_teacher(tsd, [1]))
    w = "bert_encoder.encoder.layer.%d.output.dense.weight"
    assert torch.equal(student.state_dict()[w % 0].cpu(), tsd[w % 1])
    opt = HipBertAdam(student, lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=40)
    b = _batch(student, labels, B=8, S=32)
    before = {n: getattr(teacher.arena, n).clone() for n in ("p", "w16", "g") if getattr(teacher.arena, n) is not None}
    soft = []
    for _ in range(21):
        out = train_step(student, opt, b, teacher=teacher, distill_alpha=1.0)
        soft.append(out["loss_parts"][3:4])
    torch.cuda.synchronize()
    soft = torch.cat(soft).cpu().tolist()
    print("train_step with a teacher: soft loss %.4f -> %.4f over 20 steps" % (soft[0], soft[20]))
    assert soft[20] < soft[0], soft
    assert not teacher.training and teacher.step_counter == 0 and opt.step_count == 21
    for n, x in before.items():
        assert torch.equal(getattr(teacher.arena, n).view(torch.uint8), x.view(torch.uint8)), n


def test_cli_distill_from(tmp_path):
    """a 2-layer teacher for one epoch (12 steps of 2 utterances), then a 1-layer student with --distill_from / --distill_teacher_layers 2 /
    --distill_init_layers 1 / --distill_alpha 0.5 for one epoch: model.pt, the log line and the kd_0.5 directory exist, and
    --testing without the distill flags on a copy of the student's model.pt reproduces its valid F1 line"""
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
    s_args = s_plain + ["--distill_from", t_pt, "--distill_teacher_layers", "2", "--distill_init_layers", "1", "--distill_alpha", "0.5"]
    assert cli.main(s_args) == 0
    d = cli.exp_dir(cli.parse_arguments(s_args))
    assert d.endswith("__kd_0.5") and os.path.isdir(d)
    assert os.path.isfile(os.path.join(d, "model.pt")), "the student's epoch reached no valid F1 above 0"
    log = open(os.path.join(d, "log.train")).read().split("\n")
    assert log[1] == "Distillation: teacher %s (2 layers), alpha 0.5; gradient of (1 - alpha) * hard + alpha * soft, Loss below is the hard loss" % t_pt
    best = [l for l in log if l.startswith("NEW BEST:")]
    f1, acc = re.search(r"valid F1/Acc: ([0-9.]+)/([0-9.]+)", best[-1]).groups()
    # the student started from the teacher's layer 1 and its heads: after one epoch it is no longer that
    teacher_sd, student_sd = torch.load(t_pt, weights_only=True), torch.load(os.path.join(d, "model.pt"), weights_only=True)
    assert set(student_sd) == {k for k in teacher_sd if ".encoder.layer.1." not in k}
    # --testing is refused with the flags; without them the directory has no kd_ part: evaluate a copy of model.pt there
    d_test = cli.exp_dir(cli.parse_arguments(s_plain))
    os.makedirs(d_test)
    shutil.copy(os.path.join(d, "model.pt"), os.path.join(d_test, "model.pt"))
    assert cli.main(s_plain + ["--testing"]) == 0
    line = [l for l in open(os.path.join(d_test, "log.test")).read().split("\n") if l.startswith("[Valid]")][0]
    tf1, tacc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", line).groups()
    assert (tf1, tacc) == (f1, acc), (line, best[-1])
    # a wrong list length is refused before training
    with pytest.raises(SystemExit, match="--distill_init_layers"):
        cli.main(s_plain + ["--distill_from", t_pt, "--distill_teacher_layers", "2", "--distill_init_layers", "0,1"])
    with pytest.raises(SystemExit, match="--distill_init_layers"):
        cli.main(s_plain + ["--distill_from", t_pt, "--distill_teacher_layers", "2", "--distill_init_layers", "2"])
