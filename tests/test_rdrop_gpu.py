"""GPU: R-Drop.  nbest_stc_heads_rdrop against the fp64 restatement of tests/test_rdrop_cpu.py (scores, the four loss parts and the
three gradients), its alpha = 0 / equal-twins / swap / repeat identities, forward_backward(rdrop=) on a whole fp32 model against the
oracle under torch autograd, the untouched path without it, train_step(rdrop_alpha=) and --rdrop_alpha through the CLI."""
import os
import re
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_distill_gpu import H, _problem, _ratio, _space
from test_rdrop_cpu import consistency, rdrop_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = ("top", "bott", "final", "loss_parts", "dcls", "dWh", "dbh")


def _call(fn, dls, hidden, Wh, bh, y, *alpha, **kw):
    """``hidden`` [B, 2, H]: the CLS rows at row stride 2 H"""
    B = hidden.shape[0]
    c = lambda x: x.to(DEV).contiguous()
    out = fn(c(hidden.reshape(B * 2, H)), 2 * H, c(Wh), c(bh), dls, c(y), *alpha, B, H, **kw)
    torch.cuda.synchronize()
    return dict(zip(KEYS, out))


def _rd(dls, hidden, Wh, bh, y, alpha, **kw):
    from nbest_amd import hipabi as hb
    return _call(hb.stc_heads_rdrop, dls, hidden, Wh, bh, y, alpha, **kw)


def _plain(dls, hidden, Wh, bh, y, **kw):
    from nbest_amd import hipabi as hb
    return _call(hb.stc_heads, dls, hidden, Wh, bh, y, **kw)


def _same_bits(a, b, keys=KEYS):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("alpha", [0.3, 4.0])
@pytest.mark.parametrize("B2", [2, 10])
@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_kernel_matches_the_fp64_restatement(space, B2, alpha, dtype, labels):
    """scores, loss_parts[0..3], dcls, dWh and dbh of nbest_stc_heads_rdrop against the restatement in fp64 on the same (fp32 or bf16)
    CLS rows, twins drawn independently, dropout 0, at the project's bars for these quantities (scores and losses 1e-5, gradients
    1e-4 of the tensor's largest element).  B2 = 10 carries the saturated row (row 9: two top logits near +-115); its twin (row 4)
    is an ordinary draw."""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, B2, dtype, seed=7 + B2, saturate=B2 > 2)
    got = _rd(dls, hidden, Wh, bh, y, alpha)
    ref = rdrop_reference(hidden[:, 0, :].float(), Wh, bh, y, alpha, ls.top2bottom)
    if B2 > 2:
        assert got["top"][B2 - 1, 0].item() == 1.0 and got["top"][B2 - 1, 1].item() == 0.0, "the saturated row does not saturate"
        assert 0.0 < got["top"][B2 // 2 - 1, 0].item() < 1.0
    worst = {}
    for k in ("top", "bott", "final"):
        _ratio(k, got[k], ref[k], 1e-5, worst)
    _ratio("loss_parts", got["loss_parts"], ref["loss_parts"], 1e-5, worst)
    _ratio("consistency", got["loss_parts"][3:], ref["loss_parts"][3:], 1e-5, worst)
    for k in ("dcls", "dWh", "dbh"):
        _ratio(k, got[k], ref[k], 1e-4, worst)
    print("stc_heads_rdrop %s B2=%d alpha=%g %s: consistency %.6f, worst error / bar %s" % (
        space, B2, alpha, str(dtype)[6:], got["loss_parts"][3].item(), ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def _consistency_from_scores(top, bott, ls):
    """fp64, from the scores the kernel returned: 1/2 (p - p')(logit p - logit p') and (1 / n_heads) 1/2 (s - s')(log s - log s')"""
    P = top.shape[0] // 2
    p, q = top[:P].double().cpu(), top[P:].double().cpu()
    s, t = bott[:P].double().cpu(), bott[P:].double().cpu()
    logit = lambda x: torch.log(x) - torch.log1p(-x)
    return (0.5 * ((p - q) * (logit(p) - logit(q))).sum() + 0.5 * ((s - t) * (torch.log(s) - torch.log(t))).sum() / len(ls.multi)).item()


@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_alpha_zero_is_the_plain_kernel(space, labels):
    """(a) dropout 0.3, the same seed: every output of stc_heads_rdrop(alpha = 0) has the bits of stc_heads on the same 2 P rows;
    loss_parts[3] is positive and is the consistency sum of the scores the kernel returned (1e-5 relative)"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, 10, torch.float32, seed=3, saturate=False)
    kw = dict(drop_p=0.3, seed=4321, drop_stream=900)
    got, plain = _rd(dls, hidden, Wh, bh, y, 0.0, **kw), _plain(dls, hidden, Wh, bh, y, **kw)
    assert not torch.equal(_rd(dls, hidden, Wh, bh, y, 0.0)["top"], got["top"])                  # the dropout is on
    _same_bits(got, plain, ("top", "bott", "final", "dcls", "dWh", "dbh"))
    assert torch.equal(got["loss_parts"][:3], plain["loss_parts"][:3]) and plain["loss_parts"][3].item() == 0.0
    want = _consistency_from_scores(got["top"], got["bott"], ls)
    assert want > 0 and abs(got["loss_parts"][3].item() - want) <= 1e-5 * want, (got["loss_parts"][3].item(), want)


@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_equal_twins(space, labels):
    """(b) duplicated rows, dropout 0, alpha 4: loss_parts[3] == 0.0 and every output has the plain kernel's bits.
    (c) duplicated rows, dropout 0.3: the twins run under different bits - loss_parts[3] > 0 and dcls differs from alpha = 0"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, 5, torch.float32, seed=5, saturate=True)
    hidden, y = torch.cat([hidden, hidden]), torch.cat([y, y])
    got, plain = _rd(dls, hidden, Wh, bh, y, 4.0), _plain(dls, hidden, Wh, bh, y)
    assert got["loss_parts"][3].item() == 0.0
    _same_bits(got, plain)
    kw = dict(drop_p=0.3, seed=99, drop_stream=900)
    on, off = _rd(dls, hidden, Wh, bh, y, 4.0, **kw), _rd(dls, hidden, Wh, bh, y, 0.0, **kw)
    assert on["loss_parts"][3].item() > 0 and torch.equal(on["loss_parts"], off["loss_parts"])
    assert not torch.equal(on["top"][:5], on["top"][5:])                                           # independent masks
    assert not torch.equal(on["dcls"], off["dcls"]) and not torch.equal(on["dWh"], off["dWh"])
    _same_bits(on, off, ("top", "bott", "final"))


@pytest.mark.parametrize("space", ["shipped", "wide"])
def test_swapping_the_halves_and_repeating(space, labels):
    """(d) dropout 0: the halves of the input swapped - top, bott, final and dcls swap row-wise, bit for bit, loss_parts[3] stays
    (1e-6 relative: the pairs' halves are summed in another order).  (e) two identical calls (dropout on) give identical bits"""
    ls = _space(space, labels)
    dls, hidden, Wh, bh, y, _, _, _ = _problem(ls, 10, torch.bfloat16, seed=13, saturate=True)
    sw = lambda x: torch.cat([x[5:], x[:5]])
    a, b = _rd(dls, hidden, Wh, bh, y, 1.5), _rd(dls, sw(hidden), Wh, bh, sw(y), 1.5)
    for k in ("top", "bott", "final", "dcls"):
        assert torch.equal(sw(a[k]), b[k]), k
    la, lb = a["loss_parts"][3].item(), b["loss_parts"][3].item()
    assert la > 0 and abs(la - lb) <= 1e-6 * la, (la, lb)
    kw = dict(drop_p=0.3, seed=7, drop_stream=900)
    _same_bits(_rd(dls, hidden, Wh, bh, y, 1.5, **kw), _rd(dls, hidden, Wh, bh, y, 1.5, **kw))


def test_whole_model_fp32_matches_the_oracle_under_autograd(labels):
    """bert_L2, alpha 1, dropout 0: rows P .. 2 P - 1 are the case's utterances rolled by one (the twins need not be copies).  The
    arena gradients of forward_backward(rdrop=) against the oracle model with the hard loss of the 2 P rows + alpha * R (+ MSE)
    under torch autograd - the logits from forward hooks on the heads' linear layers - at the fp32 gradient bars of
    tests/test_model_gpu.py (noise-to-signal 2e-3 per tensor, the STC heads as one fused matrix, key bias skipped); losses 1e-4
    relative; two runs give the same bits"""
    from test_model_gpu import _build, _oracle_for
    from conftest import case_inputs
    from oracle import stc
    meta, _ = load_case("bert_L2")
    alpha = 1.0
    cfg, sd, batch = case_inputs(meta, labels)
    om = _oracle_for(cfg, sd, labels)
    dbl = lambda x: torch.cat([x, torch.roll(x, 1, 0)])
    t = {k: dbl(torch.from_numpy(v)) for k, v in batch.items()}
    P = t["ids"].shape[0] // 2
    caught = {}
    hooks = [om.clf.top_linear_layer.register_forward_hook(lambda mod, i, o: caught.__setitem__("top", o))]
    for k, lin in om.clf.linear_layers.items():
        hooks.append(lin.register_forward_hook(lambda mod, i, o, k=k: caught.__setitem__(k, o)))
    top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"] if meta["seg"] else None, trans_seg_ids=t["tseg"])
    for h in hooks:
        h.remove()
    _, _, parts = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, stc.bottom2top_matrix(labels.top2bottom),
                                 asr, tr, meta["add_l2"])
    z = torch.cat([caught["top"]] + [caught["lin_%d" % k] for k in labels.multi], dim=1)
    r = consistency(z[:P], z[P:], labels.top2bottom)
    hard = parts["bottom_bce"] + parts["top_bce"] + parts["ce"]
    total = hard + alpha * r
    if meta["add_l2"]:
        total = total + parts["mse"]
    total.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    m, b = _build(meta, labels, torch.float32)
    b = {k: dbl(v) for k, v in b.items()}
    step = lambda mm, **kw: mm.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                                                trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"], **kw)
    runs = []
    for _ in range(2):
        out = step(m, rdrop=dict(alpha=alpha))
        torch.cuda.synchronize()
        runs.append(m.arena.g.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "the R-Drop step is not bit-reproducible"
    assert out["top"].shape[0] == 2 * P
    lp = out["loss_parts"].double().cpu()
    print("forward_backward(rdrop=) bert_L2 fp32: hard loss %.6f vs %.6f, consistency %.6f vs %.6f" % (lp[:3].sum(), hard.item(), lp[3], r.item()))
    assert abs(lp[:3].sum().item() - hard.item()) <= 1e-4 * hard.item() and abs(lp[3].item() - r.item()) <= 1e-4 * r.item()
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
    print("forward_backward(rdrop=) bert_L2 fp32: worst gradient noise-to-signal %.3e (%s), bar 2e-3" % worst)
    # the gradient is not the hard one, the hard terms are; slot 3 carries the consistency sum: the MSE comes back beside it
    plain, _ = _build(meta, labels, torch.float32)
    pout = step(plain)
    assert not torch.equal(plain.arena.g, m.arena.g) and torch.equal(pout["loss_parts"][:3], out["loss_parts"][:3])
    if meta["add_l2"]:
        assert torch.equal(out["mse"], pout["loss_parts"][3:4])


def test_without_rdrop_nothing_changes(labels):
    """a forward_backward without ``rdrop`` after one with it gives the bits of a model that never saw one (dropout on: the step
    seeds advance the same way); need_grad=False with ``rdrop`` computes the losses only; bad arguments raise before anything runs"""
    from test_optim_adam_gpu import _batch, _model
    a, twin = _model(labels, torch.bfloat16, dropout=0.3), _model(labels, torch.bfloat16, dropout=0.3)
    b = _batch(a, labels, B=6)
    rd = dict(alpha=0.7)
    out = a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], rdrop=rd)
    tout = twin.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    assert out["loss_parts"][3].item() > 0 and tout["loss_parts"][3].item() == 0.0 and not torch.equal(a.arena.g, twin.arena.g)
    for k in ("top", "bott", "final"):
        assert torch.equal(out[k], tout[k]), k
    assert torch.equal(out["loss_parts"][:3], tout["loss_parts"][:3])
    kw = dict(seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    o1, o2 = a.forward_backward(b["ids"], b["labels"], **kw), twin.forward_backward(b["ids"], b["labels"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.g.view(torch.int32), twin.arena.g.view(torch.int32))
    assert a.step_counter == twin.step_counter == 2
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(o1[k], o2[k]), k
    assert "mse" not in o1
    # with the MSE: slot 3 stays the consistency sum
    o3 = a.forward_backward(b["ids"], b["labels"], rdrop=rd, **kw)
    assert o3["mse"].shape == (1,) and o3["mse"].item() > 0 and o3["loss_parts"][3].item() > 0
    # losses only (eval: no dropout anywhere, but the twins are different utterances here)
    g0 = a.arena.g.clone()
    a.eval()
    ev = a.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False, rdrop=rd)
    torch.cuda.synchronize()
    want = _consistency_from_scores(ev["top"], ev["bott"], labels)
    assert want > 0 and abs(ev["loss_parts"][3].item() - want) <= 1e-5 * want and torch.equal(a.arena.g, g0)
    a.train()
    distill = dict(logits=torch.zeros(6, a.dls.n_rows, device=DEV), alpha=0.5, temperature=2.0)
    steps = a.step_counter
    for ids, kwargs in ((b["ids"][:5], dict(rdrop=rd)), (b["ids"], dict(rdrop=dict(alpha=-1.0))),
                        (b["ids"], dict(rdrop=dict(alpha=float("nan")))), (b["ids"], dict(rdrop=rd, distill=distill))):
        with pytest.raises(ValueError, match="rdrop"):
            a.forward_backward(ids, b["labels"][:ids.shape[0]], seg_ids=b["seg"][:ids.shape[0]], **kwargs)
    assert a.step_counter == steps and torch.equal(a.arena.g, g0)


def test_train_step_with_rdrop(labels):
    """a 1-layer bf16 model, B 8, S 32, dropout 0.3 / 0.1, alpha 1, 20 steps on one batch: the consistency term is positive at step
    0, the hard loss falls, the optimizer stepped once per call and the returned tensors have 16 rows"""
    from nbest_amd.optim import HipBertAdam
    from nbest_amd.trainer import train_step
    from test_optim_adam_gpu import BERT_LR, LR, _batch, _model
    m = _model(labels, torch.bfloat16, layers=1, seed=34, dropout=0.3)
    opt = HipBertAdam(m, lr=LR, bert_lr=BERT_LR, warmup=0.1, t_total=40)
    b = _batch(m, labels, B=8, S=32)
    parts = []
    for _ in range(21):
        out = train_step(m, opt, b, rdrop_alpha=1.0)
        parts.append(out["loss_parts"].clone())
    torch.cuda.synchronize()
    parts = torch.stack(parts).double().cpu()
    hard = parts[:, :3].sum(dim=1).tolist()
    print("train_step(rdrop_alpha=1): hard loss %.4f -> %.4f, consistency %.4f -> %.4f over 20 steps" % (hard[0], hard[20], parts[0, 3], parts[20, 3]))
    assert parts[0, 3].item() > 0 and hard[20] < hard[0], (hard, parts[:, 3].tolist())
    assert opt.step_count == 21
    for k, n in (("top", labels.n_top), ("final", labels.n_bottom)):
        assert out[k].shape == (16, n), k
    assert out["bott"].shape[0] == 16 and out["asr_cls"].shape[0] == 16 and b["ids"].shape[0] == 8
    with pytest.raises(ValueError, match="rdrop"):
        train_step(m, opt, b, teacher=m, rdrop_alpha=1.0)
    assert opt.step_count == 21


def test_cli_rdrop_alpha(tmp_path):
    """one epoch on valid_head.txt (12 steps of 2 utterances, 4 rows each) with --rdrop_alpha 1.0: the __rdrop_1.0 directory, the
    log line and a parsable [Train] line exist; --testing is refused with the flag and, without it, reproduces the valid F1 line on
    a copy of model.pt in the plain-named directory"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    plain = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
             "--bert_dropout", "0.1", "--optim_choice", "bertadam", "--lr", "1e-2", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
             "--batchSize", "2", "--max_epoch", "1", "--experiment", str(tmp_path / "exp"), "--pre_trained_model", "bert",
             "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
             "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "1", "--n_best", "5"]
    args = plain + ["--rdrop_alpha", "1.0", "--resume"]
    assert cli.main(args) == 0
    d = cli.exp_dir(cli.parse_arguments(args))
    assert d.endswith("__rdrop_1.0") and os.path.isdir(d)
    pt = os.path.join(d, "model.pt")
    if not os.path.isfile(pt):         # written on a NEW BEST valid F1 only: otherwise the epoch's weights
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], pt)
    log = open(os.path.join(d, "log.train")).read().split("\n")
    assert sum(l.startswith("R-Drop: alpha 1.0;") for l in log) == 1
    train = [l for l in log if l.startswith("[Train]\tEpoch: 00")]
    assert len(train) == 1
    loss, f1 = re.search(r"Loss: ([0-9.]+)\t\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)", train[0]).groups()
    assert 0.0 < float(loss) < 1e4 and 0.0 <= float(f1) <= 100.0
    valid = [l for l in log if l.startswith("[Valid]\tEpoch: 00")][0]
    f1, acc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", valid).groups()
    with pytest.raises(SystemExit):
        cli.main(args + ["--testing"])
    d_test = cli.exp_dir(cli.parse_arguments(plain))
    assert d_test != d and d == d_test + "__rdrop_1.0"
    os.makedirs(d_test)
    shutil.copy(pt, os.path.join(d_test, "model.pt"))
    assert cli.main(plain + ["--testing"]) == 0
    line = [l for l in open(os.path.join(d_test, "log.test")).read().split("\n") if l.startswith("[Valid]")][0]
    tf1, tacc = re.search(r"\(p/r/f\): \([0-9.]+/[0-9.]+/([0-9.]+)\)\tAcc: ([0-9.]+)", line).groups()
    assert (tf1, tacc) == (f1, acc), (line, valid)
