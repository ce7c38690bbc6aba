"""CPU tests of R-Drop (--rdrop_alpha): the fp64 restatement that tests/test_rdrop_gpu.py holds nbest_stc_heads_rdrop to (its
logarithm-free consistency term against 1/2 [KL + KL] built from log_softmax / logsigmoid, its closed-form d(logits) against torch
autograd), the C ABI surface, the entry point's host-side checks, the command line, trainer.rdrop_batch and model._check_rdrop -
device-free."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi, trainer
from test_distill_cpu import SMALL_SPACE, hard_parts, heads_scores

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]
RD = ["--rdrop_alpha", "1.0", "--dropout", "0.3"]


# ---- the restatement (any float dtype; the GPU tests run it in fp64) ---------------------------------------------------------------
def _head_slices(top2bottom):
    """[(first row, rows)] of every multi-bottom head in the logits' row order (after the n_top top rows)"""
    row, out = len(top2bottom), []
    for t in range(len(top2bottom)):
        n = len(top2bottom[t])
        if n >= 2:
            out.append((row, n))
            row += n
    return out


def consistency(z, zt, top2bottom):
    """sum over the rows of R(row of z, row of zt): the symmetric KL of the model's factorisation in its logarithm-free form,
    sum_t 1/2 (p_t - p'_t)(z_t - z'_t) + (1 / n_heads) sum_k 1/2 sum_j (s_kj - s'_kj)(z_kj - z'_kj)"""
    n_top, heads = len(top2bottom), _head_slices(top2bottom)
    r = 0.5 * ((torch.sigmoid(z[:, :n_top]) - torch.sigmoid(zt[:, :n_top])) * (z[:, :n_top] - zt[:, :n_top])).sum()
    for lo, n in heads:
        a, b = z[:, lo:lo + n], zt[:, lo:lo + n]
        r = r + 0.5 * ((torch.softmax(a, dim=1) - torch.softmax(b, dim=1)) * (a - b)).sum() / len(heads)
    return r


def consistency_kl(z, zt, top2bottom):
    """the same quantity as 1/2 [KL(P || P') + KL(P' || P)] from logsigmoid / log_softmax"""
    n_top, heads = len(top2bottom), _head_slices(top2bottom)

    def kl(a, b):
        at, bt = a[:, :n_top], b[:, :n_top]
        v = (torch.sigmoid(at) * (F.logsigmoid(at) - F.logsigmoid(bt)) + torch.sigmoid(-at) * (F.logsigmoid(-at) - F.logsigmoid(-bt))).sum()
        for lo, n in heads:
            la, lb = F.log_softmax(a[:, lo:lo + n], dim=1), F.log_softmax(b[:, lo:lo + n], dim=1)
            v = v + (la.exp() * (la - lb)).sum() / len(heads)
        return v
    return 0.5 * (kl(z, zt) + kl(zt, z))


def consistency_dz(z, zt, top2bottom):
    """d consistency(z, zt) / dz in closed form - the gradient with respect to the first argument, the rows' own logits (the twin
    rows get theirs from the same expression with the arguments exchanged):
    top t: 1/2 [p (1 - p)(z - z') + (p - p')];  head column i: (1 / n_heads) 1/2 [(s_i - s'_i) + s_i ((z_i - z'_i) - sum_j s_j (z_j - z'_j))]"""
    n_top, heads = len(top2bottom), _head_slices(top2bottom)
    g = torch.zeros_like(z)
    p, pt, d = torch.sigmoid(z[:, :n_top]), torch.sigmoid(zt[:, :n_top]), z[:, :n_top] - zt[:, :n_top]
    g[:, :n_top] = 0.5 * (p * (1 - p) * d + (p - pt))
    for lo, n in heads:
        a, b = z[:, lo:lo + n], zt[:, lo:lo + n]
        s, st, d = torch.softmax(a, dim=1), torch.softmax(b, dim=1), a - b
        g[:, lo:lo + n] = 0.5 * ((s - st) + s * (d - (s * d).sum(dim=1, keepdim=True))) / len(heads)
    return g


def rdrop_reference(cls, Wh, bh, y, alpha, top2bottom):
    """fp64: rows b and b + P of ``cls`` [2 P, H] are twins.  Returns the scores, loss_parts[4] = the three hard terms over the 2 P
    rows and the sum over the P pairs of R, and the gradients of hard + alpha * that with respect to the CLS rows, Wh and bh - what
    nbest_stc_heads_rdrop returns"""
    d = lambda x: x.detach().double().cpu()
    cls, Wh, bh = (d(x).requires_grad_(True) for x in (cls, Wh, bh))
    P = cls.shape[0] // 2
    assert cls.shape[0] == 2 * P
    z = cls @ Wh.t() + bh
    top, bott, final = heads_scores(cls, Wh, bh, top2bottom)
    hard = hard_parts(top, bott, final, d(y), top2bottom)
    r = consistency(z[:P], z[P:], top2bottom)
    (sum(hard) + alpha * r).backward()
    return dict(loss_parts=torch.stack(hard + [r]).detach(), dcls=cls.grad, dWh=Wh.grad, dbh=bh.grad, top=top.detach(),
                bott=bott.detach(), final=final.detach())


def _logits(B, gen, scale=2.0):
    R = len(SMALL_SPACE) + sum(n for _, n in _head_slices(SMALL_SPACE))
    return torch.randn(B, R, generator=gen, dtype=torch.float64) * scale, torch.randn(B, R, generator=gen, dtype=torch.float64) * scale


def test_consistency_is_the_symmetric_kl():
    """random logits, and a row whose logits are +-127 against an ordinary twin: the logarithm-free form equals 1/2 [KL + KL] from
    logsigmoid / log_softmax to 1e-12 relative"""
    gen = torch.Generator().manual_seed(0)
    z, zt = _logits(6, gen)
    a, b = consistency(z, zt, SMALL_SPACE).item(), consistency_kl(z, zt, SMALL_SPACE).item()
    assert a > 0 and abs(a - b) <= 1e-12 * b, (a, b)
    z, zt = _logits(1, gen)
    z[0] = torch.tensor([127.0, -127.0, 127.0, -127.0, 127.0, 127.0, -127.0, 0.0, -127.0, 127.0])
    a, b = consistency(z, zt, SMALL_SPACE).item(), consistency_kl(z, zt, SMALL_SPACE).item()
    assert a > 50 and abs(a - b) <= 1e-12 * b, (a, b)
    # symmetric, and zero for equal twins
    assert consistency(zt, z, SMALL_SPACE).item() == pytest.approx(a, rel=1e-14)
    assert consistency(z, z.clone(), SMALL_SPACE).item() == 0.0


def test_closed_form_dz_is_autograd():
    gen = torch.Generator().manual_seed(1)
    z, zt = _logits(5, gen)
    z[4, :3] = torch.tensor([40.0, -40.0, 3.0])
    for a, b in ((z, zt), (zt, z)):
        a = a.clone().requires_grad_(True)
        consistency(a, b, SMALL_SPACE).backward()
        want, got = a.grad, consistency_dz(a.detach(), b, SMALL_SPACE)
        assert (got - want).abs().max().item() <= 1e-10 * max(want.abs().max().item(), 1.0)
    assert consistency_dz(z, z.clone(), SMALL_SPACE).abs().max().item() == 0.0


def test_reference_gradients_are_the_chain_rule_of_the_closed_form():
    """rdrop_reference (autograd through the heads) against dz_R pushed through the linear layer by hand: both twins get a gradient"""
    gen = torch.Generator().manual_seed(2)
    R = len(SMALL_SPACE) + sum(n for _, n in _head_slices(SMALL_SPACE))
    cls = torch.randn(4, 6, generator=gen, dtype=torch.float64)
    Wh, bh = torch.randn(R, 6, generator=gen, dtype=torch.float64) * 0.5, torch.randn(R, generator=gen, dtype=torch.float64) * 0.5
    y = torch.zeros(4, 8, dtype=torch.float64)
    y[0, 0] = y[1, 4] = y[2, 1] = 1
    a0, a2 = (rdrop_reference(cls, Wh, bh, y, al, SMALL_SPACE) for al in (0.0, 2.0))
    assert torch.equal(a0["loss_parts"], a2["loss_parts"]) and a0["loss_parts"][3].item() > 0
    z = cls @ Wh.t() + bh
    dz = torch.cat([consistency_dz(z[:2], z[2:], SMALL_SPACE), consistency_dz(z[2:], z[:2], SMALL_SPACE)])
    assert torch.allclose(a2["dcls"] - a0["dcls"], 2.0 * dz @ Wh, rtol=1e-10, atol=1e-13)
    assert torch.allclose(a2["dWh"] - a0["dWh"], 2.0 * dz.t() @ cls, rtol=1e-10, atol=1e-13)
    assert torch.allclose(a2["dbh"] - a0["dbh"], 2.0 * dz.sum(0), rtol=1e-10, atol=1e-13)
    assert (a2["dcls"] - a0["dcls"])[2:].abs().max().item() > 0


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hipabi_binds_the_entry_point():
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    m = re.search(r"int nbest_stc_heads_rdrop\(([^;]*)\);", hdr)
    assert m, "include/nbest_hip.h does not declare nbest_stc_heads_rdrop"
    decl = " ".join(m.group(1).split())
    assert "float alpha" in decl and "int B2" in decl
    plain = " ".join(re.search(r"int nbest_stc_heads\(([^;]*)\);", hdr).group(1).split())
    assert len(decl.split(",")) == len(plain.split(",")) + 1
    assert "1/2 (p_t - p'_t)(z_t - z'_t)" in hdr                       # the definition of the loss sits with the prototype
    assert "nbest_stc_heads_rdrop" in hipabi.EXPORTS
    assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), "nbest_stc_heads_rdrop")
    L = hipabi.lib()
    assert len(L.nbest_stc_heads_rdrop.argtypes) == len(L.nbest_stc_heads.argtypes) + 1
    assert L.nbest_stc_heads_rdrop.argtypes[6] is ctypes.c_float
    assert hasattr(hipabi, "stc_heads_rdrop")


def test_entry_point_checks_alpha_and_the_batch_on_the_host():
    """a negative or non-finite alpha, an odd B2: an error code and a message before anything touches a device"""
    L = hipabi.lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    ls = hipabi.LabelSpaceC(3, 8, 10, 1 << 20, 1 << 20, 1 << 20)

    def call(alpha, B2):
        return L.nbest_stc_heads_rdrop(fake, 4, fake, fake, ctypes.byref(ls), fake, alpha, fake, fake, fake, fake, fake, fake, fake,
                                       B2, 4, hipabi.F32, 1, 0, 0.0, 0, 0, fake, 1 << 20, null)
    for args in ((-0.1, 2), (float("nan"), 2), (float("inf"), 2), (1.0, 3), (1.0, 1), (1.0, 0)):
        assert call(*args) < 0, args
        assert "stc_heads_rdrop" in hipabi.last_error(), args


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_default_and_combinations():
    assert cli.parse_arguments(BASE).rdrop_alpha is None
    assert cli.parse_arguments(BASE + RD).rdrop_alpha == 1.0
    assert cli.parse_arguments(BASE + ["--rdrop_alpha", "4"]).rdrop_alpha == 4.0       # --bert_dropout defaults to 0.1
    for optim in (["--optim_choice", "bertadam"], ["--optim_choice", "adam"], ["--optim_choice", "adamw", "--restated_adamw"]):
        opt = cli.parse_arguments(BASE + RD + optim + ["--ema_decay", "0.9", "--freeze_layers", "1", "--freeze_embeddings", "--resume",
                                                       "--dtype", "fp8w", "--add_l2_loss"])
        assert opt.rdrop_alpha == 1.0 and opt.ema_decay == 0.9


def test_cli_exp_dir_moves_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert plain.endswith("__cls_stc") and "rdrop" not in plain
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--rdrop_alpha", "1.0"])) == plain + "__rdrop_1.0"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--rdrop_alpha", "0.5", "--ema_decay", "0.9", "--freeze_layers", "1"])) == \
        plain + "__fz_none_1__ema_0.9__rdrop_0.5"
    # the names of the other flags stay as they were
    kd = cli.exp_dir(cli.parse_arguments(BASE + ["--distill_from", "t.pt", "--distill_temperature", "2.0"]))
    assert kd == plain + "__kd_0.5__kdT_2.0"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--ema_decay", "0.9"])) == plain + "__ema_0.9"


def test_cli_refusals(tmp_path, monkeypatch, capsys):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    for bad, word in ((RD + ["--testing"], "--testing"), (RD + ["--predict", str(src)], "--predict"),
                      (RD + ["--head_importance", str(tmp_path / "imp.json")], "--head_importance"),
                      (RD + ["--distill_from", "t.pt"], "--distill_from"),
                      (["--rdrop_alpha", "0"], "--rdrop_alpha"), (["--rdrop_alpha", "-1"], "--rdrop_alpha"),
                      (["--rdrop_alpha", "nan"], "--rdrop_alpha"), (["--rdrop_alpha", "inf"], "--rdrop_alpha"),
                      (["--rdrop_alpha", "1.0", "--dropout", "0", "--bert_dropout", "0"], "identical")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        assert word in capsys.readouterr().err, bad
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + RD)
    assert "data parallelism is not built" in capsys.readouterr().err
    assert cli.parse_arguments(BASE).rdrop_alpha is None                # ... and fine without the flag
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.parse_arguments(BASE + ["--rdrop_alpha", "1.0", "--dropout", "0.3", "--bert_dropout", "0"]).rdrop_alpha == 1.0


# ---- trainer and model -------------------------------------------------------------------------------------------------------------
def test_rdrop_batch_doubles_the_rows_and_rebuilds_the_perm():
    gen = torch.Generator().manual_seed(3)
    ids, tids = torch.randint(0, 7, (3, 5), generator=gen), torch.randint(0, 4, (3, 2), generator=gen)     # few ids: many ties
    batch = dict(ids=ids, seg=torch.randint(0, 2, (3, 5), generator=gen), labels=torch.rand(3, 8, generator=gen), tids=tids,
                 tseg=torch.zeros(3, 2, dtype=torch.long), word_rows=torch.arange(7), tok_perm=trainer.token_perm(ids),
                 ttok_perm=trainer.token_perm(tids))
    before = {k: v.clone() for k, v in batch.items()}
    out = trainer.rdrop_batch(batch)
    for k in ("ids", "seg", "labels", "tids", "tseg"):
        assert out[k].shape[0] == 6 and torch.equal(out[k][:3], batch[k]) and torch.equal(out[k][3:], batch[k]), k
    assert out["word_rows"] is batch["word_rows"]
    for k, src in (("tok_perm", "ids"), ("ttok_perm", "tids")):
        want = torch.from_numpy(trainer.token_perm(out[src], as_numpy=True))
        assert out[k].dtype == torch.int32 and out[k].shape == (out[src].numel(),) and torch.equal(out[k], want), k
        flat = out[src].reshape(-1)[out[k].long()]
        assert bool((flat[1:] >= flat[:-1]).all())                      # sorted by word id ...
        ties = flat[1:] == flat[:-1]
        assert bool((out[k][1:][ties] > out[k][:-1][ties]).all())       # ... ties in ascending token index
    assert all(torch.equal(batch[k], before[k]) for k in batch), "rdrop_batch modified its argument"
    # a batch without transcripts or segment ids
    small = trainer.rdrop_batch(dict(ids=ids, labels=batch["labels"]))
    assert set(small) == {"ids", "labels", "tok_perm"} and small["ids"].shape == (6, 5)


def test_rdrop_hard_loss_parts_halves_the_hard_terms():
    lp = torch.tensor([2.0, 4.0, 6.0, 9.0])
    assert trainer.rdrop_hard_loss_parts(dict(loss_parts=lp)).tolist() == [1.0, 2.0, 3.0, 0.0]
    assert trainer.rdrop_hard_loss_parts(dict(loss_parts=lp, mse=torch.tensor([0.25]))).tolist() == [1.0, 2.0, 3.0, 0.25]
    assert lp.tolist() == [2.0, 4.0, 6.0, 9.0]


def test_check_rdrop():
    from nbest_amd.model import _check_rdrop
    assert _check_rdrop(dict(alpha=1), 4) == dict(alpha=1.0) and _check_rdrop(dict(alpha=0.0), 2) == dict(alpha=0.0)
    for bad, B, distill in ((dict(alpha=1.0), 5, None), (dict(alpha=1.0), 1, None), (dict(alpha=1.0), 0, None),
                            (dict(alpha=-0.5), 4, None), (dict(alpha=float("nan")), 4, None), (dict(alpha=float("inf")), 4, None),
                            (dict(alpha="x"), 4, None), (dict(), 4, None), (dict(alpha=1.0, beta=2.0), 4, None), (1.0, 4, None),
                            (dict(alpha=1.0), 4, dict(top=None, bott=None, final=None, alpha=0.5))):
        with pytest.raises(ValueError, match="rdrop"):
            _check_rdrop(bad, B, distill)


def test_train_step_refuses_a_teacher_before_touching_anything():
    with pytest.raises(ValueError, match="rdrop"):
        trainer.train_step(None, None, dict(ids=torch.zeros(2, 3, dtype=torch.long)), teacher=object(), rdrop_alpha=1.0)
