"""CPU tests of distillation at a temperature (--distill_temperature): the fp64 restatement of the tempered soft loss that
tests/test_distill_temperature_gpu.py holds nbest_stc_heads_kd_t to (gradcheck, T = 1 is the probability form, T changes the
gradient), the C ABI and its binding for nbest_stc_heads_kd_t and nbest_stc_heads_logits, their host-side argument checks, and
the command-line surface - device-free."""
import ctypes
import os
import re

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi
from test_distill_cpu import BASE, KD, SMALL_SPACE, _small_problem, hard_parts, heads_scores, kd_reference, soft_loss


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def scores_from_logits(z, top2bottom):
    """top / bott / final from a row of R logits: heads_scores with the identity as the head matrix"""
    R = z.shape[1]
    return heads_scores(z, torch.eye(R, dtype=z.dtype), torch.zeros(R, dtype=z.dtype), top2bottom)


def soft_loss_t(cls, Wh, bh, t_logits, T, top2bottom):
    """T^2 x the soft loss of the tempered scores.  The logits are linear in the head parameters, so the student's tempered scores
    are heads_scores(cls, Wh / T, bh / T); the teacher's come from t_logits / T"""
    return T * T * soft_loss(*heads_scores(cls, Wh / T, bh / T, top2bottom), *scores_from_logits(t_logits / T, top2bottom), top2bottom)


def kd_t_reference(cls, Wh, bh, y, t_logits, alpha, T, top2bottom):
    """fp64: loss_parts[4] = kd_reference's three hard terms and soft_T, and the gradients of (1 - alpha) * hard + alpha * soft_T
    with respect to the CLS rows, Wh and bh - what nbest_stc_heads_kd_t returns (top / bott / final: the T = 1 scores)"""
    d = lambda x: x.detach().double().cpu()
    cls, Wh, bh = (d(x).requires_grad_(True) for x in (cls, Wh, bh))
    top, bott, final = heads_scores(cls, Wh, bh, top2bottom)
    hard = hard_parts(top, bott, final, d(y), top2bottom)
    soft = soft_loss_t(cls, Wh, bh, d(t_logits), float(T), top2bottom)
    ((1.0 - alpha) * sum(hard) + alpha * soft).backward()
    return dict(loss_parts=torch.stack(hard + [soft]).detach(), dcls=cls.grad, dWh=Wh.grad, dbh=bh.grad,
                top=top.detach(), bott=bott.detach(), final=final.detach())


def _teacher(cls, R, gen, scale=1.0):
    """a random teacher on the same CLS rows: its head matrix, bias and logits"""
    Wt = torch.randn(R, cls.shape[1], generator=gen, dtype=torch.float64) * scale
    bt = torch.randn(R, generator=gen, dtype=torch.float64) * scale
    return Wt, bt, cls @ Wt.t() + bt


def _labels(B):
    y = torch.zeros(B, 8, dtype=torch.float64)
    y[0, 0] = y[0, 4] = 1
    y[1, 1] = 1
    if B > 2:
        y[2, 7] = y[2, 2] = 1
    return y


def test_tempered_soft_loss_gradcheck():
    """d(soft_T) / d(CLS rows, Wh, bh) at T = 2 on the 3-top label space: a single-bottom top, a 2-column head, a 5-column head"""
    cls, Wh, bh, gen = _small_problem()
    _, _, tz = _teacher(cls, Wh.shape[0], gen)

    def f(cls, Wh, bh):
        return soft_loss_t(cls, Wh, bh, tz, 2.0, SMALL_SPACE)
    assert torch.autograd.gradcheck(f, tuple(x.clone().requires_grad_(True) for x in (cls, Wh, bh)), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_temperature_one_is_the_probability_form():
    """t_logits from a random teacher, T = 1: the four loss parts and the three gradients are kd_reference's, fed that teacher's
    fp64 scores"""
    cls, Wh, bh, gen = _small_problem(B=4)
    Wt, bt, tz = _teacher(cls, Wh.shape[0], gen)
    y = _labels(4)
    for alpha in (0.3, 1.0):
        a = kd_t_reference(cls, Wh, bh, y, tz, alpha, 1.0, SMALL_SPACE)
        b = kd_reference(cls, Wh, bh, y, *heads_scores(cls, Wt, bt, SMALL_SPACE), alpha, SMALL_SPACE)
        for k in ("loss_parts", "dcls", "dWh", "dbh", "top", "bott", "final"):
            assert torch.allclose(a[k], b[k], rtol=1e-12, atol=1e-14), (alpha, k)


def test_temperature_changes_the_gradient():
    """a fixed draw (seed 0, teacher logits of scale 3): the alpha = 1 gradient at T = 4 differs from the one at T = 1 by more than
    1e-3 of its size, and the hard terms and scores do not move"""
    cls, Wh, bh, gen = _small_problem(B=4)
    _, _, tz = _teacher(cls, Wh.shape[0], gen, scale=3.0)
    y = _labels(4)
    a = kd_t_reference(cls, Wh, bh, y, tz, 1.0, 1.0, SMALL_SPACE)
    b = kd_t_reference(cls, Wh, bh, y, tz, 1.0, 4.0, SMALL_SPACE)
    for k in ("dcls", "dWh", "dbh"):
        rel = ((a[k] - b[k]).norm() / a[k].norm()).item()
        assert rel > 1e-3, (k, rel)
    assert torch.equal(a["loss_parts"][:3], b["loss_parts"][:3]) and torch.equal(a["top"], b["top"])
    assert abs(a["loss_parts"][3].item() - b["loss_parts"][3].item()) > 1e-3 * a["loss_parts"][3].item()


def test_alpha_zero_gradient_is_the_hard_one():
    cls, Wh, bh, gen = _small_problem(B=4)
    Wt, bt, tz = _teacher(cls, Wh.shape[0], gen)
    y = _labels(4)
    a = kd_t_reference(cls, Wh, bh, y, tz, 0.0, 3.0, SMALL_SPACE)
    b = kd_reference(cls, Wh, bh, y, *heads_scores(cls, Wt, bt, SMALL_SPACE), 0.0, SMALL_SPACE)
    for k in ("dcls", "dWh", "dbh"):
        assert torch.allclose(a[k], b[k], rtol=1e-12, atol=1e-14), k
    assert a["loss_parts"][3].item() > 0


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def _decl(hdr, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, "include/nbest_hip.h does not declare %s" % name
    return " ".join(m.group(1).split())


def test_header_declares_and_hipabi_binds_the_entry_points():
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    plain = _decl(hdr, "nbest_stc_heads")
    decl = _decl(hdr, "nbest_stc_heads_kd_t")
    for arg in ("const float* t_logits", "float alpha", "float temperature"):
        assert arg in decl, arg
    assert len(decl.split(",")) == len(plain.split(",")) + 3
    lg = _decl(hdr, "nbest_stc_heads_logits")
    for arg in ("const void* hidden", "int64_t cls_stride", "const nbest_label_space* ls", "float* logits", "nbest_stream_t stream"):
        assert arg in lg, arg
    assert len(lg.split(",")) == 10
    raw = ctypes.CDLL(hipabi.LIB_PATH)
    L = hipabi.lib()
    for name in ("nbest_stc_heads_kd_t", "nbest_stc_heads_logits"):
        assert name in hipabi.EXPORTS and hasattr(raw, name), name
    assert len(L.nbest_stc_heads_kd_t.argtypes) == len(L.nbest_stc_heads.argtypes) + 3
    assert L.nbest_stc_heads_kd_t.argtypes[7] is ctypes.c_float and L.nbest_stc_heads_kd_t.argtypes[8] is ctypes.c_float
    assert L.nbest_stc_heads_kd_t.argtypes[6] is ctypes.c_void_p and L.nbest_stc_heads_kd_t.argtypes[9] is ctypes.c_void_p
    assert len(L.nbest_stc_heads_logits.argtypes) == 10
    assert hasattr(hipabi, "stc_heads_kd_t") and hasattr(hipabi, "stc_heads_logits")
    # the formulas are in the K7 comment block
    for word in ("K7 kd_t", "K7 logits", "T^2"):
        assert word in hdr, word


def test_entry_points_check_their_arguments_on_the_host():
    """alpha outside [0, 1], a temperature that is 0, negative, infinite or nan, null teacher logits with alpha != 0, a null output:
    NBEST_ERR_ARG (-1) and a message before anything touches a device; nbest_stc_heads_logits: null pointers, the dtype, the shape"""
    L = hipabi.lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    ls = hipabi.LabelSpaceC(3, 8, 10, 1 << 20, 1 << 20, 1 << 20)
    inf, nan = float("inf"), float("nan")

    def call(t_logits, alpha, T, top=fake, loss=fake):
        return L.nbest_stc_heads_kd_t(fake, 4, fake, fake, ctypes.byref(ls), fake, t_logits, alpha, T, top, fake, fake, loss,
                                      fake, fake, fake, 1, 4, hipabi.F32, 1, 0, 0.0, 0, 0, fake, 1 << 20, null)
    for args in ((fake, -0.1, 2.0), (fake, 1.5, 2.0), (fake, nan, 2.0), (fake, 0.5, 0.0), (fake, 0.5, -1.0), (fake, 0.5, inf),
                 (fake, 0.5, -inf), (fake, 0.5, nan), (fake, 0.0, 0.0), (null, 0.5, 2.0), (null, 1.0, 1.0)):
        assert call(*args) == -1, args
        assert "stc_heads_kd_t" in hipabi.last_error(), args
    for kw in (dict(top=null), dict(loss=null)):                        # a null output, with and without a teacher
        for t_logits, alpha in ((fake, 0.5), (null, 0.0)):
            assert call(t_logits, alpha, 2.0, **kw) == -1, kw
            assert "null pointer" in hipabi.last_error()

    def logits(hidden=fake, Wh=fake, bh=fake, space=ls, out=fake, B=1, H=4, dtype=hipabi.F32):
        return L.nbest_stc_heads_logits(hidden, 4, Wh, bh, ctypes.byref(space), out, B, H, dtype, null)
    for kw in (dict(hidden=null), dict(Wh=null), dict(bh=null), dict(out=null), dict(B=0), dict(H=0)):
        assert logits(**kw) == -1, kw
        assert "stc_heads_logits" in hipabi.last_error()
    assert logits(dtype=77) == -3 and "stc_heads_logits" in hipabi.last_error()                     # NBEST_ERR_DTYPE
    assert logits(H=2049) == -2 and "stc_heads_logits" in hipabi.last_error()                       # NBEST_ERR_SHAPE
    assert logits(space=hipabi.LabelSpaceC(3, 8, 3, 1 << 20, 1 << 20, 1 << 20)) == -2               # R > n_top


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_default_and_values():
    assert cli.parse_arguments(BASE).distill_temperature is None
    assert cli.parse_arguments(BASE + KD).distill_temperature is None
    assert cli.parse_arguments(BASE + KD + ["--distill_temperature", "2"]).distill_temperature == 2.0
    assert cli.parse_arguments(BASE + KD + ["--distill_temperature", "1.0", "--distill_alpha", "1"]).distill_temperature == 1.0


def test_cli_refusals(capsys):
    for bad, word in ((["--distill_temperature", "2"], "--distill_from"),
                      (KD + ["--distill_temperature", "0"], "--distill_temperature"),
                      (KD + ["--distill_temperature", "-1"], "--distill_temperature"),
                      (KD + ["--distill_temperature", "nan"], "--distill_temperature"),
                      (KD + ["--distill_temperature", "inf"], "--distill_temperature"),
                      (KD + ["--distill_temperature", "2", "--testing"], "--testing")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_exp_dir_gains_kdT_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert "kdT_" not in plain
    assert cli.exp_dir(cli.parse_arguments(BASE + KD)) == plain + "__kd_0.5"
    assert cli.exp_dir(cli.parse_arguments(BASE + KD + ["--distill_temperature", "2"])) == plain + "__kd_0.5__kdT_2.0"
    assert cli.exp_dir(cli.parse_arguments(BASE + KD + ["--distill_temperature", "1"])) == plain + "__kd_0.5__kdT_1.0"
    # every existing combination keeps its name without the flag, and gains only the last part with it
    for extra in ([], ["--distill_alpha", "0.3"], ["--ema_decay", "0.9"], ["--freeze_layers", "1"],
                  ["--distill_alpha", "0.3", "--ema_decay", "0.9", "--freeze_layers", "1"], ["--encoder_layers", "3", "--dtype", "fp8w"]):
        without = cli.exp_dir(cli.parse_arguments(BASE + KD + extra))
        assert "kdT_" not in without
        assert cli.exp_dir(cli.parse_arguments(BASE + KD + extra + ["--distill_temperature", "4"])) == without + "__kdT_4.0"
    assert cli.exp_dir(cli.parse_arguments(BASE + KD + ["--distill_alpha", "0.3", "--ema_decay", "0.9", "--freeze_layers", "1"])) == \
        plain + "__fz_none_1__ema_0.9__kd_0.3"
