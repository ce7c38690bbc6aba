"""CPU tests of knowledge distillation (--distill_from): the C ABI declares and hipabi binds nbest_stc_heads_kd, its host-side
argument checks, the command-line surface (defaults, refused combinations, the experiment-directory name), the teacher -> student
layer mapping on state dicts, and the fp64 restatement of the soft loss that tests/test_distill_gpu.py holds the kernel to
(checked here by torch.autograd.gradcheck and against the hard loss for a one-hot teacher) - device-free."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi, trainer

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]
KD = ["--distill_from", "teacher.pt"]


# ---- the restatement (any float dtype; the GPU tests run it in fp64) ---------------------------------------------------------------
def heads_scores(cls, Wh, bh, top2bottom):
    """The STC heads on CLS rows [B, H] with the concatenated head matrix Wh [R, H] / bh [R] of the C ABI (rows 0..n_top-1: the top
    classifier, then one block per multi-value top in top order) -> top [B, n_top], bott [B, R - n_top], final [B, n_bottom]"""
    n_top = len(top2bottom)
    z = cls @ Wh.t() + bh
    top = torch.sigmoid(z[:, :n_top])
    row, botts, cols, ids = n_top, [], [], []
    for t in range(n_top):
        bs = top2bottom[t]
        if len(bs) >= 2:
            s = torch.softmax(z[:, row:row + len(bs)], dim=1)
            row += len(bs)
            botts.append(s)
            cols.append(top[:, t:t + 1] * s)
        else:
            cols.append(top[:, t:t + 1])
        ids += list(bs)
    inv = torch.empty(len(ids), dtype=torch.long)
    inv[torch.tensor(ids)] = torch.arange(len(ids))
    return top, torch.cat(botts, dim=1), torch.cat(cols, dim=1)[:, inv]


def bottoms_dict(bott, top2bottom):
    out, col = {}, 0
    for t in range(len(top2bottom)):
        n = len(top2bottom[t])
        if n >= 2:
            out["lin_%d" % t] = bott[:, col:col + n]
            col += n
    return out


def soft_loss(top, bott, final, t_top, t_bott, t_final, top2bottom):
    """The reference's three loss terms with a teacher's scores in place of the labels, summed over the batch:
    BCE_sum(final, t_final) + BCE_sum(top, t_top) + (1 / n_heads) sum_k sum_j -t_bott_kj log(s_kj + 1e-12).
    torch's BCE clamps its logs at -100 and its gradient's denominator at 1e-12, as the kernel does."""
    n_heads = sum(1 for v in top2bottom.values() if len(v) >= 2)
    ce = -(t_bott * torch.log(bott + 1e-12)).sum() / n_heads
    return F.binary_cross_entropy(final, t_final, reduction="sum") + F.binary_cross_entropy(top, t_top, reduction="sum") + ce


def hard_parts(top, bott, final, y, top2bottom):
    """[BCE_sum(final, y), BCE_sum(top, y . B2T), mean over heads of NLL_sum] through the oracle's restatement of the reference"""
    from oracle import stc
    b2t = stc.bottom2top_matrix(top2bottom).to(y.dtype)
    _, _, parts = stc.total_loss(top, bottoms_dict(bott, top2bottom), final, y, top2bottom, b2t)
    return [parts["bottom_bce"], parts["top_bce"], parts["ce"]]


def onehot_teacher(y, top2bottom):
    """the teacher that IS the labels: t_final = y, t_top = y . B2T, t_bott = the one-hot class of every head, its last column
    (NONE) where the head has no active label"""
    from oracle import stc
    t_top = y @ stc.bottom2top_matrix(top2bottom).to(y.dtype)
    botts = []
    for t in range(len(top2bottom)):
        ids = top2bottom[t]
        if len(ids) >= 2:
            botts.append(F.one_hot(stc.class_index(y[:, ids]), len(ids)).to(y.dtype))
    return t_top, torch.cat(botts, dim=1), y.clone()


def kd_reference(cls, Wh, bh, y, t_top, t_bott, t_final, alpha, top2bottom):
    """fp64: loss_parts[4] = the three hard terms and the soft loss, and the gradients of (1 - alpha) * hard + alpha * soft with
    respect to the CLS rows, Wh and bh - what nbest_stc_heads_kd returns"""
    d = lambda x: x.detach().double().cpu()
    cls, Wh, bh = (d(x).requires_grad_(True) for x in (cls, Wh, bh))
    top, bott, final = heads_scores(cls, Wh, bh, top2bottom)
    hard = hard_parts(top, bott, final, d(y), top2bottom)
    soft = soft_loss(top, bott, final, d(t_top), d(t_bott), d(t_final), top2bottom)
    ((1.0 - alpha) * sum(hard) + alpha * soft).backward()
    return dict(loss_parts=torch.stack(hard + [soft]).detach(), dcls=cls.grad, dWh=Wh.grad, dbh=bh.grad,
                top=top.detach(), bott=bott.detach(), final=final.detach())


# a 3-top label space: a single-bottom top, a 2-column head and a 5-column head (R = 3 + 2 + 5, n_bottom = 8)
SMALL_SPACE = {0: [0], 1: [1, 2], 2: [3, 4, 5, 6, 7]}


def _teacher_draw(B, top2bottom, gen, dtype=torch.float64):
    n_top = len(top2bottom)
    t_top = torch.sigmoid(torch.randn(B, n_top, generator=gen, dtype=dtype))
    botts, fin = [], torch.zeros(B, sum(len(v) for v in top2bottom.values()), dtype=dtype)
    for t in range(n_top):
        ids = top2bottom[t]
        if len(ids) >= 2:
            s = torch.softmax(torch.randn(B, len(ids), generator=gen, dtype=dtype), dim=1)
            botts.append(s)
            fin[:, ids] = t_top[:, t:t + 1] * s
        else:
            fin[:, ids] = t_top[:, t:t + 1]
    return t_top, torch.cat(botts, dim=1), fin


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hipabi_binds_the_entry_point():
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    m = re.search(r"int nbest_stc_heads_kd\(([^;]*)\);", hdr)
    assert m, "include/nbest_hip.h does not declare nbest_stc_heads_kd"
    decl = " ".join(m.group(1).split())
    for arg in ("const float* t_top", "const float* t_bott", "const float* t_final", "float alpha"):
        assert arg in decl, arg
    plain = " ".join(re.search(r"int nbest_stc_heads\(([^;]*)\);", hdr).group(1).split())
    assert len(decl.split(",")) == len(plain.split(",")) + 4
    assert "nbest_stc_heads_kd" in hipabi.EXPORTS and "nbest_stc_heads" in hipabi.EXPORTS
    assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), "nbest_stc_heads_kd")
    L = hipabi.lib()
    assert len(L.nbest_stc_heads_kd.argtypes) == len(L.nbest_stc_heads.argtypes) + 4
    assert L.nbest_stc_heads_kd.argtypes[9] is ctypes.c_float
    assert hasattr(hipabi, "stc_heads_kd")


def test_entry_point_checks_alpha_and_the_teacher_pointers_on_the_host():
    """alpha outside [0, 1], a null teacher array with alpha != 0, or only some of the three: NBEST_ERR_ARG (-1) and a message
    before anything touches a device"""
    L = hipabi.lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    ls = hipabi.LabelSpaceC(3, 8, 10, 1 << 20, 1 << 20, 1 << 20)

    def call(t_top, t_bott, t_fin, alpha):
        return L.nbest_stc_heads_kd(fake, 4, fake, fake, ctypes.byref(ls), fake, t_top, t_bott, t_fin, alpha, fake, fake, fake, fake,
                                    fake, fake, fake, 1, 4, hipabi.F32, 1, 0, 0.0, 0, 0, fake, 1 << 20, null)
    for args in ((fake, fake, fake, -0.1), (fake, fake, fake, 1.5), (fake, fake, fake, float("nan")), (null, fake, fake, 0.5),
                 (fake, null, fake, 0.5), (fake, fake, null, 1.0), (null, null, null, 0.5), (null, fake, fake, 0.0)):
        assert call(*args) == -1, args
        assert "stc_heads_kd" in hipabi.last_error()


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_defaults():
    opt = cli.parse_arguments(BASE)
    assert opt.distill_from is None and opt.distill_teacher_layers is None and opt.distill_init_layers is None
    assert opt.distill_alpha == 0.5
    opt = cli.parse_arguments(BASE + KD)
    assert opt.distill_from == "teacher.pt" and opt.distill_alpha == 0.5 and opt.distill_teacher_layers is None
    opt = cli.parse_arguments(BASE + KD + ["--distill_teacher_layers", "12", "--distill_alpha", "1", "--distill_init_layers", "1,3,5",
                                           "--encoder_layers", "3", "--ema_decay", "0.9", "--freeze_layers", "1", "--resume",
                                           "--dtype", "fp8w"])
    assert (opt.distill_teacher_layers, opt.distill_alpha, opt.distill_init_layers) == (12, 1.0, [1, 3, 5])
    assert cli.parse_arguments(BASE + KD + ["--distill_alpha", "0"]).distill_alpha == 0.0


def test_cli_exp_dir_moves_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert plain.endswith("__cls_stc") and "kd_" not in plain
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--distill_alpha", "0.3"])) == plain
    assert cli.exp_dir(cli.parse_arguments(BASE + KD)) == plain + "__kd_0.5"
    assert cli.exp_dir(cli.parse_arguments(BASE + KD + ["--distill_alpha", "0.3", "--ema_decay", "0.9", "--freeze_layers", "1"])) == \
        plain + "__fz_none_1__ema_0.9__kd_0.3"


def test_cli_refusals(tmp_path, monkeypatch, capsys):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    for bad, word in ((KD + ["--testing"], "--testing"), (KD + ["--predict", str(src)], "--predict"),
                      (KD + ["--head_importance", str(tmp_path / "imp.json")], "--head_importance"),
                      (KD + ["--distill_alpha", "1.5"], "--distill_alpha"), (KD + ["--distill_alpha", "-0.1"], "--distill_alpha"),
                      (KD + ["--distill_alpha", "nan"], "--distill_alpha"),
                      (KD + ["--distill_init_layers", "1,3", "--init_checkpoint", "x.pt"], "replaces --init_checkpoint"),
                      (KD + ["--distill_init_layers", "1,x"], "--distill_init_layers"), (KD + ["--distill_init_layers", "-1"], ">= 0"),
                      (KD + ["--distill_teacher_layers", "0"], "--distill_teacher_layers"),
                      (["--distill_init_layers", "1,3"], "--distill_from"), (["--distill_teacher_layers", "12"], "--distill_from")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        assert word in capsys.readouterr().err, bad
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + KD)
    assert "data-parallel teacher is not built" in capsys.readouterr().err
    assert cli.parse_arguments(BASE).distill_from is None            # ... and fine without the flag
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.parse_arguments(BASE + KD + ["--init_checkpoint", "x.pt"]).init_checkpoint == "x.pt"


# ---- teacher -> student state dicts ------------------------------------------------------------------------------------------------
def _synthetic_state(L):
    sd = {"bert_encoder.embeddings.word_embeddings.weight": torch.full((4, 2), -1.0),
          "bert_encoder.embeddings.LayerNorm.bias": torch.full((2,), -2.0),
          "bert_encoder.pooler.dense.weight": torch.full((2, 2), -3.0),
          "clf.top_linear_layer.weight": torch.full((3, 2), -4.0), "clf.linear_layers.lin_2.bias": torch.full((5,), -5.0)}
    for l in range(L):
        sd["bert_encoder.encoder.layer.%d.attention.self.query.weight" % l] = torch.full((2, 2), float(l))
        sd["bert_encoder.encoder.layer.%d.output.LayerNorm.bias" % l] = torch.full((2,), 10.0 + l)
    return sd


def test_student_state_from_teacher_maps_layers_and_copies_the_rest():
    sd = _synthetic_state(6)
    before = {k: v.clone() for k, v in sd.items()}
    out = trainer.student_state_from_teacher(sd, [1, 3, 5])
    layer_keys = sorted(k for k in out if ".encoder.layer." in k)
    assert layer_keys == sorted("bert_encoder.encoder.layer.%d.%s" % (k, s) for k in range(3)
                                for s in ("attention.self.query.weight", "output.LayerNorm.bias"))
    for k, i in enumerate([1, 3, 5]):
        assert torch.equal(out["bert_encoder.encoder.layer.%d.attention.self.query.weight" % k], torch.full((2, 2), float(i)))
        assert torch.equal(out["bert_encoder.encoder.layer.%d.output.LayerNorm.bias" % k], torch.full((2,), 10.0 + i))
    for k in sd:
        if ".encoder.layer." not in k:
            assert torch.equal(out[k], sd[k]), k                      # embeddings, pooler and heads as they are
    assert len(out) == 5 + 2 * 3
    assert set(sd) == set(before) and all(torch.equal(sd[k], before[k]) for k in sd), "the teacher's state dict was modified"
    # a layer may be used twice, and the order is the list's
    out = trainer.student_state_from_teacher(sd, [4, 4, 0])
    assert [float(out["bert_encoder.encoder.layer.%d.attention.self.query.weight" % k][0, 0]) for k in range(3)] == [4.0, 4.0, 0.0]


@pytest.mark.parametrize("layers", [[], [6], [0, 7], [-1], [1, 3, 5, 6]])
def test_student_state_from_teacher_refuses_bad_lists(layers):
    with pytest.raises(ValueError):
        trainer.student_state_from_teacher(_synthetic_state(6), layers)


# ---- the restatement itself --------------------------------------------------------------------------------------------------------
def _small_problem(B=3, H=6, seed=0):
    gen = torch.Generator().manual_seed(seed)
    R = len(SMALL_SPACE) + sum(len(v) for v in SMALL_SPACE.values() if len(v) >= 2)
    cls = torch.randn(B, H, generator=gen, dtype=torch.float64)
    Wh = torch.randn(R, H, generator=gen, dtype=torch.float64) * 0.5
    bh = torch.randn(R, generator=gen, dtype=torch.float64) * 0.5
    return cls, Wh, bh, gen


def test_restatement_shapes_and_scores():
    cls, Wh, bh, _ = _small_problem()
    top, bott, final = heads_scores(cls, Wh, bh, SMALL_SPACE)
    assert top.shape == (3, 3) and bott.shape == (3, 7) and final.shape == (3, 8)
    assert torch.allclose(final[:, 0], top[:, 0]) and torch.allclose(final[:, 1:3], top[:, 1:2] * bott[:, :2])
    assert torch.allclose(final[:, 3:], top[:, 2:3] * bott[:, 2:]) and torch.allclose(bott[:, 2:].sum(1), torch.ones(3, dtype=torch.float64))


def test_soft_loss_gradcheck():
    """d(soft loss) / d(CLS rows, Wh, bh) through the heads, on the 3-top label space: a single-bottom top, a 2-column head and a
    5-column head; the teacher's scores are random sigmoid / softmax draws"""
    cls, Wh, bh, gen = _small_problem()
    t_top, t_bott, t_fin = _teacher_draw(3, SMALL_SPACE, gen)

    def f(cls, Wh, bh):
        return soft_loss(*heads_scores(cls, Wh, bh, SMALL_SPACE), t_top, t_bott, t_fin, SMALL_SPACE)
    assert torch.autograd.gradcheck(f, tuple(x.clone().requires_grad_(True) for x in (cls, Wh, bh)), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_one_hot_teacher_turns_the_soft_loss_into_the_hard_loss():
    """t_final = y, t_top = y . B2T, t_bott = the one-hot class (NONE for an empty head): the soft loss is the sum of the three hard
    terms, and so is its gradient"""
    cls, Wh, bh, _ = _small_problem(B=4)
    y = torch.zeros(4, 8, dtype=torch.float64)
    y[0, 0] = y[0, 4] = 1          # the single-bottom top and a column of the 5-column head; the 2-column head takes NONE
    y[1, 1] = 1
    y[2, 7] = y[2, 2] = 1          # row 3: no label at all
    t_top, t_bott, t_fin = onehot_teacher(y, SMALL_SPACE)
    assert t_bott.tolist()[0] == [0, 1, 0, 1, 0, 0, 0] and t_bott.tolist()[3] == [0, 1, 0, 0, 0, 0, 1]
    assert t_top.tolist() == [[1, 0, 1], [0, 1, 0], [0, 1, 1], [0, 0, 0]]
    a = kd_reference(cls, Wh, bh, y, t_top, t_bott, t_fin, 0.0, SMALL_SPACE)
    b = kd_reference(cls, Wh, bh, y, t_top, t_bott, t_fin, 1.0, SMALL_SPACE)
    assert torch.allclose(a["loss_parts"][3], a["loss_parts"][:3].sum(), rtol=1e-12)
    for k in ("dcls", "dWh", "dbh"):
        assert torch.allclose(a[k], b[k], rtol=1e-10, atol=1e-12), k
    # ... and a soft teacher does not
    gen = torch.Generator().manual_seed(5)
    c = kd_reference(cls, Wh, bh, y, *_teacher_draw(4, SMALL_SPACE, gen), 1.0, SMALL_SPACE)
    assert not torch.allclose(c["dcls"], a["dcls"], rtol=1e-3)
