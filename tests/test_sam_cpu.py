"""CPU: sharpness-aware minimization (--sam_rho).  The fp64 restatement of tests/sam_ref.py against the closed form on a quadratic
and ASAM's invariance under a rescaling of the weights; where the bar of the adaptive block sums comes from (an fp32 restatement's
own error over the summation orders of a 256-lane reduction, 4 x); the declarations, bindings and host-side argument checks of the
three entry points; trainer.sam_args' refusals; the command line."""
import ctypes
import math
import os
import re

import pytest
import torch

import conftest
import optim_ref as R
import sam_ref as S
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi, trainer

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]
SAM = ["--sam_rho", "0.05"]
SYMBOLS = ("nbest_sam_norms", "nbest_sam_perturb", "nbest_sam_restore")


@pytest.fixture(scope="module")
def tab():
    return R.table()


@pytest.fixture(scope="module")
def pg(tab):
    return S.state(tab)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_reference_matches_the_closed_form_on_a_quadratic(tab, pg):
    """L = 1/2 w^T A w with a diagonal A: the gradient is A w, the SAM gradient A (w + rho A w / ||A w||) = A w + rho A^2 w / ||A w||.
    sam_reference fed g = A w must land on w + rho A w / ||A w|| (to fp64 rounding), ||e|| = rho, and leave the guards, the gaps and
    the inactive tensor where they were"""
    p = pg[0]
    act = R.covered(tab, active_only=True)
    gen = torch.Generator().manual_seed(5)
    a = (torch.rand(tab.total, generator=gen) + 0.5).float()
    g = (a * p).float()                                              # fp32 inputs, as the arenas hold
    r = S.sam_reference(tab, p, g, S.RHO)
    a64, w, g64 = a.double(), p.double(), g.double()
    gn = g64[act].norm().item()
    want_grad = a64 * w + S.RHO * a64 * g64 / gn                     # A w + rho A (A w) / ||A w||, A w as the fp32 g holds it
    got_grad = a64 * r.p
    assert ((got_grad - want_grad)[act].abs().max() / want_grad[act].abs().max()).item() < 1e-12
    assert abs(r.e[act].norm().item() - S.RHO) < 1e-12 and abs(r.norm - gn) < 1e-9 * gn
    assert torch.equal(r.p[~act], w[~act]) and r.e[~act].abs().max().item() == 0.0
    # rho = 0, a zero gradient, an infinite norm: nothing moves and nothing is NaN
    for kw in (dict(rho=0.0), dict(rho=S.RHO, norm=0.0), dict(rho=S.RHO, norm=float("inf")), dict(rho=S.RHO, norm=float("nan"))):
        z = S.sam_reference(tab, p, g, **kw)
        assert z.s == 0.0 and torch.equal(z.p, w)
    assert S.sam_reference(tab, p, torch.zeros_like(g), S.RHO).s == 0.0


def test_asam_is_invariant_under_a_rescaling_of_the_weights(tab, pg):
    """w -> c w, g -> g / c (the gradient of the same function in the rescaled coordinates), eta -> c eta: T g and hence the norm do
    not change and e -> c e, so the perturbed point is the rescaled perturbed point.  c = 4: every rescaled fp32 input is exact.
    Plain SAM has no such property: its e shrinks by 1 / c while w grows by c"""
    p, g = pg
    act = R.covered(tab, active_only=True)
    c = 4.0
    r1 = S.sam_reference(tab, p, g, S.ASAM_RHO, eta=S.ETA)
    rc = S.sam_reference(tab, p * c, g / c, S.ASAM_RHO, eta=R.f32(S.ETA) * c)
    assert abs(rc.norm - r1.norm) <= 1e-12 * r1.norm
    assert ((rc.p - c * r1.p)[act].abs().max() / (c * r1.p)[act].abs().max()).item() < 1e-12
    t = p.double().abs() + R.f32(S.ETA)
    assert abs((r1.e / t)[act].norm().item() - S.ASAM_RHO) < 1e-12              # ||T^-1 e|| = rho: the adaptive ball's radius
    s1 = S.sam_reference(tab, p, g, S.RHO)
    sc = S.sam_reference(tab, p * c, g / c, S.RHO)
    assert abs(sc.e[act].norm().item() - S.RHO) < 1e-12 and (sc.p - c * s1.p)[act].abs().max().item() > 1e-3


def test_reference_scale_from_the_device_norm_is_fp32(tab, pg):
    """fed the device's norm, s is float32(rho) / (norm + 1e-12f) in IEEE fp32 - representable in fp32 - and within 3 x 2^-24 of the
    fp64 quotient (rho's conversion, the addition, the division)"""
    import numpy as np
    p, g = pg
    exact = S.sam_reference(tab, p, g, S.RHO)
    r = S.sam_reference(tab, p, g, S.RHO, norm=float(np.float32(exact.norm)))
    assert float(np.float32(r.s)) == r.s
    assert abs(r.s - exact.s) <= 3 * S.EPS * exact.s


# ---- the bar of the adaptive block sums --------------------------------------------------------------------------------------------------
def test_adaptive_partials_leg_stays_inside_what_the_bar_assumes(tab, pg):
    """every fp32 summation order is under 16 x 2^-24 (a cap on the legs, not on the kernel) and under ASAM_LEG_WORST, which the
    kernel test's bar is 4 x of; the fp64 block sums are 0 exactly where the kernel must write 0"""
    p, g = pg
    worst = S.adaptive_leg_ratios(tab, p, g, S.ETA)
    R.log("sam-leg adaptive block sums, fp32 vs fp64, worst ratios in 2^-24: %s   bar = 4 x, rounded up: %d"
          % ("  ".join("%s %.2f" % kv for kv in sorted(worst.items())), S.ASAM_PARTIAL_K))
    assert len(worst) >= 4
    for order, w in worst.items():
        assert w < 16 and w <= S.ASAM_LEG_WORST, (order, w)
    assert max(worst.values()) > 0.25 and S.ASAM_PARTIAL_K == math.ceil(4 * S.ASAM_LEG_WORST)
    ref = S.adaptive_partials(tab, p, g, S.ETA)
    for t in tab.tensors:
        blocks = ref[t.block_start:t.block_start + (t.numel + R.CHUNK - 1) // R.CHUNK]
        assert bool((blocks == 0).all()) == (not t.active or t.gnorm == 0.0)


# ---- header, bindings, host-side checks -----------------------------------------------------------------------------------------------------
def test_header_declares_and_hipabi_binds_the_entry_points():
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    assert "K9s" in hdr
    L = ctypes.CDLL(hipabi.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name) and name in hipabi.EXPORTS
    L = hipabi.lib()
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert list(L.nbest_sam_norms.argtypes) == [vp, vp, vp, i32, i32, f32, vp, vp]
    assert list(L.nbest_sam_perturb.argtypes) == [vp, vp, vp, vp, vp, i32, i32, vp, f32, f32, vp]
    assert list(L.nbest_sam_restore.argtypes) == [vp, vp, vp, vp, i32, i32, vp]
    assert all(getattr(L, n).restype is ctypes.c_int for n in SYMBOLS)


def test_entry_points_check_their_arguments_on_the_host():
    """a NULL p / g / backup / descs / norm / partial, n_tensors <= 0, n_blocks <= 0, a negative or non-finite rho, eta == 0 or a
    non-finite eta (norms: eta <= 0): NBEST_ERR_ARG (-1) and a message naming the call, before anything touches a device"""
    L = hipabi.lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    inf, nan = float("inf"), float("nan")

    def norms(p=fake, g=fake, d=fake, n_t=3, n_b=5, eta=0.01, part=fake):
        return L.nbest_sam_norms(p, g, d, n_t, n_b, eta, part, null)

    def perturb(p=fake, g=fake, bk=fake, low=fake, d=fake, n_t=3, n_b=5, norm=fake, rho=0.05, eta=-1.0):
        return L.nbest_sam_perturb(p, g, bk, low, d, n_t, n_b, norm, rho, eta, null)

    def restore(p=fake, bk=fake, low=fake, d=fake, n_t=3, n_b=5):
        return L.nbest_sam_restore(p, bk, low, d, n_t, n_b, null)

    bad = [(norms, dict(p=null)), (norms, dict(g=null)), (norms, dict(d=null)), (norms, dict(part=null)), (norms, dict(n_t=0)),
           (norms, dict(n_b=0)), (norms, dict(eta=0.0)), (norms, dict(eta=-0.01)), (norms, dict(eta=inf)), (norms, dict(eta=nan)),
           (perturb, dict(p=null)), (perturb, dict(g=null)), (perturb, dict(bk=null)), (perturb, dict(d=null)), (perturb, dict(norm=null)),
           (perturb, dict(n_t=0)), (perturb, dict(n_t=-1)), (perturb, dict(n_b=0)), (perturb, dict(rho=-0.05)), (perturb, dict(rho=inf)),
           (perturb, dict(rho=nan)), (perturb, dict(eta=0.0)), (perturb, dict(eta=inf)), (perturb, dict(eta=-inf)), (perturb, dict(eta=nan)),
           (restore, dict(p=null)), (restore, dict(bk=null)), (restore, dict(d=null)), (restore, dict(n_t=0)), (restore, dict(n_b=0))]
    for fn, kw in bad:
        assert fn(**kw) == -1, (fn.__name__, kw)
        assert "sam_" + fn.__name__ in hipabi.last_error(), (fn.__name__, kw, hipabi.last_error())


# ---- trainer.sam_args ---------------------------------------------------------------------------------------------------------------------
class _M:
    lora, fp8_forward, head_mask_trainable = None, False, False


class _O:
    sharded = False


def test_sam_args():
    m, o = _M(), _O()
    assert trainer.sam_args(None, True, 0.01, m, o, 1.0, 4, 4) is None                      # without sam_rho nothing is looked at
    assert trainer.sam_args(0.05, False, 0.01, m, o, None, 1) == dict(rho=0.05, adaptive=False, eta=0.01)
    assert trainer.sam_args(0, True, 0.1, m, o, None, 1) == dict(rho=0.0, adaptive=True, eta=0.1)
    for rho in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sam_rho"):
            trainer.sam_args(rho, False, 0.01, m, o, None, 1)
    for eta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sam_eta"):
            trainer.sam_args(0.05, True, eta, m, o, None, 1)
    assert trainer.sam_args(0.05, False, 0.0, m, o, None, 1)["eta"] == 0.0                  # plain SAM does not read eta
    with pytest.raises(ValueError, match="adv_epsilon"):
        trainer.sam_args(0.05, False, 0.01, m, o, 1.0, 1)
    for field, word in (("lora", "LoRA"), ("fp8_forward", "fp8w"), ("head_mask_trainable", "head mask")):
        mm = _M()
        setattr(mm, field, object() if field == "lora" else True)
        with pytest.raises(RuntimeError, match=word):
            trainer.sam_args(0.05, False, 0.01, mm, o, None, 1)
    oo = _O()
    oo.sharded = True
    with pytest.raises(RuntimeError, match="sharded"):
        trainer.sam_args(0.05, False, 0.01, m, oo, None, 1)
    with pytest.raises(RuntimeError, match="data parallelism"):
        trainer.sam_args(0.05, False, 0.01, m, o, None, 2)
    with pytest.raises(RuntimeError, match="gradient accumulation"):
        trainer.sam_args(0.05, False, 0.01, m, o, None, 1, 4)


def test_train_step_refuses_before_touching_anything():
    """the batch is never looked at: the refusals come before the teacher runs, the batch is doubled or anything is enqueued"""
    batch = dict(ids=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="adv_epsilon"):
        trainer.train_step(_M(), _O(), batch, adv_epsilon=1.0, sam_rho=0.05)
    with pytest.raises(ValueError, match="sam_rho"):
        trainer.train_step(_M(), _O(), batch, sam_rho=-1.0)
    o = _O()
    o.sam_pending = True
    with pytest.raises(RuntimeError, match="pending"):
        trainer.train_step(_M(), o, batch, sam_rho=0.05)
    import inspect
    from nbest_amd.model import NBestSTCModel
    assert inspect.signature(NBestSTCModel.forward_backward).parameters["advance"].default is True


# ---- command line ------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_and_combinations():
    opt = cli.parse_arguments(BASE)
    assert opt.sam_rho is None and opt.sam_adaptive is False and opt.sam_eta is None
    opt = cli.parse_arguments(BASE + SAM)
    assert (opt.sam_rho, opt.sam_adaptive, opt.sam_eta) == (0.05, False, 0.01)
    opt = cli.parse_arguments(BASE + SAM + ["--sam_adaptive"])
    assert (opt.sam_rho, opt.sam_adaptive, opt.sam_eta) == (0.05, True, 0.01)
    opt = cli.parse_arguments(BASE + ["--sam_rho", "1", "--sam_adaptive", "--sam_eta", "0.1"])
    assert (opt.sam_rho, opt.sam_adaptive, opt.sam_eta) == (1.0, True, 0.1)
    for optim in (["--optim_choice", "bertadam"], ["--optim_choice", "adam"], ["--optim_choice", "adamw", "--restated_adamw"]):
        opt = cli.parse_arguments(BASE + SAM + optim + ["--ema_decay", "0.9", "--resume", "--add_l2_loss", "--freeze_embeddings",
                                                        "--freeze_layers", "1"])
        assert opt.sam_rho == 0.05 and opt.ema_decay == 0.9 and opt.n_accum_steps == 1
    assert cli.parse_arguments(BASE + SAM + ["--rdrop_alpha", "1.0", "--dropout", "0.3", "--contrastive_weight", "0.1"]).sam_rho == 0.05
    assert cli.parse_arguments(BASE + SAM + ["--distill_from", "t.pt", "--distill_temperature", "2"]).sam_rho == 0.05


def test_cli_exp_dir_moves_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert plain.endswith("__cls_stc") and "sam" not in plain
    assert cli.exp_dir(cli.parse_arguments(BASE + SAM)) == plain + "__sam_0.05"
    assert cli.exp_dir(cli.parse_arguments(BASE + SAM + ["--sam_adaptive"])) == plain + "__asam_0.05_0.01"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--sam_rho", "1", "--sam_adaptive", "--sam_eta", "0.1"])) == plain + "__asam_1.0_0.1"
    assert cli.exp_dir(cli.parse_arguments(BASE + SAM + ["--ema_decay", "0.9", "--rdrop_alpha", "1.0", "--dropout", "0.3"])) \
        == plain.replace("dp_0.0_", "dp_0.3_") + "__ema_0.9__rdrop_1.0__sam_0.05"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--rdrop_alpha", "1.0", "--dropout", "0.3"])).endswith("__rdrop_1.0")


def test_cli_refusals(tmp_path, monkeypatch, capsys):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    hm = tmp_path / "mask.json"
    hm.write_text("[[1.0, 0.0]]\n")
    for bad, word in ((SAM + ["--testing"], "--testing"), (SAM + ["--predict", str(src)], "--predict"),
                      (SAM + ["--head_importance", str(tmp_path / "imp.json")], "--head_importance"),
                      (SAM + ["--adv_epsilon", "1.0"], "--adv_epsilon"), (SAM + ["--lora_rank", "4"], "--lora_rank"),
                      (SAM + ["--dtype", "fp8w"], "fp8w"), (SAM + ["--train_head_mask", str(hm)], "--train_head_mask"),
                      (SAM + ["--shard_optimizer", "on"], "--shard_optimizer"), (SAM + ["--n_layers", "12"], "gradient accumulation"),
                      (["--sam_rho", "0"], "--sam_rho"), (["--sam_rho", "-0.1"], "--sam_rho"), (["--sam_rho", "inf"], "--sam_rho"),
                      (["--sam_rho", "nan"], "--sam_rho"), (SAM + ["--sam_adaptive", "--sam_eta", "0"], "--sam_eta"),
                      (SAM + ["--sam_adaptive", "--sam_eta", "-1"], "--sam_eta"), (SAM + ["--sam_adaptive", "--sam_eta", "inf"], "--sam_eta"),
                      (SAM + ["--sam_eta", "0.1"], "--sam_adaptive"), (["--sam_adaptive"], "--sam_rho"), (["--sam_eta", "0.1"], "--sam_rho")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        err = capsys.readouterr().err
        assert word in err and "sam" in err, (bad, err)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + SAM)
    assert "data parallelism is not built" in capsys.readouterr().err
    assert cli.parse_arguments(BASE).sam_rho is None                       # ... and fine without the flag
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.parse_arguments(BASE + SAM).sam_rho == 0.05
