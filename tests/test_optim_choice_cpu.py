"""CPU tests of --optim_choice adam | adamw: the CLI accepts them, the host learning-rate schedule equals
transformers.get_linear_schedule_with_warmup, and the C ABI exports the fused Adam / AdamW entry points."""
import ctypes

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import arena as ar, cli, hipabi, synth
from nbest_amd import config as ncfg
from nbest_amd.optim import HipAdam, linear_schedule_with_warmup

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]


@pytest.mark.parametrize("kind", ["adam", "adamw", "bertadam"])
def test_cli_accepts_every_reference_optimizer(kind):
    extra = ["--restated_adamw"] if kind == "adamw" else []
    opt = cli.parse_arguments(BASE + ["--optim_choice", kind, "--max_norm", "2.5", "--l2", "1e-4"] + extra)
    assert opt.optim_choice == kind and opt.max_norm == 2.5 and opt.l2 == 1e-4


def test_cli_adamw_needs_the_restatement_acknowledged(capsys):
    """the reference's AdamW is gone from current transformers releases: adamw runs this build's restatement, asked for by name"""
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + ["--optim_choice", "adamw"])
    assert "--restated_adamw" in capsys.readouterr().err
    assert cli.parse_arguments(BASE + ["--optim_choice", "adam"]).optim_choice == "adam"


def test_cli_defaults_match_the_reference_for_the_clip():
    opt = cli.parse_arguments(BASE + ["--optim_choice", "adamw", "--restated_adamw"])
    assert opt.max_norm == 5.0 and opt.l2 == 0


@pytest.mark.parametrize("T", [1, 7, 40, 123])
def test_linear_schedule_matches_transformers(T):
    transformers = pytest.importorskip("transformers")
    for W in sorted({0, 1, int(0.1 * T)}):
        p1, p2 = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
        o = torch.optim.SGD([dict(params=[p1], lr=3e-5), dict(params=[p2], lr=5e-4)], lr=1.0)
        s = transformers.get_linear_schedule_with_warmup(o, num_warmup_steps=W, num_training_steps=T)
        for k in range(T + 1):
            mult = linear_schedule_with_warmup(k, W, T)
            assert [g["lr"] for g in o.param_groups] == [3e-5 * mult, 5e-4 * mult], (T, W, k)
            o.step()
            s.step()


def test_adam_symbols_are_exported():
    for sym in ("nbest_adam_clip_coef", "nbest_adam_update", "nbest_adam_step"):
        assert sym in hipabi.EXPORTS
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), sym)
    assert ctypes.sizeof(hipabi.TensorDesc) == 32
    assert (hipabi.ADAM_L2, hipabi.ADAMW) == (0, 1)


def test_adam_descriptors_carry_one_lr_and_the_l2_decay(labels):
    """torch Adam's single group: every descriptor holds lr and wd = l2; the default grouping is unchanged"""
    cfg = ncfg.bert_base(num_hidden_layers=1)
    a = ar.ParamArena(cfg, labels, "cpu", compute_dtype=torch.float32)

    def descs(**kw):
        dev, n, _ = a.build_descs(5e-4, 3e-5, **kw)
        raw = dev.numpy().tobytes()
        return list((hipabi.TensorDesc * n).from_buffer_copy(raw[:n * ctypes.sizeof(hipabi.TensorDesc)]))

    grouped = {s.name: d for s, d in zip(a.slots, descs())}
    assert grouped["bert_encoder.encoder.layer.0.output.dense.weight"].wd == pytest.approx(0.01)
    assert grouped["bert_encoder.encoder.layer.0.output.dense.bias"].wd == 0.0
    assert grouped["bert_encoder.encoder.layer.0.output.dense.weight"].lr == pytest.approx(3e-5)
    assert grouped["clf." + synth.head_param_shapes(labels, cfg.hidden_size)[0][0]].lr == pytest.approx(5e-4)
    dev, n, _ = a.build_descs(5e-4, 5e-4, wd=1e-3)
    uniform = list((hipabi.TensorDesc * n).from_buffer_copy(dev.numpy().tobytes()[:n * 32]))
    assert all(d.lr == pytest.approx(5e-4) and d.wd == pytest.approx(1e-3) for d in uniform)
    assert [d.active for d in uniform] == [d.active for d in grouped.values()]


def test_hipadam_refuses_an_unknown_kind():
    with pytest.raises(ValueError):
        HipAdam(None, kind="sgd")
