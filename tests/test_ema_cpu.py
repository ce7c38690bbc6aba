"""CPU tests of --ema_decay: the C ABI exports and hipabi binds the two weight-EMA entry points, the decay warm-up, and the
command-line surface (parsing, the refused combinations, the experiment-directory name) - device-free."""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi
from nbest_amd.optim import HipAdam, HipBertAdam, ema_decay_at

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]


def test_ema_symbols_are_exported_and_bound():
    """int nbest_ema_update(float* ema, const float* p, const nbest_tensor_desc*, int n_tensors, int n_blocks, float w, stream)
    int nbest_ema_exchange(float* p, float* ema, void* p_lowp, const nbest_tensor_desc*, int n_tensors, int n_blocks, stream)"""
    raw = ctypes.CDLL(hipabi.LIB_PATH)
    for sym in ("nbest_ema_update", "nbest_ema_exchange"):
        assert sym in hipabi.EXPORTS
        assert hasattr(raw, sym)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L = hipabi.lib()
    assert list(L.nbest_ema_update.argtypes) == [vp, vp, vp, i32, i32, f32, vp]
    assert list(L.nbest_ema_exchange.argtypes) == [vp, vp, vp, vp, i32, i32, vp]
    assert L.nbest_ema_update.restype is ctypes.c_int and L.nbest_ema_exchange.restype is ctypes.c_int


def test_ema_entry_points_check_their_arguments_on_the_host():
    """a NULL pointer, n_tensors <= 0 or n_blocks <= 0: NBEST_ERR_ARG (-1) and a message, before anything touches a device"""
    L = hipabi.lib()
    fake = ctypes.c_void_p(1 << 20)
    null = ctypes.c_void_p(0)
    for args in ((null, fake, fake, 1, 1), (fake, null, fake, 1, 1), (fake, fake, null, 1, 1), (fake, fake, fake, 0, 1),
                 (fake, fake, fake, 1, 0), (fake, fake, fake, -1, 1)):
        assert L.nbest_ema_update(*args, 0.5, null) == -1
        assert "ema_update" in hipabi.last_error()
    for args in ((null, fake, fake, fake, 1, 1), (fake, null, fake, fake, 1, 1), (fake, fake, fake, null, 1, 1),
                 (fake, fake, null, fake, 0, 1), (fake, fake, null, fake, 1, 0)):
        assert L.nbest_ema_exchange(*args, null) == -1
        assert "ema_exchange" in hipabi.last_error()


def test_ema_decay_warm_up():
    assert ema_decay_at(1, 0.99) == pytest.approx(2.0 / 11.0, rel=1e-15)
    assert ema_decay_at(90, 0.9) == 0.9
    assert ema_decay_at(89, 0.9) == 0.9                      # 90 / 99 > 0.9
    assert ema_decay_at(80, 0.9) == pytest.approx(81.0 / 90.0, rel=1e-15) and ema_decay_at(80, 0.9) < 0.9 + 1e-15
    for decay in (0.0, 0.5, 0.9, 0.999, 0.9999):
        vals = [ema_decay_at(t, decay) for t in range(1, 20001)]
        assert all(b >= a for a, b in zip(vals, vals[1:])), decay          # monotone in t
        assert all(0.0 <= v <= decay for v in vals), decay
        assert decay >= 0.9999 or vals[-1] == decay


def test_cli_ema_decay_flag(tmp_path):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    opt = cli.parse_arguments(BASE + ["--ema_decay", "0.99"])
    assert opt.ema_decay == 0.99
    assert cli.parse_arguments(BASE + ["--ema_decay", "0"]).ema_decay == 0.0
    assert cli.parse_arguments(BASE).ema_decay is None
    for bad in (["--ema_decay", "1"], ["--ema_decay", "1.5"], ["--ema_decay", "-0.1"], ["--ema_decay", "nan"],
                ["--ema_decay", "0.99", "--shard_optimizer", "on"],
                ["--ema_decay", "0.99", "--testing"],
                ["--ema_decay", "0.99", "--predict", str(src)],
                ["--ema_decay", "0.99", "--head_importance", str(tmp_path / "imp.json")]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
    # the combinations are fine without the flag
    for ok in (["--shard_optimizer", "on"], ["--testing"], ["--predict", str(src)], ["--head_importance", str(tmp_path / "imp.json")]):
        assert cli.parse_arguments(BASE + ok).ema_decay is None


def test_exp_dir_moves_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert plain.endswith("__score_pp__repr_bin_sa_cls__cls_stc") and "ema" not in plain
    with_flag = cli.exp_dir(cli.parse_arguments(BASE + ["--ema_decay", "0.99"]))
    assert with_flag == plain + "__ema_0.99"
    frozen = cli.exp_dir(cli.parse_arguments(BASE + ["--ema_decay", "0.5", "--freeze_layers", "1"]))
    assert frozen == plain + "__fz_none_1__ema_0.5"


@pytest.mark.parametrize("bad", [1.0, -0.5, 2])
def test_optimizers_refuse_a_decay_outside_the_range(bad):
    """checked before the model is touched"""
    with pytest.raises(ValueError, match="ema_decay"):
        HipBertAdam(None, lr=1e-3, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        HipAdam(None, kind="adamw", ema_decay=bad)


def test_optimizers_refuse_the_sharded_form():
    with pytest.raises(ValueError, match="shard"):
        HipBertAdam(None, lr=1e-3, shard=True, ema_decay=0.9)
    with pytest.raises(ValueError, match="shard"):
        HipAdam(None, kind="adam", shard=True, ema_decay=0.9)
