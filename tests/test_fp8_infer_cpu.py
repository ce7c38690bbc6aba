"""fp8 inference, the parts that answer without a GPU: the exports, the workspace size, the plan of NBEST_EPI_BIAS_GELU_Q8 and its
refusals, and the command line of --predict_fp8."""
import ctypes as C
import os
import re

import pytest

import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("nbest_fp8_amax_fold_max", "nbest_encoder_infer_fp8_ws_bytes", "nbest_encoder_infer_fp8")


def test_exports_agree():
    header = open(os.path.join(ROOT, "include", "nbest_hip.h")).read()
    lib = C.CDLL(hb.LIB_PATH)
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s + " is not declared in the header"
        assert s in hb.EXPORTS and hasattr(lib, s), s
    assert "NBEST_EPI_BIAS_GELU_Q8 = 7" in header and hb.EPI_BIAS_GELU_Q8 == 7


def _desc(B, S, H, F, heads, L):
    d = hb.EncoderDesc()
    d.dtype, d.B, d.S, d.H, d.L, d.heads, d.F = hb.BF16, B, S, H, L, heads, F
    return d


@pytest.mark.parametrize("B,S,H,F,heads", [(3, 40, 768, 3072, 12), (2, 64, 1024, 4096, 16)])
def test_workspace_adds_the_four_e4m3_regions(B, S, H, F, heads):
    sizes = []
    for L in (2, 12):
        d = _desc(B, S, H, F, heads, L)
        base, f8 = hb.lib().nbest_encoder_infer_ws_bytes(C.byref(d)), hb.lib().nbest_encoder_infer_fp8_ws_bytes(C.byref(d))
        assert f8 >= base + B * S * (3 * H + F), (base, f8)
        assert f8 <= base + B * S * (3 * H + F) + 4 * 256, "more than the four regions and their 256-byte alignment"
        sizes.append(f8)
    assert sizes[0] == sizes[1], "the workspace depends on L"


def _q8(M, N, K, **over):
    g = hb.GemmFp8Args()
    fake = 1 << 20
    g.A = g.B = g.bias = g.C8 = fake
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.ldu, g.ldc8, g.ldr = M, N, K, K, K, N, N, N, N
    g.epilogue, g.out_scale = hb.EPI_BIAS_GELU_Q8, 1.0
    for k, v in over.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("M,N,K", [(300, 3072, 768), (256, 768, 768)])
def test_q8_takes_the_plan_of_bias_gelu(M, N, K):
    assert hb.gemm_fp8_plan_args(_q8(M, N, K)) == hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU)
    assert hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU_Q8) == hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU)
    bn = hb.lib().nbest_pack_bn_fp8(N, K)
    assert hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU_Q8, packed_bn=bn) == \
        hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU, packed_bn=bn)


@pytest.mark.parametrize("over", [dict(C=1 << 20), dict(U=1 << 20), dict(c8_amax_new=1 << 20), dict(C8=None), dict(bias=None)])
def test_q8_plan_refusals(over):
    info = hb.GemmFp8PlanInfo()
    assert hb.lib().nbest_gemm_fp8_plan(C.byref(_q8(300, 3072, 768, **over)), C.byref(info)) == -1, over    # NBEST_ERR_ARG


def test_bf16_gemm_refuses_the_epilogue():
    with pytest.raises(RuntimeError, match="epilogue 7"):
        hb.gemm_plan_shape(256, 768, 768, epilogue=hb.EPI_BIAS_GELU_Q8)


# ---- command line ----------------------------------------------------------------------------------------------------------------
FILE = os.path.join(GOLDEN, "valid_head.txt")
BASE = ["--dataset", "dstc2", "--dataroot", GOLDEN, "--deviceId", "0", "--experiment", "exp", "--label_space", os.path.join(GOLDEN, "label_space.json")]


def _refused(argv, capsys, word):
    with pytest.raises(SystemExit) as e:
        cli.parse_arguments(BASE + argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_cli_accepts_predict_fp8():
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--dtype", "fp8w", "--predict_fp8"])
    assert opt.predict_fp8 and opt.fp8_calib_batches == 8
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--dtype", "fp8w", "--predict_fp8", "--fp8_calib_batches", "3"])
    assert opt.fp8_calib_batches == 3
    assert not cli.parse_arguments(BASE + ["--predict", FILE, "--dtype", "fp8w"]).predict_fp8


def test_cli_parse_errors(capsys, tmp_path):
    mask = tmp_path / "mask.json"
    mask.write_text("[[1]]")
    ok = ["--predict", FILE, "--dtype", "fp8w", "--predict_fp8"]
    _refused(["--dtype", "fp8w", "--predict_fp8"], capsys, "--predict FILE")
    _refused(["--predict", FILE, "--predict_fp8"], capsys, "--dtype fp8w")
    _refused(["--predict", FILE, "--dtype", "bf16", "--predict_fp8"], capsys, "--dtype fp8w")
    _refused(ok + ["--head_mask", str(mask)], capsys, "--head_mask")
    _refused(ok + ["--head_mask", str(mask), "--compact_heads"], capsys, "--compact_heads")
    _refused(ok + ["--predict_attention", str(tmp_path / "a.jsonl")], capsys, "--predict_attention")
    _refused(ok + ["--predict_attribution", str(tmp_path / "b.jsonl")], capsys, "--predict_attribution")
    _refused(ok + ["--fp8_calib_batches", "0"], capsys, "--fp8_calib_batches")
