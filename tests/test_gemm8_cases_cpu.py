"""nbest_gemm_fp8_plan / nbest_wgrad_fp8_plan (host only): every case of tests/gemm8_cases.py resolves to the tile, ring depth, split
count and last-split length it declares; every (bn, stages) and both weight-gradient paths have a case; the plan refuses what
nbest_gemm_fp8 refuses with the same code.  Runs without a GPU: the plans make no HIP call."""
import ctypes

import pytest

import nbest_amd  # noqa: F401
from nbest_amd import hipabi as hb

import gemm8_cases as g8

ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE = -1, -2, -4, -6        # include/nbest_hip.h


def test_error_codes_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbest_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"(NBEST_ERR_[A-Z]+)\s*=\s*(-?\d+)", text)}
    assert (codes["NBEST_ERR_ARG"], codes["NBEST_ERR_SHAPE"], codes["NBEST_ERR_ALIGN"], codes["NBEST_ERR_WORKSPACE"]) == \
        (ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE)


def test_every_case_resolves_to_the_tile_it_declares():
    for c in g8.ALL_CASES:
        for epi in c.epis:
            plan = hb.gemm_fp8_plan_shape(c.M, c.N, c.K, epi, drop_p=0.1 if c.drop else 0.0)
            assert g8.tile_of(plan) == c.tile, "%s resolves to %r" % (g8.case_id(c, epi), plan)
            assert plan["tiles_m"] == (c.M + 255) // 256 and plan["tiles_n"] == c.N // c.tile[0]
            if c.tiles_m is not None:
                assert plan["tiles_m"] == c.tiles_m, g8.case_id(c, epi)
            if c.group_cols is not None:
                assert plan["group_cols"] == c.group_cols and plan["tiles_n"] // plan["group_cols"] >= 2, g8.case_id(c, epi)
            assert plan["packed_taken"] == 0
            # strides change nothing; the packed operand is taken at the tile's own width with packed rows only
            wide = hb.gemm_fp8_plan_shape(c.M, c.N, c.K, epi, lda=c.K + 64, ldb=c.K + 64, ldc=c.N + 64, packed_bn=c.tile[0])
            assert g8.tile_of(wide) == c.tile and wide["packed_taken"] == 0
            assert hb.gemm_fp8_plan_shape(c.M, c.N, c.K, epi, packed_bn=c.tile[0])["packed_taken"] == 1
            assert hb.gemm_fp8_plan_shape(c.M, c.N, c.K, epi, packed_bn=384 - c.tile[0])["packed_taken"] == 0
    assert {c.tile for c in g8.EPILOGUE_CASES} == set(g8.ALL_TILES)
    for tile in g8.ALL_TILES:
        assert {e for c in g8.EPILOGUE_CASES if c.tile == tile for e in c.epis} == set(g8.ALL_EPIS)
        assert sorted(c.K // g8.BK for c in g8.SHORT_K_CASES if c.tile == tile and c.epis == (g8.BIAS,)) == list(g8.SHORT_K[tile])
        assert any(c.tile == tile and c.epis == (g8.DGELU,) and c.K == g8.BK for c in g8.SHORT_K_CASES)
        # fewer stages than the ring is deep (1 .. stages - 1), exactly as many, and more than one turn
        assert set(range(1, tile[1] + 1)) <= set(g8.SHORT_K[tile]) and max(g8.SHORT_K[tile]) > 2 * tile[1]
        assert sorted({c.M % 256 for c in g8.ROW_TAIL_CASES if c.tile == tile}) == [0, 1, 255]
        assert {(c.epis[0], c.drop) for c in g8.ROW_TAIL_CASES if c.tile == tile} == {(g8.BIAS_DROP_RES, True), (g8.DGELU, False)}
    # the 256 x 256 tile is reached both ways: by K > 1024 at a tile count the 128-column tile would take, and by the tile count at K <= 1024
    assert any(c.tile == g8.T256 and c.K > 1024 and c.N * ((c.M + 255) // 256) <= 3 * 128 * 256 for c in g8.EPILOGUE_CASES)
    assert any(c.tile == g8.T256 and c.K <= 1024 for c in g8.EPILOGUE_CASES)


def test_every_weight_gradient_case_resolves_to_the_split_it_declares():
    for c in g8.WGRAD_CASES:
        splits, kps = hb.wgrad_fp8_plan(c.M, c.N, c.K)
        assert kps % g8.BK == 0
        assert (splits == 1) == (c.path == g8.DIRECT), g8.wcase_id(c)
        assert splits == c.splits and g8.last_split(c.K, splits, kps) == c.last, "%s: %d splits of %d" % (g8.wcase_id(c), splits, kps)
        ws = hb.lib().nbest_wgrad_fp8_ws_bytes(c.M, c.N, c.K)
        assert ws == (splits * c.M * c.N * 4 if splits > 1 else 0)
    assert {c.path for c in g8.WGRAD_CASES} == {g8.DIRECT, g8.SPLIT}
    assert all(c.K < 1024 for c in g8.WGRAD_DIRECT_CASES)
    assert {(c.M, c.N) for c in g8.WGRAD_DIRECT_CASES} == {(256, 256), (768, 256)}
    assert {c.K for c in g8.WGRAD_DIRECT_CASES} == set(g8.DIRECT_KS) and {c.acc for c in g8.WGRAD_DIRECT_CASES} == {False, True}
    lasts = [c.last for c in g8.WGRAD_SPLIT_CASES]
    assert any(-(-n // g8.BK) < 4 for n in lasts), "no split case whose last split has fewer than 4 k-stages"
    assert any(n % g8.BK for n in lasts) and any(c.K % g8.BK for c in g8.WGRAD_SPLIT_CASES), "no split case with a ragged last split"
    # the pair: M = Ma + Mb virtual rows
    H, K = g8.PAIR_H, g8.PAIR_K
    splits, kps = hb.wgrad_fp8_plan(3 * H + H, H, K)
    assert splits == g8.PAIR_SPLITS > 1 and g8.last_split(K, splits, kps) == g8.PAIR_LAST
    assert hb.lib().nbest_wgrad_fp8_pair_ws_bytes(3 * H, H, H, K) == splits * 4 * H * H * 4
    assert hb.lib().nbest_wgrad_fp8_pair_ws_bytes(3 * H, H, H, 512) == 0          # one split: the pair does not fit


def test_pack_bn_is_the_plan_at_training_size():
    for N, K in g8.LAYER_SHAPES:
        assert hb.lib().nbest_pack_bn_fp8(N, K) == hb.gemm_fp8_plan_shape(32768, N, K)["bn"], (N, K)
    assert hb.lib().nbest_pack_bn_fp8(768, 768) == 128 and hb.lib().nbest_pack_bn_fp8(768, 3072) == 256
    assert hb.lib().nbest_pack_bn_fp8(800, 768) == 0


def _args(**over):
    g = hb.GemmFp8Args()
    fake = 1 << 20
    g.A = g.B = g.C = g.bias = fake
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = 512, 768, 768, 768, 768, 768
    g.ldr = g.ldu = g.ldc8 = 768
    g.epilogue, g.out_scale = hb.EPI_BIAS, 1.0
    for k, v in over.items():
        setattr(g, k, v)
    return g


FAKE = 1 << 20
REFUSALS = [
    ("null A", dict(A=None), ERR_ARG),
    ("null output", dict(C=None), ERR_ARG),
    ("null output with DGELU and no C8", dict(C=None, epilogue=hb.EPI_DGELU, U=FAKE), ERR_ARG),
    ("M = 0", dict(M=0), ERR_SHAPE),
    ("N not a multiple of 256", dict(N=640, ldc=640), ERR_SHAPE),
    ("K not a multiple of 64", dict(K=736), ERR_SHAPE),
    ("K = 0", dict(K=0), ERR_SHAPE),
    ("lda not a multiple of 16", dict(lda=776), ERR_ALIGN),
    ("ldb not a multiple of 16", dict(ldb=776), ERR_ALIGN),
    ("ldc not a multiple of 8", dict(ldc=772), ERR_ALIGN),
    ("unaligned A", dict(A=FAKE + 8), ERR_ALIGN),
    ("unaligned C", dict(C=FAKE + 8), ERR_ALIGN),
    ("epilogue not built", dict(epilogue=hb.EPI_F32_SPLITK), ERR_ARG),
    ("bias missing", dict(bias=None), ERR_ARG),
    ("BIAS_GELU without U", dict(epilogue=hb.EPI_BIAS_GELU, C8=FAKE), ERR_ARG),
    ("BIAS_GELU without C8", dict(epilogue=hb.EPI_BIAS_GELU, U=FAKE), ERR_ARG),
    ("RES without R", dict(epilogue=hb.EPI_RES), ERR_ARG),
    ("BIAS_DROP_RES with ldr not a multiple of 8", dict(epilogue=hb.EPI_BIAS_DROP_RES, R=FAKE, ldr=772), ERR_ARG),
    ("DGELU without U", dict(epilogue=hb.EPI_DGELU), ERR_ARG),
    ("DGELU with unaligned C8", dict(epilogue=hb.EPI_DGELU, U=FAKE, C8=FAKE + 4, c8_amax_new=FAKE), ERR_ARG),
    ("DGELU with C8 but no c8_amax_new", dict(epilogue=hb.EPI_DGELU, U=FAKE, C8=FAKE), ERR_ARG),
    ("DGELU column sums without a workspace", dict(epilogue=hb.EPI_DGELU, U=FAKE, colsum_out=FAKE), ERR_WORKSPACE),
    ("operand larger than 4 GiB", dict(M=1 << 23, lda=1024), ERR_SHAPE),
    ("dropout counter overflow", dict(M=1 << 23, N=768, epilogue=hb.EPI_BIAS_DROP_RES, R=FAKE, drop_p=0.1, lda=256, K=256, ldb=256), ERR_SHAPE),
]


@pytest.mark.parametrize("name,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_refuses_what_gemm_fp8_refuses(name, over, code):
    """the same argument block, the same code and message from both entries (a refused nbest_gemm_fp8 has made no HIP call: it answers
    without a GPU)"""
    L = hb.lib()
    g, info = _args(**over), hb.GemmFp8PlanInfo()
    assert L.nbest_gemm_fp8_plan(ctypes.byref(g), ctypes.byref(info)) == code, hb.last_error()
    msg = hb.last_error()
    assert L.nbest_gemm_fp8(ctypes.byref(g), None) == code
    assert hb.last_error() == msg
    with pytest.raises(RuntimeError):
        hb.gemm_fp8_plan_args(g)


def test_dgelu_copy_without_a_record_says_why():
    L = hb.lib()
    g, info = _args(epilogue=hb.EPI_DGELU, U=FAKE, C8=FAKE), hb.GemmFp8PlanInfo()
    assert L.nbest_gemm_fp8_plan(ctypes.byref(g), ctypes.byref(info)) == ERR_ARG
    assert "only where it records" in hb.last_error()
    g.c8_amax_new = FAKE
    assert L.nbest_gemm_fp8_plan(ctypes.byref(g), ctypes.byref(info)) == 0
    g.C = None                                                        # the e4m3 copy alone
    assert L.nbest_gemm_fp8_plan(ctypes.byref(g), ctypes.byref(info)) == 0


@pytest.mark.parametrize("M,N,K,code", [(0, 256, 64, ERR_ARG), (256, 256, 0, ERR_ARG), (300, 256, 64, ERR_SHAPE), (256, 128, 64, ERR_SHAPE)])
def test_wgrad_plan_refuses_what_wgrad_fp8_refuses(M, N, K, code):
    L = hb.lib()
    sp, kps = ctypes.c_int(0), ctypes.c_int64(0)
    assert L.nbest_wgrad_fp8_plan(M, N, K, ctypes.byref(sp), ctypes.byref(kps)) == code
    msg = hb.last_error()
    assert L.nbest_wgrad_fp8(FAKE, FAKE, FAKE, M, N, K, 256, 256, 256, None, None, 0, None, 0, None) == code
    assert hb.last_error() == msg
    assert L.nbest_wgrad_fp8_ws_bytes(M, N, K) == 0
    assert ctypes.sizeof(hb.GemmFp8PlanInfo) == 24
