"""nbest_gemm_plan (host only): which bf16 GEMM kernel variants the encoder's GEMMs reach, that every one of them - and every
instantiation the library holds - has a parity case in tests/gemm_cases.py, where the per-shape heuristics change variant, and
that the plan refuses what nbest_gemm refuses with the same code.  Runs without a GPU: the plan makes no HIP call."""
import ctypes

import pytest

import nbest_amd  # noqa: F401
from nbest_amd import config as ncfg, hipabi as hb

import gemm_cases as gc

ERR_ARG, ERR_SHAPE, ERR_ALIGN = -1, -2, -4                   # include/nbest_hip.h

FAMILIES = {"bert-base": ncfg.bert_base, "xlm-roberta-base": ncfg.xlmr_base, "xlm-roberta-large": ncfg.xlmr_large}
TOKENS = range(128, 65536 + 1, 128)
S_INFER = 128                                                 # sequence length of the CLS-row GEMMs (M = tokens / S utterances)


def layer_gemms(H, F, M):
    """every nbest_gemm a layer issues on M tokens (csrc/encoder.hip), as (kind, gemm_plan_shape keywords)"""
    pack = hb.lib().nbest_pack_bn
    fwd = [(3 * H, H, hb.EPI_BIAS, {}), (H, H, hb.EPI_BIAS_DROP_RES, {}), (F, H, hb.EPI_BIAS_GELU, {}), (H, F, hb.EPI_BIAS_DROP_RES, {})]
    dgrad = [(F, H, hb.EPI_DGELU, {"colsum": True}), (H, F, hb.EPI_RES, {}), (H, H, hb.EPI_NONE, {}), (H, 3 * H, hb.EPI_RES, {})]
    out = [("forward", dict(M=M, N=N, K=K, epilogue=e, packed_bn=pack(N), **kw)) for N, K, e, kw in fwd]
    out += [("dgrad", dict(M=M, N=N, K=K, epilogue=e, packed_bn=pack(N), **kw)) for N, K, e, kw in dgrad]       # on the transposed arena
    out += [("dgrad b_kn", dict(M=M, N=N, K=K, epilogue=e, trans_b=True, **kw)) for N, K, e, kw in dgrad]      # wts_t == NULL
    out += [("wgrad", dict(M=R, N=C, K=M, trans_a=True, trans_b=True, epilogue=hb.EPI_F32_SPLITK))
            for R, C in ((3 * H, H), (H, H), (F, H), (H, F))]
    B, SH = max(M // S_INFER, 1), S_INFER * H                  # nbest_encoder_infer, last layer: K | V on all rows, the rest on the CLS rows
    out += [("cls", dict(M=M, N=2 * H, K=H, epilogue=hb.EPI_BIAS)),
            ("cls", dict(M=B, N=H, K=H, epilogue=hb.EPI_BIAS, lda=SH)),
            ("cls", dict(M=B, N=H, K=H, epilogue=hb.EPI_BIAS_DROP_RES, ldr=SH)),
            ("cls", dict(M=B, N=F, K=H, epilogue=hb.EPI_BIAS_GELU, with_u=False)),
            ("cls", dict(M=B, N=H, K=F, epilogue=hb.EPI_BIAS_DROP_RES))]
    return out


# The variants each family's GEMMs reach at 128 .. 65 536 tokens, and by which GEMMs.  DESIGN.md section 4 ("used for") says the same in
# words; a change of make_plan that moves a model shape onto another kernel shows up here as a diff.
_BASE = {
    gc.V1_NN: {"cls", "dgrad", "forward"}, gc.V1_NT: {"dgrad b_kn"}, gc.V1_TT: {"wgrad"},
    gc.V2_128x384_S4: {"cls", "dgrad", "forward"}, gc.V2_128x384_S5: {"dgrad", "forward"}, gc.V2_128x512: {"cls"},
    gc.V2_RING_NT: {"dgrad b_kn"}, gc.V2_RING_NN: {"cls", "dgrad", "forward"}, gc.V2_256x256_TT: {"wgrad"},
    gc.V2_256x256_S4: {"dgrad", "forward"}, gc.V2_256x256_S5: {"dgrad", "forward"},
}
LIVE = {
    "bert-base": _BASE,
    "xlm-roberta-base": _BASE,
    "xlm-roberta-large": {
        gc.V1_NN: {"cls", "dgrad", "forward"}, gc.V1_NT: {"dgrad b_kn"}, gc.V1_TT: {"wgrad"},
        gc.V2_128x384_S4: {"forward"},                        # QKV: N = 3072 = 8 x 384
        gc.V2_128x512: {"cls", "dgrad", "forward"}, gc.V2_RING_NT: {"dgrad b_kn"}, gc.V2_RING_NN: {"cls", "dgrad", "forward"},
        gc.V2_256x256_TT: {"wgrad"}, gc.V2_256x256_S4: {"dgrad", "forward"},
    },
}


def _live(family):
    cfg = FAMILIES[family]()
    H, F = cfg.hidden_size, cfg.intermediate_size
    live = {}
    for M in TOKENS:
        for kind, kw in layer_gemms(H, F, M):
            live.setdefault(gc.variant_of(hb.gemm_plan_shape(**kw)), set()).add(kind)
    return live


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_live_variants_are_pinned_and_have_parity_cases(family):
    live = _live(family)
    named = {gc.variant_name(v): sorted(k) for v, k in live.items()}
    assert named == {gc.variant_name(v): sorted(k) for v, k in LIVE[family].items()}
    declared = {c.variant for c in gc.EPILOGUE_CASES}
    missing = [gc.variant_name(v) for v in live if v not in declared]
    assert not missing, "live kernel variants without a parity case in tests/gemm_cases.py: %s" % missing


def test_every_case_resolves_to_the_variant_it_declares():
    assert {c.variant for c in gc.EPILOGUE_CASES} == set(gc.ALL_VARIANTS)
    for c in gc.ALL_CASES:
        for epi in c.epis:
            kw = gc.plan_kwargs(c, epi)
            if c is gc.CLS_STRIDE_CASE:
                kw.update(lda=gc.CLS_ROW_STRIDE, ldr=gc.CLS_ROW_STRIDE)
            plan = hb.gemm_plan_shape(**kw)
            assert gc.variant_of(plan) == c.variant, "%s resolves to %s" % (gc.case_id(c, epi), gc.variant_name(gc.variant_of(plan)))
            # strides change nothing (the GPU test runs the full-size cases on windows of wider buffers)
            wide = dict(kw, lda=(c.M if c.ta else c.K) + 64, ldb=(c.N if c.tb else c.K) + 64, ldc=c.N + 64, ldr=c.N + 128, ldu=c.N + 64)
            if c is not gc.CLS_STRIDE_CASE:
                assert gc.variant_of(hb.gemm_plan_shape(**wide)) == c.variant
    # the short-K cases run fewer k-stages than the ring is deep, up to one more than twice its depth
    for v in {c.variant for c in gc.SHORT_K_CASES}:
        ks = sorted(c.K // 32 for c in gc.SHORT_K_CASES if c.variant == v)
        assert ks == list(range(1, v[6] + 2)) + [2 * v[6] + 1]
    # direct-write weight gradient: one split; the packed operand is used on every k-contiguous generation-2 tile of a packed width
    for c in gc.EPILOGUE_CASES:
        if c.variant == gc.V2_256x256_TT:
            assert hb.gemm_plan_shape(**gc.plan_kwargs(c, gc.F32_SPLITK))["splits"] == 1
        if c.variant[0] == 2 and c.variant[8] and c.N % 192 == 0 or c.variant in (gc.V2_128x512, gc.V2_256x256_S4, gc.V2_256x256_S5):
            bn = hb.lib().nbest_pack_bn(c.N)
            assert bn and hb.gemm_plan_shape(packed_bn=bn, **gc.plan_kwargs(c, c.epis[0]))["b_packed"] == 1, gc.case_id(c)


def _transitions(**kw):
    prev, out = None, []
    for M in TOKENS:
        v = gc.variant_of(hb.gemm_plan_shape(M=M, **kw))
        if v != prev:
            out.append((M, v))
        prev = v
    return out


def test_heuristic_cliffs_are_written_down():
    """token counts (steps of 128) from which a layer GEMM runs on another variant"""
    # bert-base / xlm-roberta-base, N = 768 (attention output forward): generation 1 again between 129 and 145 rows of 256 tokens
    assert _transitions(N=768, K=768, epilogue=hb.EPI_BIAS_DROP_RES) == [
        (128, gc.V1_NN), (16256, gc.V2_128x384_S4), (16512, gc.V1_NN), (21888, gc.V2_128x384_S4), (32896, gc.V1_NN),
        (37248, gc.V2_256x256_S4), (43648, gc.V2_128x384_S4), (49280, gc.V2_RING_NN), (55680, gc.V2_256x256_S4)]
    # FFN-up forward, N = 3072
    assert _transitions(N=3072, K=768, epilogue=hb.EPI_BIAS_GELU) == [
        (128, gc.V1_NN), (9344, gc.V2_256x256_S4), (10880, gc.V2_RING_NN), (13952, gc.V2_256x256_S4), (16512, gc.V2_RING_NN),
        (18560, gc.V2_256x256_S4)]
    # the dgrads on the forward's weights (b_kn): the ring from 43 rows of tiles at N = 3072, from 171 at N = 768
    assert _transitions(N=3072, K=768, epilogue=hb.EPI_DGELU, colsum=True, trans_b=True) == [(128, gc.V1_NT), (10880, gc.V2_RING_NT)]
    assert _transitions(N=768, K=3072, epilogue=hb.EPI_RES, trans_b=True) == [(128, gc.V1_NT), (43648, gc.V2_RING_NT)]
    # xlm-roberta-large, N = 1024: 128 x 512 tiles up to 128 rows of tiles, the 256 x 128 ring from 129 (516 tiles of 256 x 256: 67 % full rounds)
    large = _transitions(N=1024, K=1024, epilogue=hb.EPI_BIAS_DROP_RES)
    assert large == [(128, gc.V1_NN), (16256, gc.V2_128x512), (16512, gc.V1_NN), (27776, gc.V2_128x512), (32896, gc.V2_RING_NN),
                     (41856, gc.V2_128x512), (49280, gc.V2_RING_NN), (55680, gc.V2_128x512)]
    plan = lambda M: gc.variant_of(hb.gemm_plan_shape(M=M, N=1024, K=1024, epilogue=hb.EPI_BIAS_DROP_RES))   # noqa: E731
    assert plan(128 * 256) == gc.V2_128x512 and plan(130 * 256) == gc.V2_RING_NN
    assert _transitions(N=4096, K=1024, epilogue=hb.EPI_BIAS_GELU) == [
        (128, gc.V1_NN), (3968, gc.V2_256x256_S4), (4224, gc.V1_NN), (7040, gc.V2_256x256_S4), (8320, gc.V2_RING_NN),
        (10368, gc.V2_256x256_S4), (12416, gc.V2_RING_NN), (13952, gc.V2_256x256_S4)]


def test_every_built_instantiation_is_reachable_and_nothing_else():
    """Sweep of the argument blocks nbest_gemm accepts - N over the multiples of 64 up to 4096, every count of 256-token tile rows up to
    65 536 tokens (ragged and whole), the three operand forms, one epilogue of every class make_plan tells apart, K below and above the
    5-stage threshold: the variants reached are exactly those gemm_cases declares (= the instantiations gemm_v2_impl and nbest_gemm_bf16
    hold).  An instantiation nothing reaches, or a plan without a built kernel, fails here."""
    L = hb.lib()
    g, info = hb.GemmArgs(), hb.GemmPlanInfo()
    fake = 1 << 20
    g.A = g.B = g.C = g.bias = g.R = g.U = g.ws = fake
    g.ws_bytes = 1 << 62
    g.dtype = hb.BF16
    reached, refused = set(), set()

    def plan(M, N, K, ta, tb):
        g.M, g.N, g.K, g.trans_a, g.trans_b = M, N, K, ta, tb
        g.lda, g.ldb, g.ldc = (M if ta else K), (N if tb else K), N
        g.ldr = g.ldu = N
        rc = L.nbest_gemm_plan(ctypes.byref(g), ctypes.byref(info))
        if rc:
            refused.add((rc, N % 128 == 0))
        else:
            reached.add(tuple(getattr(info, f) for f in gc.VARIANT_FIELDS))

    for epi, colsum in ((hb.EPI_NONE, 0), (hb.EPI_BIAS_GELU, 0), (hb.EPI_DGELU, 1), (hb.EPI_F32_SPLITK, 0)):
        g.epilogue, g.colsum_out = epi, (fake if colsum else None)
        for N in range(64, 4096 + 1, 64):
            for tb in (0, 1):
                for K in (1024, 2048):
                    for rows in range(1, 257):
                        plan(rows * 256 - 88, N, K, 0, tb)
                        plan(rows * 256, N, K, 0, tb)
            for rows in range(128, 4096 + 1, 128):            # weight gradients: (rows, N) the matrix, K the tokens (ragged and whole)
                plan(rows, N, 424, 1, 1)
                plan(rows, N, 32768, 1, 1)
    assert {gc.variant_name(v) for v in reached} == {gc.variant_name(v) for v in gc.ALL_VARIANTS}
    # the only refusal in the sweep: a column count that generation 1 (128-column tiles) cannot tile
    assert refused == {(ERR_SHAPE, False)}


def _args(**over):
    g = hb.GemmArgs()
    fake = 1 << 20
    g.A = g.B = g.C = g.bias = fake
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = 512, 768, 768, 768, 768, 768
    g.dtype, g.epilogue = hb.BF16, hb.EPI_BIAS
    for k, v in over.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("name,over,code", [
    ("N not a multiple of 64", dict(N=800, ldc=800), ERR_SHAPE),
    ("N not a multiple of the generation-1 tile", dict(N=192, ldc=192), ERR_SHAPE),
    ("N not a multiple of the generation-2 tile", dict(M=70000, N=320, ldc=320), ERR_SHAPE),
    ("K not a multiple of bk (generation 1)", dict(K=96, lda=96, ldb=96), ERR_SHAPE),
    ("K not a multiple of bk (generation 2)", dict(M=20000, N=3072, ldc=3072, K=784, lda=784, ldb=784), ERR_SHAPE),
    ("trans_a without trans_b", dict(trans_a=1, lda=512), ERR_ARG),
    ("lda not a multiple of 8", dict(lda=772), ERR_ALIGN),
    ("ldc not a multiple of 8", dict(ldc=772), ERR_ALIGN),
    ("unaligned pointer", dict(B=(1 << 20) + 8), ERR_ALIGN),
    ("epilogue operand missing", dict(epilogue=hb.EPI_RES), ERR_ARG),
    ("bad shape", dict(M=0), ERR_SHAPE),
])
def test_plan_refuses_what_gemm_refuses(name, over, code):
    """the same argument block, the same code from both entries (a refused nbest_gemm has made no HIP call: it answers without a GPU)"""
    L = hb.lib()
    g, info = _args(**over), hb.GemmPlanInfo()
    assert L.nbest_gemm_plan(ctypes.byref(g), ctypes.byref(info)) == code, hb.last_error()
    msg = hb.last_error()
    assert L.nbest_gemm(ctypes.byref(g), None) == code
    assert hb.last_error() == msg
    with pytest.raises(RuntimeError):
        hb.gemm_plan_args(g)


def test_plan_of_the_fp32_path_and_of_an_accepted_block():
    info = hb.gemm_plan_shape(300, 200, 100, dtype=hb.F32, epilogue=hb.EPI_BIAS)
    assert info["generation"] == 0 and (info["bm"], info["bn"], info["bk"]) == (64, 64, 16) and info["splits"] == 1
    plan = hb.gemm_plan_shape(32768, 768, 3072, epilogue=hb.EPI_BIAS_DROP_RES, packed_bn=192)
    assert gc.variant_of(plan) == gc.V2_128x384_S5 and plan["b_packed"] == 1 and plan["kernel_epilogue"] == hb.EPI_BIAS_DROP_RES
    plan = hb.gemm_plan_shape(16, 3072, 768, epilogue=hb.EPI_BIAS_GELU, with_u=False)
    assert gc.variant_of(plan) == gc.V1_NN and plan["kernel_epilogue"] == hb.EPI_BIAS_GELU_NO_U
    # a weight gradient: the split-K plan of the workspace query (tests/test_host_cpu.py pins the split counts)
    plan = hb.gemm_plan_shape(2304, 768, 32768, trans_a=True, trans_b=True, epilogue=hb.EPI_F32_SPLITK)
    assert gc.variant_of(plan) == gc.V2_256x256_TT and plan["splits"] == 9 and plan["k_per_split"] * 9 >= 32768
    assert ctypes.sizeof(hb.GemmPlanInfo) == 56
