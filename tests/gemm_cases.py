"""The bf16 GEMM kernel variants nbest_gemm can pick, and the parity case pinned to each.

One table, read by tests/test_gemm_plan_cpu.py (no GPU: every case must resolve to the variant it declares, and the variants the
encoder's GEMMs reach must all have a case) and by tests/test_gemm_variants_gpu.py (which runs them).  No torch here.

A VARIANT is what nbest_gemm_plan reports about the kernel instantiation, less the per-shape numbers:
    (generation, bm, bn, bk, wave_rows, wave_cols, stages, form, reg_epilogue)
A CASE is (variant, M, N, K, trans_a, trans_b) plus the epilogues to run on it.  Token counts are the smallest that still select
the variant (make_plan counts tiles against the 256 CUs), ragged by -88 rows unless the case is about the row tail itself.
"""
from collections import namedtuple

NONE, BIAS, BIAS_GELU, BIAS_DROP_RES, DGELU, RES, F32_SPLITK = range(7)      # include/nbest_hip.h NBEST_EPI_*
F32_SPLITK_ACC = 16 + F32_SPLITK                                             # test-side name: F32_SPLITK with accumulate = 1
NN, NT, TT = 0, 1, 2                                                          # NBEST_GEMM_FORM_*
EPI_NAMES = {NONE: "none", BIAS: "bias", BIAS_GELU: "bias_gelu", BIAS_DROP_RES: "bias_drop_res", DGELU: "dgelu_colsum", RES: "res",
             F32_SPLITK: "f32", F32_SPLITK_ACC: "f32_acc"}
FORM_NAMES = {NN: "NN", NT: "NT", TT: "TT"}

VARIANT_FIELDS = ("generation", "bm", "bn", "bk", "wave_rows", "wave_cols", "stages", "form", "reg_epilogue")


def variant_of(plan):
    """the variant tuple of a plan dict (hipabi.gemm_plan)"""
    return tuple(plan[f] for f in VARIANT_FIELDS)


def variant_name(v):
    gen, bm, bn, bk, wr, wc, st, form, reg = v
    return "v%d_%dx%d_%dx%dw_%dst_%s_%s" % (gen, bm, bn, wr, wc, st, FORM_NAMES[form], "reg" if reg else "lds")


# generation 2 (gemm_bf16_v2.hip): every instantiation gemm_v2_impl holds
V2_128x512 = (2, 128, 512, 32, 2, 4, 4, NN, 1)
V2_128x384_S4 = (2, 128, 384, 32, 2, 4, 4, NN, 1)
V2_128x384_S5 = (2, 128, 384, 32, 2, 4, 5, NN, 1)
V2_256x192_S4 = (2, 256, 192, 32, 4, 2, 4, NN, 1)
V2_256x192_S5 = (2, 256, 192, 32, 4, 2, 5, NN, 1)
V2_256x256_S4 = (2, 256, 256, 32, 4, 2, 4, NN, 1)
V2_256x256_S5 = (2, 256, 256, 32, 4, 2, 5, NN, 1)
V2_256x256_NN_F32 = (2, 256, 256, 32, 2, 4, 4, NN, 0)      # ABI only: no caller in the project issues F32_SPLITK on NN operands
V2_256x256_TT = (2, 256, 256, 32, 2, 4, 4, TT, 0)          # weight gradients
V2_RING_NN = (2, 256, 128, 32, 4, 1, 3, NN, 1)
V2_RING_NN_F32 = (2, 256, 128, 32, 2, 2, 3, NN, 0)         # ABI only
V2_RING_NT = (2, 256, 128, 32, 2, 2, 3, NT, 0)
# generation 1 (gemm_bf16.hip)
V1_NN = (1, 128, 128, 64, 2, 2, 2, NN, 0)
V1_NT = (1, 128, 128, 64, 2, 2, 2, NT, 0)
V1_TT = (1, 128, 128, 64, 2, 2, 2, TT, 0)

ALL_VARIANTS = (V2_128x512, V2_128x384_S4, V2_128x384_S5, V2_256x192_S4, V2_256x192_S5, V2_256x256_S4, V2_256x256_S5, V2_256x256_NN_F32,
                V2_256x256_TT, V2_RING_NN, V2_RING_NN_F32, V2_RING_NT, V1_NN, V1_NT, V1_TT)
ABI_ONLY = (V2_256x256_NN_F32, V2_RING_NN_F32)

Case = namedtuple("Case", "variant M N K ta tb epis")

PLAIN = (NONE, BIAS, BIAS_DROP_RES, RES)                    # what the 96-column wave tiles and the 128 x 512 tile are built / chosen for
ALL_BF16 = (NONE, BIAS, BIAS_GELU, BIAS_DROP_RES, DGELU, RES)


def case_id(c, epi=None):
    s = "%s-M%d-N%d-K%d" % (variant_name(c.variant), c.M, c.N, c.K)
    return s if epi is None else s + "-" + EPI_NAMES[epi]


# ---- every variant at full size: strided operands, poisoned padding, guarded outputs, every epilogue listed -------------------------
EPILOGUE_CASES = [
    # 128 x 512: the N = 1024 GEMMs of xlm-roberta-large from 64 rows of 256 up (K = 4096: FFN-down)
    Case(V2_128x512, 16296, 1024, 1024, 0, 0, PLAIN),
    Case(V2_128x512, 16296, 1024, 4096, 0, 0, PLAIN),
    # 128 x 384: the N = 768 GEMMs; 5 stages from K = 2048 (QKV dgrad K = 2304, FFN-down K = 3072)
    Case(V2_128x384_S4, 16296, 768, 768, 0, 0, PLAIN),
    Case(V2_128x384_S5, 16296, 768, 2304, 0, 0, PLAIN),
    Case(V2_128x384_S5, 16296, 768, 3072, 0, 0, PLAIN),
    # 256 x 192: N a multiple of 192 but not of 384 (no model width; the ABI accepts it)
    Case(V2_256x192_S4, 21928, 576, 768, 0, 0, PLAIN),
    Case(V2_256x192_S5, 21928, 576, 2048, 0, 0, PLAIN),
    # 256 x 256 with the register epilogue
    Case(V2_256x256_S4, 16296, 3072, 768, 0, 0, ALL_BF16),
    Case(V2_256x256_S5, 16296, 3072, 2048, 0, 0, ALL_BF16),
    Case(V2_256x256_S4, 16296, 1024, 768, 0, 0, (BIAS_GELU, DGELU)),      # N = 1024: the GELU epilogues stay off the 128 x 512 tile
    Case(V2_256x256_S5, 16296, 1024, 2048, 0, 0, (BIAS_GELU, DGELU)),
    # 256 x 128 ring: the heuristic cliff of xlm-roberta-large (130 rows of tiles: 520 tiles of 256 x 256 fill 68 % of their rounds)
    Case(V2_RING_NN, 33192, 1024, 1024, 0, 0, ALL_BF16),
    # 256 x 128 ring, B stored [K][N]: the dgrads on the weights as the forward reads them (no transposed arena)
    Case(V2_RING_NT, 10920, 3072, 768, 0, 1, ALL_BF16),
    # reachable through the ABI only
    Case(V2_RING_NN_F32, 33192, 1024, 1024, 0, 0, (F32_SPLITK,)),
    Case(V2_256x256_NN_F32, 16296, 1024, 1024, 0, 0, (F32_SPLITK,)),
    # weight gradient written directly (splits == 1), token count K shorter than the ring and ragged
    Case(V2_256x256_TT, 1536, 768, 40, 1, 1, (F32_SPLITK, F32_SPLITK_ACC)),
    Case(V2_256x256_TT, 1536, 768, 424, 1, 1, (F32_SPLITK, F32_SPLITK_ACC)),
    # generation 1
    Case(V1_NN, 200, 256, 64, 0, 0, ALL_BF16 + (F32_SPLITK,)),
    Case(V1_NN, 200, 256, 192, 0, 0, ALL_BF16 + (F32_SPLITK,)),
    Case(V1_NT, 200, 256, 64, 0, 1, ALL_BF16 + (F32_SPLITK,)),
    Case(V1_NT, 200, 256, 192, 0, 1, ALL_BF16 + (F32_SPLITK,)),
    Case(V1_TT, 256, 256, 1000, 1, 1, ALL_BF16 + (F32_SPLITK, F32_SPLITK_ACC)),
]

# the CLS-row GEMMs of nbest_encoder_infer: one row per utterance out of [B][S][H] (lda = ldr = S H)
CLS_STRIDE_CASE = Case(V1_NN, 64, 768, 768, 0, 0, (BIAS, BIAS_DROP_RES))
CLS_ROW_STRIDE = 128 * 768


# ---- short and wrapping K: 1, 2, .. STAGES + 1 and 2 STAGES + 1 k-stages of 32, EPI_BIAS, packed rows ----------------------------------
# (the 5-stage instantiations are chosen from K = 2048 = 64 k-stages on: no argument block gives them fewer)
def _short_ks(stages):
    return [32 * n for n in list(range(1, stages + 2)) + [2 * stages + 1]]


SHORT_K_CASES = [Case(v, M, N, K, 0, tb, (BIAS,))
                 for v, M, N, tb in ((V2_128x512, 16296, 1024, 0), (V2_128x384_S4, 16296, 768, 0), (V2_256x192_S4, 21928, 576, 0),
                                     (V2_256x256_S4, 16296, 3072, 0), (V2_RING_NN, 33192, 1024, 0), (V2_RING_NT, 10920, 3072, 1))
                 for K in _short_ks(v[6])]


# ---- row tails: M mod bm in {1, bm - 1, 0}, one epilogue per variant, packed rows ---------------------------------------------------------
# (all three inside the last of `rows` tile rows, so that the tile count - and with it the plan - is the same)
def _tails(v, rows, N, K, ta, tb, epi):
    bm = v[1]
    return [Case(v, M, N, K, ta, tb, (epi,)) for M in ((rows - 1) * bm + 1, rows * bm - 1, rows * bm)]


ROW_TAIL_CASES = (
    _tails(V2_128x512, 128, 1024, 1024, 0, 0, BIAS_DROP_RES) + _tails(V2_128x384_S4, 128, 768, 768, 0, 0, BIAS_DROP_RES) +
    _tails(V2_128x384_S5, 128, 768, 2304, 0, 0, RES) + _tails(V2_256x192_S4, 86, 576, 768, 0, 0, BIAS_DROP_RES) +
    _tails(V2_256x192_S5, 86, 576, 2048, 0, 0, RES) + _tails(V2_256x256_S4, 64, 3072, 768, 0, 0, BIAS_GELU) +
    _tails(V2_256x256_S5, 64, 3072, 2048, 0, 0, DGELU) + _tails(V2_RING_NN, 130, 1024, 1024, 0, 0, BIAS_DROP_RES) +
    _tails(V2_RING_NT, 43, 3072, 768, 0, 1, RES) + _tails(V2_RING_NN_F32, 130, 1024, 1024, 0, 0, F32_SPLITK) +
    _tails(V2_256x256_NN_F32, 64, 1024, 1024, 0, 0, F32_SPLITK) +
    _tails(V1_NN, 2, 256, 192, 0, 0, BIAS_DROP_RES) + _tails(V1_NT, 2, 256, 192, 0, 1, DGELU))
# (the TT forms take whole tiles of M: M is a weight matrix's row count there, and the ragged dimension is K - above)

ALL_CASES = EPILOGUE_CASES + [CLS_STRIDE_CASE] + SHORT_K_CASES + ROW_TAIL_CASES


def plan_kwargs(c, epi):
    """keyword arguments of hipabi.gemm_plan_shape for (case, epilogue) with packed rows"""
    e = F32_SPLITK if epi == F32_SPLITK_ACC else epi
    return dict(M=c.M, N=c.N, K=c.K, trans_a=bool(c.ta), trans_b=bool(c.tb), epilogue=e, colsum=(epi == DGELU),
                accumulate=(epi == F32_SPLITK_ACC))
