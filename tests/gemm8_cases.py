"""The fp8 GEMM kernels (csrc/gemm_fp8.hip) and the parity case pinned to each path through them.

One table, read by tests/test_gemm8_cases_cpu.py (no GPU: every case must resolve, through nbest_gemm_fp8_plan / nbest_wgrad_fp8_plan,
to the tile, ring depth, split count and last-split length it declares) and by tests/test_gemm_fp8_variants_gpu.py (which runs them).
No torch here.

A TILE is (bn, stages) of gemm8_kernel<EPI, WN>: T128 = 256 x 128 on a 3-stage ring (WN = 2), T256 = 256 x 256 on the 4-stage ping-pong
ring (WN = 4).  M is the smallest row count that selects the tile, ragged by -88 rows unless the case is about the row tail.
"""
from collections import namedtuple

NONE, BIAS, BIAS_GELU, BIAS_DROP_RES, DGELU, RES = range(6)                   # include/nbest_hip.h NBEST_EPI_*
EPI_NAMES = {NONE: "none", BIAS: "bias", BIAS_GELU: "bias_gelu", BIAS_DROP_RES: "bias_drop_res", DGELU: "dgelu_colsum", RES: "res"}
ALL_EPIS = (NONE, BIAS, BIAS_GELU, BIAS_DROP_RES, DGELU, RES)
FORWARD_EPIS = (BIAS, BIAS_GELU, BIAS_DROP_RES)                               # scale target of a_amax: 224; the others (dgrads): 56

T128, T256 = (128, 3), (256, 4)
ALL_TILES = (T128, T256)
BK = 64                                                                       # k-bytes of one ring stage

# a forward / dgrad case; group_cols / tiles_m: asserted from the plan where not None; drop: BIAS_DROP_RES runs with dropout on
Case = namedtuple("Case", "tile M N K epis group_cols tiles_m drop")
Case.__new__.__defaults__ = (None, None, False)


def tile_of(plan):
    return (plan["bn"], plan["stages"])


def case_id(c, epi=None):
    s = "T%d-M%d-N%d-K%d" % (c.tile[0], c.M, c.N, c.K)
    return s if epi is None else s + "-" + EPI_NAMES[epi]


# ---- all six epilogues, strided operands, poisoned padding, guarded outputs --------------------------------------------------------
EPILOGUE_CASES = [
    Case(T128, 424, 768, 768, ALL_EPIS, drop=True),
    Case(T128, 200, 256, 192, ALL_EPIS, drop=True),
    Case(T256, 424, 768, 3072, ALL_EPIS, drop=True),                           # 256 x 256 by long K (K > 1024)
    Case(T256, 200, 256, 1088, ALL_EPIS, drop=True),
    # 256 x 256 by tile count: 33 tile rows x 12 tile columns in two L2 groups of 6 (nb_tile_coords with tiles_m > 1, two groups)
    Case(T256, 8360, 3072, 768, ALL_EPIS, group_cols=6, tiles_m=33, drop=True),
]

# ---- short and wrapping K, EPI_BIAS (packed and plain wherever the plan takes the packed operand) ------------------------------------
SHORT_K = {T256: (1, 2, 3, 4, 5, 9), T128: (1, 2, 3, 4, 7)}                   # k-stages against the 4- / 3-stage ring
SHORT_K_CASES = ([Case(T256, 8360, 3072, BK * n, (BIAS,), tiles_m=33) for n in SHORT_K[T256]] +
                 [Case(T128, 424, 768, BK * n, (BIAS,)) for n in SHORT_K[T128]] +
                 [Case(T256, 8360, 3072, BK, (DGELU,), tiles_m=33), Case(T128, 424, 768, BK, (DGELU,))])


# ---- row tails: M mod 256 in {1, 255, 0} inside the last of `rows` tile rows (the same tile count, the same plan) -----------------------
def _tails(tile, rows, N, K, epi, drop=False):
    return [Case(tile, M, N, K, (epi,), tiles_m=rows, drop=drop) for M in ((rows - 1) * 256 + 1, rows * 256 - 1, rows * 256)]


ROW_TAIL_CASES = (_tails(T128, 2, 768, 768, BIAS_DROP_RES, drop=True) + _tails(T128, 2, 768, 768, DGELU) +
                  _tails(T256, 2, 256, 1088, BIAS_DROP_RES, drop=True) + _tails(T256, 2, 256, 1088, DGELU))

ALL_CASES = EPILOGUE_CASES + SHORT_K_CASES + ROW_TAIL_CASES

# ---- weight gradients (gemm8tt_kernel): M x N the output, K the token count ----------------------------------------------------------
DIRECT, SPLIT = "direct", "split"
# splits / last: the split count and the token count of the last split, asserted from nbest_wgrad_fp8_plan (None: any)
WCase = namedtuple("WCase", "path M N K acc splits last")
WCase.__new__.__defaults__ = (None, None)

DIRECT_KS = (40, 64, 128, 192, 256, 320, 424, 576)                            # ragged, 1 .. 9 k-stages against the 4-stage ring
WGRAD_DIRECT_CASES = [WCase(DIRECT, M, 256, K, acc, 1, K) for M in (256, 768) for K in DIRECT_KS for acc in (False, True)]
WGRAD_SPLIT_CASES = [
    WCase(SPLIT, 256, 256, 4160, False, 8, 128),                              # last split: two k-stages, fewer than the ring holds
    WCase(SPLIT, 256, 256, 4160, True, 8, 128),
    WCase(SPLIT, 768, 256, 1320, False, 2, 616),                              # last split ragged: K is no multiple of 64
    WCase(SPLIT, 768, 256, 1320, True, 2, 616),
]
WGRAD_CASES = WGRAD_DIRECT_CASES + WGRAD_SPLIT_CASES
# the pair: Q|K|V ([3H][H], rows of dQ|dK|dV with leading dimension 3H) + attention output ([H][H]); K such that the pair splits
PAIR_H, PAIR_K = 256, 1320
PAIR_SPLITS, PAIR_LAST = 2, 616


def wcase_id(c):
    return "%s-M%d-N%d-K%d%s" % (c.path, c.M, c.N, c.K, "-acc" if c.acc else "")


def last_split(K, splits, k_per_split):
    """token count of the last split"""
    return K - (splits - 1) * k_per_split


# ---- the layer shapes (bert-base / xlm-roberta-base, xlm-roberta-large): (N, K) of the forward and of the dgrad GEMMs ----------------
LAYER_SHAPES = [(3 * H, H) for H in (768, 1024)] + [(H, H) for H in (768, 1024)] + [(4 * H, H) for H in (768, 1024)] + \
               [(H, 4 * H) for H in (768, 1024)] + [(H, 3 * H) for H in (768, 1024)]
