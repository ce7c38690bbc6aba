"""Every path through the fp8 GEMM kernels (csrc/gemm_fp8.hip; the cases of tests/gemm8_cases.py), each against an fp64 reference of
the same operation on the same e4m3 bytes, element by element.

  * a case asserts through nbest_gemm_fp8_plan / nbest_wgrad_fp8_plan that it runs the tile / split it names before it launches;
  * reference: acc = A8 . W8^T and mag = |A8| . |W8|^T in fp64 from the dequantised bytes (every product of two e4m3 values is exact),
    both carried through the epilogue; bounds per element, u = 2^-23, K the summed length, G the one factor of this file:
        bf16 outputs   |got - ref| <= 2^-8 |ref| + G (K + 8) u mag_epi
        fp32 outputs   |got - ref| <= G (K + 8) u mag (+ u |base| with accumulate)
        column sums    |cs - ref|  <= G (K + M) u sum_m mag_epi
        dropped elements of BIAS_DROP_RES equal R bit for bit; the dropped set is tk._keep_mask's
        BIAS_GELU: C within 1e-2 of the largest |ref|, U within 2.6e-3 + 1e-3 (tests/test_kernels_gpu.py: the kernel's erf is an
        approximation); its e4m3 copy within fp8_producer_ref.fp32_rounded_bound of clamp(C s_c)
    G = 1 would be the bf16 file's bound.  The block-scaled MFMA's sum of 64 products is no plain fp32 chain: one instruction alone
    (K = 40, K = 64) leaves up to 7.6 (K + 8) u mag, and the excess falls off as the fp32 chain over the k-stages takes over (1.3 at
    K = 128, 0.5 at K = 192, below 0.15 from K = 424).  So G is measured, not derived, by the rule the file was written under: the
    worst err / ((K + 8) u mag) over all weight-gradient cases (fp32 outputs: no output rounding hides the term) is 7.602, G is the
    next power of two at or above twice that.  profiles/fp8_gemm_parity.txt holds the ratio of every case;
  * e4m3 copies (DGELU, BIAS_GELU): |deq(C8) - clamp(C s_c, +-448)| <= fp32_rounded_bound, s_c from c8_amax_prev (56 / 224) or 1; the
    recorded amax, rounded to bf16, equals max |C| of the stored bf16 output; C = NULL changes no other output;
  * epilogue and tail cases run on windows of wider buffers (lda = K + 64, ldb = K + 64, ldc = N + 64, ldr = N + 128, ldu = N + 64,
    ldc8 = N + 64) whose padding holds the e4m3 NaN code 0x7F / bf16 NaN (inputs) or a sentinel (outputs, 256 spare rows above and
    below): no NaN may leak, no byte outside a window change;
  * wherever the plan takes the packed B operand, the packed run equals the plain one byte for byte in every output.
"""
import ctypes
import gc as _gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import nbest_amd  # noqa: E402,F401
from nbest_amd import hipabi as hb  # noqa: E402

import fp8_producer_ref as ref8  # noqa: E402
import gemm8_cases as g8  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402  (_keep_mask, _log, gelu / dgelu)
from test_gemm_variants_gpu import Window, _embed, assert_within  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
U23 = 2.0 ** -23
G = 16.0                                                             # the factor g of the accumulation term (module docstring)
DROP = dict(drop_p=0.1, seed=11, drop_stream=5)
W = hb.AMAX_TENSOR_WORDS
POS = ref8.slot_positions(W)
ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE = -1, -2, -4, -6        # include/nbest_hip.h


def _randn(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV) * scale


def _to_e4m3_bytes(x):
    """torch's conversion (round to nearest even, saturating), on the CPU; bytes on the device"""
    return ref8.e4m3_bytes(x.cpu()).to(DEV)


def _deq64(b):
    return ref8.dequant(b).double()


def _bits(v):
    return ref8.float_bits(v).to(DEV)


def _embed8(b, pad):
    """e4m3 bytes as a column window of a buffer `pad` bytes wider whose other bytes are the NaN code 0x7F"""
    return _embed(b.view(F8), pad).view(torch.uint8)


def _amax_off_edge(a, target):
    """an amax near `a` whose scale does not depend on how a log2 rounds at a power of two"""
    while ref8.binade_margin(a, target) < 0.1:
        a *= 1.09
    return a


# ---- operands and the fp64 products of one shape: built once, shared by the epilogues and modes of the case ---------------------------
_problem = {}


def problem(M, N, K):
    key = (M, N, K)
    if _problem.get("key") != key:
        _problem.clear()
        _gc.collect()
        torch.cuda.empty_cache()
        A8 = _to_e4m3_bytes(_randn((M, K), 1000 + M + K))
        Wf = _randn((N, K), 2000 + N + K, 0.03)
        s = ref8.pow2_scale(float(Wf.abs().max()), 224.0)
        W8 = _to_e4m3_bytes(Wf * s)
        A64, W64 = _deq64(A8), _deq64(W8)
        acc = (A64 @ W64.t()) / s                                  # (s is a power of two: exact)
        mag = (A64.abs() @ W64.abs().t()) / s
        del A64, W64
        Wp, pbn = hb.pack_weight_fp8(W8)
        _problem.update(key=key, A8=A8, W8=W8, A8s=_embed8(A8, 64), W8s=_embed8(W8, 64), out_scale=1.0 / s, acc=acc, mag=mag,
                        bias=_randn((N,), 3000 + N), R=_randn((M, N), 4000 + M + N).to(BF),
                        Uin=hb.gelu_d_encode(tk.dgelu(_randn((M, N), 5000 + M + N))), packed=Wp, packed_bn=pbn)
    return _problem


def reference(P, c, epi, scale_div=1.0, drop=None):
    """(ref, mag_epi, keep) in fp64: acc and mag carried through the epilogue"""
    acc, mag = P["acc"] / scale_div, P["mag"] / scale_div
    b64 = P["bias"].double()
    keep = None
    if epi == g8.NONE:
        return acc, mag, None
    if epi in (g8.BIAS, g8.BIAS_GELU):
        return acc + b64, mag + b64.abs(), None
    if epi == g8.RES:
        return acc + P["R"].double(), mag + P["R"].double().abs(), None
    if epi == g8.DGELU:
        ud = ((P["Uin"].float() - 26.0) * 0.005).double()          # the kernel's decode, exact in fp32
        return acc * ud, mag * ud.abs(), None
    R64 = P["R"].double()
    if drop is None:
        return acc + b64 + R64, mag + b64.abs() + R64.abs(), None
    keep, scale = tk._keep_mask(c.M, c.N, drop["drop_p"], drop["seed"], drop["drop_stream"])
    zero = torch.zeros_like(acc)
    return torch.where(keep, (acc + b64) * scale, zero) + R64, torch.where(keep, (mag + b64.abs()) * scale, zero) + R64.abs(), keep


class Run:
    """one launch of nbest_gemm_fp8 on guarded windows; .C / .U / .C8 are the window views (None: not an output), .cs the column sums,
    .slots the amax slot block"""

    def __init__(self, P, c, epi, strided, b_strided, packed, want_c=True, drop=None, a_amax=None, c8_prev=None, slots=None,
                 out_scale=None, out_scale_dev=None, colsum=True, Rin=None):
        M, N, K = c.M, c.N, c.K
        ldpad = 64 if strided else 0
        self.tag = g8.case_id(c, epi) + (" strided" if strided else "") + (" packed" if packed else "") + ("" if want_c else " C=NULL")
        self.Cw = Window(M, N, BF, ldpad) if want_c else None
        self.Uw = Window(M, N, torch.uint8, ldpad) if epi == g8.BIAS_GELU else None
        self.C8w = Window(M, N, torch.uint8, ldpad) if epi in (g8.BIAS_GELU, g8.DGELU) else None
        self.cs = torch.zeros(N, device=DEV) if (epi == g8.DGELU and colsum) else None
        self.slots = None
        kw = dict(epilogue=epi, out_scale=P["out_scale"] if out_scale is None else out_scale, want_c=want_c, a_amax=a_amax,
                  out_scale_dev=out_scale_dev)
        if want_c:
            kw["out"] = self.Cw.view
        if epi in g8.FORWARD_EPIS:
            kw["bias"] = P["bias"]
        if epi in (g8.BIAS_DROP_RES, g8.RES):
            R = P["R"] if Rin is None else Rin
            kw["R"] = _embed(R, 128 if strided else 0, 64 if strided else 0)
        if epi == g8.BIAS_DROP_RES and drop is not None:
            kw.update(drop)
        if epi == g8.BIAS_GELU:
            kw.update(U=self.Uw.view, C8=self.C8w.view)
        if epi == g8.DGELU:
            U = P["Uin"]
            if strided:                                            # (a byte has no NaN: the padding holds 0xFF = a GELU' of 1.145)
                wide = torch.full((M, N + ldpad), 0xFF, dtype=torch.uint8, device=DEV)
                wide[:, 32:32 + N] = U
                U = wide[:, 32:32 + N]
            kw.update(U=U, C8=self.C8w.view, colsum_out=self.cs)
        if epi in (g8.BIAS_GELU, g8.DGELU):
            self.slots = torch.zeros(W, dtype=torch.int32, device=DEV) if slots is None else slots
            kw.update(c8_amax_prev=c8_prev, c8_amax_slots=self.slots)
        if packed:
            kw.update(B_packed=P["packed"], b_pack_bn=P["packed_bn"])
        A, B = (P["A8s"] if strided else P["A8"]), (P["W8s"] if b_strided else P["W8"])
        self.plan = hb.gemm_fp8_plan(A, B, M, N, K, **kw)
        assert g8.tile_of(self.plan) == c.tile, "%s runs bn = %d on %d stages" % (self.tag, self.plan["bn"], self.plan["stages"])
        assert self.plan["packed_taken"] == int(packed), "%s: packed_taken = %d" % (self.tag, self.plan["packed_taken"])
        if c.tiles_m is not None:
            assert self.plan["tiles_m"] == c.tiles_m
        if c.group_cols is not None:
            assert self.plan["group_cols"] == c.group_cols and self.plan["tiles_n"] == 2 * c.group_cols
        hb.gemm_fp8(A, B, M, N, K, **kw)
        torch.cuda.synchronize()
        for w, name in ((self.Cw, "C"), (self.Uw, "U"), (self.C8w, "C8")):
            if w is not None:
                w.assert_outside_untouched(self.tag + " " + name)
        self.C = self.Cw.view if want_c else None
        self.U = self.Uw.view if self.Uw is not None else None
        self.C8 = self.C8w.view if self.C8w is not None else None

    def outputs(self):
        out = {"C8": self.C8, "U": self.U, "column sums": self.cs, "amax words": self.slots}
        return {k: v for k, v in out.items() if v is not None}


def _same_bytes(tag, a, b):
    for name, x in a.outputs().items():
        y = b.outputs()[name]
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), "%s: %s differs" % (tag, name)
    if a.C is not None and b.C is not None:
        assert torch.equal(a.C.view(torch.int16), b.C.view(torch.int16)), "%s: C differs" % tag


def recorded_amax(tag, slots):
    """max over the slot words of a block that started as zeros; no other word written"""
    host = slots.cpu()
    mask = torch.ones(W, dtype=torch.bool)
    mask[POS] = False
    assert not bool(host[mask].any()), tag + ": a word that is no slot position was written"
    return float(host[POS].view(torch.float32).max())


def check_copy(run, epi, hist, ref, accbound):
    """the e4m3 copy and the amax record of a run that has C"""
    tag, C, C8 = run.tag, run.C, run.C8
    s_c = ref8.pow2_scale(hist, ref8.GRAD_TARGET if epi == g8.DGELU else ref8.ACT_TARGET)
    assert not bool(ref8.is_nan_code(C8).any()), "%s: e4m3 NaN codes in C8" % tag
    v = (C.float() * s_c).clamp(-ref8.E4M3_MAX, ref8.E4M3_MAX)
    err, bound = (ref8.dequant(C8.contiguous()) - v).abs(), ref8.fp32_rounded_bound(v)
    tk._log("gemm8 %-72s C8 s_c=%g worst err/bound=%.3f" % (tag, s_c, float((err / bound).max())))
    assert bool((err <= bound).all()), "%s: %d bytes of C8 outside the bound (s_c = %g)" % (tag, int((err > bound).sum()), s_c)
    rec = recorded_amax(tag, run.slots)
    stored = float(C.float().abs().max())
    assert float(torch.tensor(rec).to(BF).float()) == stored, "%s: recorded amax %r, max |C| stored %r" % (tag, rec, stored)
    want = float(ref.abs().max())
    slack = float(accbound.max()) if epi == g8.DGELU else 1e-2 * want
    assert abs(rec - want) <= slack, "%s: recorded amax %r, fp64 max |ref| %r" % (tag, rec, want)


def check_run(run, P, c, epi, ref, m, keep, K_sum, hist=None):
    """every output of a run with C against the reference"""
    tag, got = run.tag, run.C
    M = c.M
    assert not bool(torch.isnan(got).any()), "%s: NaN in the output" % tag
    accbound = G * (K_sum + 8) * U23 * m
    if epi == g8.BIAS_GELU:
        r = tk.gelu(ref)
        scale = max(float(r.abs().max()), 1e-6)
        cerr = float((got.double() - r).abs().max()) / scale
        gerr = float((((run.U.float() - 26.0) * 0.005).double() - tk.dgelu(ref)).abs().max())
        tk._log("gemm8 %-72s C rel_err=%.3e (1e-2)  U abs_err=%.3e (3.6e-3)" % (tag, cerr, gerr))
        assert cerr <= 1e-2, "%s: C rel err %.3e" % (tag, cerr)
        assert gerr <= 2.6e-3 + 1e-3, "%s: U abs err %.3e" % (tag, gerr)
        check_copy(run, epi, hist, r, accbound)
        return
    if keep is not None:
        R = P["R"]
        assert torch.equal(got[~keep].view(torch.int16), R[~keep].view(torch.int16)), "%s: a dropped element differs from R" % tag
    assert_within("fp8 " + tag, got, ref, 2.0 ** -8 * ref.abs() + accbound, 256, c.tile[0])
    if run.cs is not None:
        assert_within("fp8 " + tag + " column sums", run.cs, ref.sum(0), G * (K_sum + M) * U23 * m.sum(0), 1 << 30, c.tile[0])
    if epi == g8.DGELU:
        check_copy(run, epi, hist, ref, accbound)


def run_case(c, epi, strided):
    """strided: everything on windows of wider buffers, with a history for the e4m3 copy; then B with packed rows, plain and packed
    (no history), byte for byte.  Not strided: plain and packed."""
    P = problem(c.M, c.N, c.K)
    drop = DROP if (c.drop and epi == g8.BIAS_DROP_RES) else None
    ref, m, keep = reference(P, c, epi, drop=drop)
    assert P["packed"] is not None and P["packed_bn"] == c.tile[0], "the packed image is built for %d-column tiles" % P["packed_bn"]
    if strided:
        hist = None
        if epi in (g8.BIAS_GELU, g8.DGELU):
            top = float((tk.gelu(ref) if epi == g8.BIAS_GELU else ref).abs().max())
            target = ref8.GRAD_TARGET if epi == g8.DGELU else ref8.ACT_TARGET
            hist = _amax_off_edge(0.05 * top, target)              # (a history far below the amax: the top values saturate at +-448)
        run = Run(P, c, epi, True, True, False, drop=drop, c8_prev=None if hist is None else _bits(hist))
        check_run(run, P, c, epi, ref, m, keep, c.K, hist)
        del run
    plain = Run(P, c, epi, strided, False, False, drop=drop)
    check_run(plain, P, c, epi, ref, m, keep, c.K)
    packed = Run(P, c, epi, strided, False, True, drop=drop)
    _same_bytes(plain.tag + " packed B against plain B", plain, packed)


def _params(cases):
    return [pytest.param(c, e, id=g8.case_id(c, e)) for c in cases for e in c.epis]


@pytest.mark.parametrize("c,epi", _params(g8.EPILOGUE_CASES))
def test_fp8_epilogues_strided_and_guarded(c, epi):
    run_case(c, epi, strided=True)


@pytest.mark.parametrize("c,epi", _params(g8.SHORT_K_CASES))
def test_fp8_short_and_wrapping_k(c, epi):
    """fewer k-stages than the ring is deep (the prologue's `nk` guards and the counted waits of the drain), as many, one more, and more
    than two turns"""
    run_case(c, epi, strided=False)


@pytest.mark.parametrize("c,epi", _params(g8.ROW_TAIL_CASES))
def test_fp8_row_tails(c, epi):
    """M mod 256 in {1, 255, 0}: the rows of the last tile past M are neither read into the result (column sums, amax) nor written"""
    run_case(c, epi, strided=True)


# ---- the e4m3 copy without C, slots that already hold more --------------------------------------------------------------------------------
SMALL = {g8.T128: g8.EPILOGUE_CASES[1], g8.T256: g8.EPILOGUE_CASES[3]}
assert SMALL[g8.T128].tile == g8.T128 and SMALL[g8.T256].tile == g8.T256


@pytest.mark.parametrize("tile", g8.ALL_TILES, ids=["T128", "T256"])
@pytest.mark.parametrize("epi", [g8.BIAS_GELU, g8.DGELU], ids=["bias_gelu", "dgelu"])
def test_fp8_copy_without_c_and_full_slots(tile, epi):
    c = SMALL[tile]
    P = problem(c.M, c.N, c.K)
    hist = _bits(_amax_off_edge(2.0, 56.0))
    with_c = Run(P, c, epi, True, True, False, c8_prev=hist)
    without = Run(P, c, epi, True, True, False, c8_prev=hist, want_c=False)
    _same_bytes(with_c.tag + " against C = NULL", with_c, without)
    # slots that hold a larger value are not lowered, and no other word is written
    big = torch.zeros(W, dtype=torch.int32, device=DEV)
    big[POS] = _bits(1e30)
    before = big.clone()
    Run(P, c, epi, True, True, False, c8_prev=hist, slots=big)
    assert torch.equal(big, before), "a slot holding 1e30 was changed"


# ---- the delayed scales ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", g8.ALL_TILES, ids=["T128", "T256"])
@pytest.mark.parametrize("epi", g8.ALL_EPIS, ids=[g8.EPI_NAMES[e] for e in g8.ALL_EPIS])
def test_fp8_a_amax_scale_target(tile, epi):
    """a_amax: the accumulator is divided by pow2_scale(amax, 224) under a forward epilogue, by pow2_scale(amax, 56) under a dgrad one
    (amax 3: 64 against 16 - a wrong target is a factor of 4)"""
    c = SMALL[tile]
    P = problem(c.M, c.N, c.K)
    target = ref8.ACT_TARGET if epi in g8.FORWARD_EPIS else ref8.GRAD_TARGET
    s = ref8.pow2_scale(3.0, target)
    assert s == (64.0 if epi in g8.FORWARD_EPIS else 16.0) and ref8.binade_margin(3.0, target) >= 0.1
    ref, m, _ = reference(P, c, epi, scale_div=s)
    run = Run(P, c, epi, False, False, False, a_amax=_bits(3.0))
    run.tag += " a_amax=3"
    check_run(run, P, c, epi, ref, m, None, c.K)


@pytest.mark.parametrize("tile", g8.ALL_TILES, ids=["T128", "T256"])
@pytest.mark.parametrize("epi", [g8.BIAS, g8.RES], ids=["bias", "res"])
def test_fp8_degenerate_amax_and_device_scale(tile, epi):
    c = SMALL[tile]
    P = problem(c.M, c.N, c.K)
    ref, m, _ = reference(P, c, epi)
    for bad in (0.0, float("inf"), float("nan"), 1e-40):
        run = Run(P, c, epi, False, False, False, a_amax=_bits(bad))
        run.tag += " a_amax=%r" % bad
        check_run(run, P, c, epi, ref, m, None, c.K)
    # out_scale_dev overrides a deliberately wrong host out_scale; together with a_amax
    dev = torch.tensor([P["out_scale"]], dtype=torch.float32, device=DEV)
    run = Run(P, c, epi, False, False, False, out_scale=P["out_scale"] * 7.0, out_scale_dev=dev)
    run.tag += " out_scale_dev"
    check_run(run, P, c, epi, ref, m, None, c.K)
    s = ref8.pow2_scale(0.37, ref8.ACT_TARGET if epi in g8.FORWARD_EPIS else ref8.GRAD_TARGET)
    ref, m, _ = reference(P, c, epi, scale_div=s)
    run = Run(P, c, epi, False, False, False, out_scale=123.0, out_scale_dev=dev, a_amax=_bits(0.37))
    run.tag += " out_scale_dev a_amax=0.37"
    check_run(run, P, c, epi, ref, m, None, c.K)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("c", [g8.EPILOGUE_CASES[0], g8.EPILOGUE_CASES[3]], ids=["T128", "T256"])
def test_fp8_dropout_counter(c, p):
    """BIAS_DROP_RES with dropout on a strided C: the dropped set is tk._keep_mask's (counter m N + n whatever ldc is) and that of the
    bf16 GEMM and of the LayerNorm backward at the same (seed, stream) and shape; dropped elements are R bit for bit; survivors are
    (acc scale + bias) 65536 / (65536 - thr16) + R within the bf16 bound"""
    P = problem(c.M, c.N, c.K)
    M, N, K = c.M, c.N, c.K
    drop = dict(drop_p=p, seed=7, drop_stream=3)
    ref, m, keep = reference(P, c, g8.BIAS_DROP_RES, drop=drop)
    run = Run(P, c, g8.BIAS_DROP_RES, True, True, False, drop=drop)
    run.tag += " p=%g" % p
    check_run(run, P, c, g8.BIAS_DROP_RES, ref, m, keep, K)
    # the dropped set itself: with R = 0 a dropped element is +0 and a survivor is not (acc scale + bias == 0 does not occur: asserted)
    zeros = torch.zeros(M, N, dtype=BF, device=DEV)
    base = Run(P, c, g8.BIAS_DROP_RES, True, True, False, Rin=zeros)
    assert not bool((base.C == 0).any())
    z = Run(P, c, g8.BIAS_DROP_RES, True, True, False, drop=drop, Rin=zeros)
    dropped = z.C.view(torch.int16) == 0
    assert torch.equal(dropped, ~keep), "%s: %d elements dropped, the counter stream drops %d; first difference at %s" % (
        run.tag, int(dropped.sum()), int((~keep).sum()), (dropped != ~keep).nonzero()[0].tolist())
    frac = float(dropped.float().mean())
    assert abs(frac - round(p * 65536) / 65536) < 0.01, frac
    # the bf16 GEMM on the same shape ...
    A, B = ref8.dequant(P["A8"]).to(BF), ref8.dequant(P["W8"]).to(BF)     # (exact: e4m3 has 3 mantissa bits)
    y0 = hb.gemm(A, B, M, N, K, epilogue=hb.EPI_BIAS_DROP_RES, bias=P["bias"], R=zeros)
    y = hb.gemm(A, B, M, N, K, epilogue=hb.EPI_BIAS_DROP_RES, bias=P["bias"], R=zeros, **drop)
    assert not bool((y0 == 0).any())
    assert torch.equal(y.view(torch.int16) == 0, dropped), "the bf16 GEMM drops another set"
    # ... and the LayerNorm backward, which regenerates the mask for the dense-branch gradient
    x, dy = _randn((M, N), 23).to(BF), _randn((M, N), 24).to(BF)
    gam = torch.ones(N, device=DEV)
    _, stats = hb.layernorm_fwd(x, gam, torch.zeros(N, device=DEV), 1e-12)
    dx, dxd, *_ = hb.layernorm_bwd(dy, x, stats, gam, **drop)
    live = dx.float() != 0
    assert torch.equal((dxd.float() == 0) & live, dropped & live), "the LayerNorm backward drops another set"


# ---- weight gradients -------------------------------------------------------------------------------------------------------------------------
_wproblem = {}


def wproblem(M, N, K):
    key = (M, N, K)
    if _wproblem.get("key") != key:
        _wproblem.clear()
        dY8, X8 = _to_e4m3_bytes(_randn((K, M), 7000 + M + K)), _to_e4m3_bytes(_randn((K, N), 8000 + N + K))
        d64, x64 = _deq64(dY8), _deq64(X8)
        _wproblem.update(key=key, dY8=_embed8(dY8, 64), X8=_embed8(X8, 64), acc=d64.t() @ x64, mag=d64.abs().t() @ x64.abs(),
                         base=_randn((M, N), 6000 + M + N))
    return _wproblem


def run_wgrad(c, a_amax=None, x_amax=None):
    """operands with leading dimensions M + 64 / N + 64 (padding: the NaN code), dW a window of a sentinel-filled buffer (ldc = N + 64)"""
    M, N, K = c.M, c.N, c.K
    P = wproblem(M, N, K)
    splits, kps = hb.wgrad_fp8_plan(M, N, K)
    assert splits == c.splits and g8.last_split(K, splits, kps) == c.last, "%s runs %d splits of %d" % (g8.wcase_id(c), splits, kps)
    s = ref8.pow2_scale(a_amax, ref8.GRAD_TARGET) * ref8.pow2_scale(x_amax, ref8.ACT_TARGET)
    tag = "wgrad " + g8.wcase_id(c) + ("" if a_amax is None else " a_amax=%g" % a_amax) + ("" if x_amax is None else " x_amax=%g" % x_amax)
    win = Window(M, N, torch.float32, 64)
    ref, bound = P["acc"] / s, G * (K + 8) * U23 * P["mag"] / s
    if c.acc:
        win.view.copy_(P["base"])
        ref, bound = ref + P["base"].double(), bound + U23 * P["base"].double().abs()
    hb.wgrad_fp8(P["dY8"], P["X8"], M, N, K, a_amax=None if a_amax is None else _bits(a_amax), out=win.view, accumulate=c.acc,
                 x_amax=None if x_amax is None else _bits(x_amax))
    torch.cuda.synchronize()
    win.assert_outside_untouched(tag)
    assert not bool(torch.isnan(win.view).any()), tag + ": NaN in the output"
    raw = float(((win.view.double() - ref).abs() / ((K + 8) * U23 * P["mag"] / s)).max())      # what G is measured from (G itself left out)
    tk._log("gemm8 %-72s worst err / ((K + 8) u mag) = %.3f" % (tag, raw))
    return assert_within("fp8 " + tag, win.view, ref, bound, 256, 256)


@pytest.mark.parametrize("c", g8.WGRAD_CASES, ids=[g8.wcase_id(c) for c in g8.WGRAD_CASES])
def test_fp8_wgrad_direct_and_split(c):
    """gemm8tt_kernel: 1 .. 9 k-stages written directly (the tail logic of its generic loop against the 4-stage ring, ragged token
    counts zero-filled by the buffer range check), and K-splits whose last split is short / ragged.  The logged worst err/bound of
    these cases is the measured accumulation term: G stands on it."""
    run_wgrad(c)


@pytest.mark.parametrize("c", [g8.WGRAD_DIRECT_CASES[13], g8.WGRAD_SPLIT_CASES[3]], ids=["direct", "split"])
def test_fp8_wgrad_scales(c):
    """a_amax alone (gradient scale, target 56), x_amax alone (activation scale, target 224), both; degenerate amaxes give scale 1"""
    assert ref8.pow2_scale(3.0, 56.0) == 16.0 and ref8.pow2_scale(0.4, 224.0) == 512.0
    run_wgrad(c, a_amax=3.0)
    run_wgrad(c, x_amax=0.4)
    run_wgrad(c, a_amax=3.0, x_amax=0.4)
    for bad in (0.0, float("inf"), float("nan"), 1e-40):
        run_wgrad(c, a_amax=bad, x_amax=bad)


def test_fp8_wgrad_pair_scales_and_accumulate():
    """nbest_wgrad_fp8_pair at H = 256: Q|K|V ([3H][H], dQ|dK|dV rows with leading dimension 3H) and attention output ([H][H]) in one
    split launch, each problem with its own gradient and activation scale, accumulated into existing gradients"""
    H, K = g8.PAIR_H, g8.PAIR_K
    splits, kps = hb.wgrad_fp8_plan(4 * H, H, K)
    assert splits == g8.PAIR_SPLITS and g8.last_split(K, splits, kps) == g8.PAIR_LAST
    ops = [_to_e4m3_bytes(_randn((K, n), 9000 + i)) for i, n in enumerate((3 * H, H, H, H))]
    dqkv, x, dy, ctx = ops
    assert dqkv.stride(0) == 3 * H
    amax = {"a": (3.0, 0.4), "b": (0.37, 150.0)}                   # (gradient, activation) amax of each problem
    wins, refs, bounds = [], [], []
    for (d8, x8, key, rows, seed) in ((dqkv, x, "a", 3 * H, 1), (dy, ctx, "b", H, 2)):
        s = ref8.pow2_scale(amax[key][0], 56.0) * ref8.pow2_scale(amax[key][1], 224.0)
        d64, x64 = _deq64(d8), _deq64(x8)
        base = _randn((rows, H), 6100 + seed)
        win = Window(rows, H, torch.float32, 64)
        win.view.copy_(base)
        wins.append(win)
        refs.append(d64.t() @ x64 / s + base.double())
        bounds.append(G * (K + 8) * U23 * (d64.abs().t() @ x64.abs()) / s + U23 * base.double().abs())
    assert ref8.pow2_scale(3.0, 56.0) != ref8.pow2_scale(0.37, 56.0)
    hb.wgrad_fp8_pair(dqkv, x, dy, ctx, amax_a=_bits(amax["a"][0]), amax_b=_bits(amax["b"][0]), outs=(wins[0].view, wins[1].view),
                      accumulate=True, xamax_a=_bits(amax["a"][1]), xamax_b=_bits(amax["b"][1]))
    torch.cuda.synchronize()
    for win, r, b, name in zip(wins, refs, bounds, ("QKV", "attention output")):
        win.assert_outside_untouched("wgrad pair " + name)
        assert_within("fp8 wgrad pair H=%d K=%d %s" % (H, K, name), win.view, r, b, 256, 256)


# ---- refusals: the code each host check states, nothing written ---------------------------------------------------------------------------------
def test_fp8_refusals_leave_the_outputs_untouched():
    """every buffer is real and as large as the (unmodified) block declares: no case relies on a check to stop an undersized launch (the
    4 GiB and dropout-counter checks are exercised by tests/test_gemm8_cases_cpu.py on the plan alone)"""
    M, N, K = 512, 256, 128
    A8, W8 = _to_e4m3_bytes(_randn((M + 8, K + 64), 1)), _to_e4m3_bytes(_randn((N + 8, K + 64), 2))
    bias, R = _randn((N,), 3), _randn((M + 8, N + 64), 4).to(BF)
    U = torch.full((M + 8, N + 64), 100, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(8 * N * 4 + 64, dtype=torch.uint8, device=DEV)
    slots = torch.zeros(W, dtype=torch.int32, device=DEV)
    Cw, C8w, Uw = Window(M + 8, N + 64, BF, 0), Window(M + 8, N + 64, torch.uint8, 0), Window(M + 8, N + 64, torch.uint8, 0)
    cs = torch.full((N,), 7.0, device=DEV)
    L = hb.lib()

    def block(**over):
        g = hb.GemmFp8Args()
        g.A, g.B, g.C, g.bias = A8.data_ptr(), W8.data_ptr(), Cw.view.data_ptr(), bias.data_ptr()
        g.M, g.N, g.K, g.lda, g.ldb, g.ldc = M, N, K, K + 64, K + 64, N + 64
        g.ldr = g.ldu = g.ldc8 = N + 64
        g.epilogue, g.out_scale = hb.EPI_BIAS, 1.0
        for k, v in over.items():
            setattr(g, k, v)
        return g

    dgelu = dict(epilogue=hb.EPI_DGELU, U=U.data_ptr(), bias=None)
    cases = [
        ("null A", dict(A=None), ERR_ARG),
        ("null C", dict(C=None), ERR_ARG),
        ("N not a multiple of 256", dict(N=128), ERR_SHAPE),
        ("K not a multiple of 64", dict(K=96), ERR_SHAPE),
        ("M = 0", dict(M=0), ERR_SHAPE),
        ("lda not a multiple of 16", dict(lda=K + 8), ERR_ALIGN),
        ("ldb not a multiple of 16", dict(ldb=K + 8), ERR_ALIGN),
        ("ldc not a multiple of 8", dict(ldc=N + 4), ERR_ALIGN),
        ("unaligned A", dict(A=A8.data_ptr() + 8), ERR_ALIGN),
        ("unaligned B", dict(B=W8.data_ptr() + 8), ERR_ALIGN),
        ("unaligned C", dict(C=Cw.view.data_ptr() + 8), ERR_ALIGN),
        ("epilogue not built", dict(epilogue=hb.EPI_F32_SPLITK), ERR_ARG),
        ("bias missing", dict(bias=None), ERR_ARG),
        ("BIAS_GELU without U", dict(epilogue=hb.EPI_BIAS_GELU, C8=C8w.view.data_ptr()), ERR_ARG),
        ("BIAS_GELU without C8", dict(epilogue=hb.EPI_BIAS_GELU, U=Uw.view.data_ptr()), ERR_ARG),
        ("BIAS_GELU with ldu not a multiple of 8", dict(epilogue=hb.EPI_BIAS_GELU, U=Uw.view.data_ptr(), C8=C8w.view.data_ptr(), ldu=N + 4), ERR_ARG),
        ("RES without R", dict(epilogue=hb.EPI_RES, bias=None), ERR_ARG),
        ("BIAS_DROP_RES with unaligned R", dict(epilogue=hb.EPI_BIAS_DROP_RES, R=R.data_ptr() + 8), ERR_ARG),
        ("DGELU without U", dict(dgelu, U=None), ERR_ARG),
        ("DGELU with unaligned C8", dict(dgelu, C8=C8w.view.data_ptr() + 4, c8_amax_new=slots.data_ptr()), ERR_ARG),
        ("DGELU with C8 but no c8_amax_new", dict(dgelu, C8=C8w.view.data_ptr()), ERR_ARG),
        ("DGELU with C8 alone (C = NULL) but no c8_amax_new", dict(dgelu, C=None, C8=C8w.view.data_ptr()), ERR_ARG),
        ("DGELU column sums with a short workspace", dict(dgelu, colsum_out=cs.data_ptr(), ws=ws.data_ptr(), ws_bytes=2 * 2 * N * 4 - 4),
         ERR_WORKSPACE),
        ("DGELU column sums without a workspace", dict(dgelu, colsum_out=cs.data_ptr()), ERR_WORKSPACE),
    ]
    for name, over, code in cases:
        g, info = block(**over), hb.GemmFp8PlanInfo()
        assert L.nbest_gemm_fp8(ctypes.byref(g), hb.stream_ptr()) == code, "%s: %s" % (name, hb.last_error())
        msg = hb.last_error()
        assert L.nbest_gemm_fp8_plan(ctypes.byref(g), ctypes.byref(info)) == code and hb.last_error() == msg, name
    torch.cuda.synchronize()
    for w, name in ((Cw, "C"), (C8w, "C8"), (Uw, "U")):
        assert bool((w.buf.view(w.itype) == w.sent).all()), "a refused call wrote " + name
    assert bool((cs == 7.0).all()) and not bool(slots.any()) and not bool(ws.any())

    # the weight gradients
    Mw, Nw, Kw = 256, 256, 4160                                      # splits: needs a workspace
    splits, _ = hb.wgrad_fp8_plan(Mw, Nw, Kw)
    assert splits > 1
    dY8, X8 = _to_e4m3_bytes(_randn((Kw + 1, Mw + 64), 5)), _to_e4m3_bytes(_randn((Kw + 1, Nw + 64), 6))
    dW = Window(Mw + 8, Nw + 64, torch.float32, 0)
    wsw = torch.zeros(splits * Mw * Nw * 4, dtype=torch.uint8, device=DEV)
    dp, xp, wp, wsp, st = dY8.data_ptr(), X8.data_ptr(), dW.view.data_ptr(), wsw.data_ptr(), hb.stream_ptr()
    ld, full = Mw + 64, wsw.numel()
    wcases = [
        ("null dY8", (None, xp, wp, Mw, Nw, Kw, ld, ld, ld, None, None, 0, wsp, full, st), ERR_ARG),
        ("K = 0", (dp, xp, wp, Mw, Nw, 0, ld, ld, ld, None, None, 0, wsp, full, st), ERR_ARG),
        ("M not a multiple of 256", (dp, xp, wp, Mw - 128, Nw, Kw, ld, ld, ld, None, None, 0, wsp, full, st), ERR_SHAPE),
        ("N not a multiple of 256", (dp, xp, wp, Mw, Nw - 128, Kw, ld, ld, ld, None, None, 0, wsp, full, st), ERR_SHAPE),
        ("lda not a multiple of 16", (dp, xp, wp, Mw, Nw, Kw, ld - 8, ld, ld, None, None, 0, wsp, full, st), ERR_ALIGN),
        ("ldc not a multiple of 8", (dp, xp, wp, Mw, Nw, Kw, ld, ld, ld - 4, None, None, 0, wsp, full, st), ERR_ALIGN),
        ("unaligned X8", (dp, xp + 8, wp, Mw, Nw, Kw, ld, ld, ld, None, None, 0, wsp, full, st), ERR_ALIGN),
        ("declared workspace too small", (dp, xp, wp, Mw, Nw, Kw, ld, ld, ld, None, None, 0, wsp, full - 4, st), ERR_WORKSPACE),
        ("no workspace", (dp, xp, wp, Mw, Nw, Kw, ld, ld, ld, None, None, 0, None, 0, st), ERR_WORKSPACE),
    ]
    for name, args, code in wcases:
        assert L.nbest_wgrad_fp8(*args) == code, "%s: %s" % (name, hb.last_error())
    # the pair: both problems [K][256 + 64] -> 256 x 256 each (512 virtual rows: splits)
    assert hb.wgrad_fp8_plan(2 * Mw, Nw, Kw)[0] > 1
    ws2 = torch.zeros(L.nbest_wgrad_fp8_pair_ws_bytes(Mw, Mw, Nw, Kw), dtype=torch.uint8, device=DEV)
    dW2 = Window(Mw + 8, Nw + 64, torch.float32, 0)
    w2p, ws2p, full2 = dW2.view.data_ptr(), ws2.data_ptr(), ws2.numel()

    def pair(a=dp, Ma=Mw, lda=ld, b=dp, Mb=Mw, ldcb=ld, N=Nw, K=Kw, wsb=full2):
        return L.nbest_wgrad_fp8_pair(a, xp, wp, Ma, lda, ld, ld, None, None, b, xp, w2p, Mb, ld, ld, ldcb, None, None, N, K, 0, ws2p, wsb, st)

    assert pair(a=None) == ERR_ARG, hb.last_error()
    assert pair(Mb=Mw - 128) == ERR_SHAPE, hb.last_error()
    assert pair(N=Nw - 128) == ERR_SHAPE, hb.last_error()
    assert pair(K=512) == ERR_SHAPE, hb.last_error()                  # one split: the pair does not fit
    assert pair(lda=ld - 8) == ERR_ALIGN, hb.last_error()
    assert pair(ldcb=ld - 4) == ERR_ALIGN, hb.last_error()
    assert pair(b=dp + 8) == ERR_ALIGN, hb.last_error()
    assert pair(wsb=full2 - 4) == ERR_WORKSPACE, hb.last_error()
    torch.cuda.synchronize()
    for w in (dW, dW2):
        assert bool((w.buf.view(w.itype) == w.sent).all()), "a refused weight gradient wrote its output"
    assert not bool(wsw.any()) and not bool(ws2.any())
