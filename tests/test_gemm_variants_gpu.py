"""Every bf16 GEMM kernel variant nbest_gemm can pick (tests/gemm_cases.py), each against an fp64 reference of the same operation
on the same bf16 inputs, element by element.

  * the case asserts through nbest_gemm_plan that it runs the variant it names before it launches;
  * per-element bound, derived (u = 2^-23, K the summed length, mag = |A| . |B| carried through the epilogue):
        bf16 outputs   |got - ref| <= 2^-8 |ref| + (K + 8) u mag      one bf16 rounding (truncation allowed for) + a length-K fp32 sum
                                                                      in any order + a few epilogue operations
        fp32 outputs   |got - ref| <= (K + 8) u mag (+ u |base| with accumulate)
        column sums    |cs - ref|  <= (K + M) u sum_m mag
        dropped elements of BIAS_DROP_RES equal R bit for bit
        BIAS_GELU: C within 1e-2 of the largest |ref|, U within 2.6e-3 + 4e-3 (tests/test_kernels_gpu.py: the kernel's erf is an
        approximation whose error the project does not state);
  * full-size cases run on windows of wider buffers (lda = K + 64, ldb + 64, ldr = N + 128, ldu = N + 64, ldc = N + 64) whose padding holds
    NaN (inputs) or a sentinel bit pattern (outputs, 256 spare rows above and below): no NaN may leak, no byte outside the window change;
  * where the plan takes the packed B operand, the packed run equals the unpacked one bit for bit.
"""
import gc as _gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import nbest_amd  # noqa: E402,F401
from nbest_amd import hipabi as hb  # noqa: E402

import gemm_cases as gc  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402  (_keep_mask: the independent restatement of the dropout decision; _log; gelu / dgelu)

DEV = "cuda"
BF = torch.bfloat16
U23 = 2.0 ** -23
DROP = dict(drop_p=0.1, seed=11, drop_stream=5)
SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A), torch.uint8: (torch.uint8, 0xA5)}


def _gen(shape, seed, scale, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def _embed(x, pad, col0=0):
    """x as a column window of a buffer `pad` columns wider whose other elements are NaN"""
    if pad == 0:
        return x
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, col0:col0 + x.shape[1]] = x
    return buf[:, col0:col0 + x.shape[1]]


class Window:
    """an [M][N] output window inside a buffer pre-filled with a sentinel bit pattern"""

    def __init__(self, M, N, dtype, ldpad, spare=256):
        self.M, self.N, self.spare, self.col0 = M, N, spare, (32 if ldpad else 0)
        self.itype, self.sent = SENTINEL[dtype]
        self.buf = torch.empty((M + 2 * spare, N + ldpad), dtype=dtype, device=DEV)
        self.buf.view(self.itype).fill_(self.sent)
        self.view = self.buf[spare:spare + M, self.col0:self.col0 + N]

    def assert_outside_untouched(self, tag):
        iv = self.buf.view(self.itype).clone()
        iv[self.spare:self.spare + self.M, self.col0:self.col0 + self.N] = self.sent
        bad = iv != self.sent
        if bool(bad.any()):
            r, c = [int(x) for x in bad.nonzero()[0]]
            raise AssertionError("%s: written outside the output window, first at buffer row %d (window rows %d .. %d), column %d (%d .. %d)"
                                 % (tag, r, self.spare, self.spare + self.M - 1, c, self.col0, self.col0 + self.N - 1))


# ---- operands and the fp64 products of one (shape, layout): built once, shared by the epilogues of the case ---------------------------
_problem = {}


def problem(c, strided):
    key = (c.M, c.N, c.K, c.ta, c.tb, strided)
    if _problem.get("key") != key:
        _problem.clear()
        _gc.collect()
        torch.cuda.empty_cache()
        M, N, K = c.M, c.N, c.K
        both_tokens = c.ta and c.tb                              # weight gradient: two activation-like operands
        A = _gen((K, M) if c.ta else (M, K), 1000 + M + K, 1.0 if both_tokens else 0.5)
        B = _gen((K, N) if c.tb else (N, K), 2000 + N + K, 1.0 if both_tokens else 0.05)
        A64 = A.double().t() if c.ta else A.double()
        B64 = B.double() if c.tb else B.double().t()
        acc = A64 @ B64
        mag = A64.abs() @ B64.abs()
        del A64, B64
        if strided == "cls":
            lda_pad = gc.CLS_ROW_STRIDE - K
        else:
            lda_pad = 64 if strided else 0
        _problem.update(key=key, A=_embed(A, lda_pad), B=_embed(B, 64 if strided else 0), B_plain=B, acc=acc, mag=mag,
                        bias=_gen((N,), 3000 + N, 1.0, torch.float32), R=_gen((M, N), 4000 + M + N, 1.0),
                        Uin=hb.gelu_d_encode(tk.dgelu(_gen((M, N), 5000 + M + N, 1.0, torch.float32))),
                        base=_gen((M, N), 6000 + M + N, 1.0, torch.float32), packed=None)
        if not c.ta and not c.tb:
            _problem["packed"] = hb.pack_weight(B.contiguous())
    return _problem


def assert_within(tag, got, ref, bound, bm, bn):
    """torch.all(|got - ref| <= bound); the failure names the worst element, its tile and its err / bound"""
    err = (got.double() - ref).abs()
    ok = err <= bound                                             # NaN compares false
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    worst = float(ratio.max())
    tk._log("gemm-variant %-72s worst err/bound=%.3f %s" % (tag, worst, "OK" if bool(ok.all()) else "FAIL"))
    if not bool(ok.all()):
        flat = int(ratio.argmax())
        ncol = ratio.shape[-1] if ratio.dim() > 1 else ratio.shape[0]
        m, n = (flat // ncol, flat % ncol) if ratio.dim() > 1 else (0, flat)
        raise AssertionError("%s: %d elements out of bound; worst at (m=%d, n=%d), tile (%d, %d): got %r ref %r err/bound %.3f"
                             % (tag, int((~ok).sum()), m, n, m // bm, n // bn, float(got.reshape(-1)[flat]), float(ref.reshape(-1)[flat]), worst))
    return worst


def run_case(c, epi, strided):
    """plan check, launch (twice where the packed operand is taken), reference, bounds, guards"""
    P = problem(c, strided)
    M, N, K = c.M, c.N, c.K
    bm, bn = c.variant[1], c.variant[2]
    tag = gc.case_id(c, epi) + (" strided" if strided else "")
    acc, mag, bias, b64 = P["acc"], P["mag"], P["bias"], P["bias"].double()
    kepi = gc.F32_SPLITK if epi == gc.F32_SPLITK_ACC else epi
    f32_out = kepi == gc.F32_SPLITK
    ldpad = 64 if strided else 0
    kw = dict(trans_a=bool(c.ta), trans_b=bool(c.tb), epilogue=kepi)
    R = U = Uwin = cs = base = None
    if epi in (gc.BIAS, gc.BIAS_GELU, gc.BIAS_DROP_RES):
        kw["bias"] = bias
    if epi in (gc.BIAS_DROP_RES, gc.RES):
        R = P["R"]
        if strided == "cls":
            kw["R"] = _embed(R, gc.CLS_ROW_STRIDE - N)
        else:
            kw["R"] = _embed(R, 128 if strided else 0, 64 if strided else 0)
    if epi == gc.BIAS_DROP_RES:
        kw.update(DROP)
    if epi == gc.DGELU:
        U = P["Uin"]
        cs = torch.zeros(N, device=DEV)
        kw.update(U=U, colsum_out=cs)
        if strided:                                               # (a byte has no NaN: the padding holds 0xFF = a GELU' of 1.145)
            wide = torch.full((M, N + ldpad), 0xFF, dtype=torch.uint8, device=DEV)
            wide[:, 32:32 + N] = U
            kw["U"] = wide[:, 32:32 + N]
    if epi == gc.F32_SPLITK_ACC:
        base = P["base"]
        kw["accumulate"] = True

    def launch(**more):
        win = Window(M, N, torch.float32 if f32_out else BF, ldpad)
        uw = Window(M, N, torch.uint8, ldpad) if epi == gc.BIAS_GELU else None
        if base is not None:
            win.view.copy_(base)
        args = dict(kw, out=win.view, **more)
        if uw is not None:
            args["U"] = uw.view
        plan = hb.gemm_plan(P["A"], P["B"], M, N, K, **args)
        assert gc.variant_of(plan) == c.variant, "%s runs %s" % (tag, gc.variant_name(gc.variant_of(plan)))
        if more and not plan["b_packed"]:
            return plan, None, None
        hb.gemm(P["A"], P["B"], M, N, K, **args)
        torch.cuda.synchronize()
        win.assert_outside_untouched(tag + " C")
        if uw is not None:
            uw.assert_outside_untouched(tag + " U")
        return plan, win, uw

    plan, win, uw = launch()
    got = win.view
    assert not bool(torch.isnan(got).any()), "%s: NaN in the output" % tag

    # ---- reference and bound --------------------------------------------------------------------------------------------------------------
    if epi == gc.BIAS_GELU:
        u = acc + b64
        ref = tk.gelu(u)
        scale = max(float(ref.abs().max()), 1e-6)
        cerr = float((got.double() - ref).abs().max()) / scale
        gerr = float((hb.gelu_d_decode(uw.view).double() - tk.dgelu(u)).abs().max())
        tk._log("gemm-variant %-72s C rel_err=%.3e (1e-2)  U abs_err=%.3e (6.6e-3)" % (tag, cerr, gerr))
        assert cerr <= 1e-2, "%s: C rel err %.3e" % (tag, cerr)
        assert gerr <= 2.6e-3 + 4e-3, "%s: U abs err %.3e" % (tag, gerr)
    else:
        if epi == gc.NONE or f32_out:
            ref, m = acc, mag
        elif epi == gc.BIAS:
            ref, m = acc + b64, mag + b64.abs()
        elif epi == gc.RES:
            ref, m = acc + R.double(), mag + R.double().abs()
        elif epi == gc.DGELU:
            ud = hb.gelu_d_decode(U).double()
            ref, m = acc * ud, mag * ud.abs()
        else:                                                     # BIAS_DROP_RES
            keep, scale = tk._keep_mask(M, N, DROP["drop_p"], DROP["seed"], DROP["drop_stream"])
            zero = torch.zeros_like(acc)
            ref = torch.where(keep, (acc + b64) * scale, zero) + R.double()
            m = torch.where(keep, (mag + b64.abs()) * scale, zero) + R.double().abs()
            assert torch.equal(got[~keep].view(torch.int16), R[~keep].view(torch.int16)), "%s: a dropped element differs from R" % tag
        if f32_out:
            bound = (K + 8) * U23 * m
            if base is not None:
                ref = ref + base.double()
                bound = bound + U23 * base.double().abs()
        else:
            bound = 2.0 ** -8 * ref.abs() + (K + 8) * U23 * m
        assert_within(tag, got, ref, bound, bm, bn)
        if cs is not None:
            assert_within(tag + " column sums", cs, ref.sum(0), (K + M) * U23 * m.sum(0), 1 << 30, bn)
        del ref, m, bound

    # ---- the packed B operand, wherever this tile takes it: bit-equal ---------------------------------------------------------------------
    assert plan["b_packed"] == 0
    if P["packed"] is not None and P["packed"][0] is not None and c.variant[0] == 2 and not f32_out:
        Bp, pbn = P["packed"]
        if cs is not None:
            kw["colsum_out"] = torch.zeros(N, device=DEV)
        plan2, win2, uw2 = launch(B_packed=Bp, b_pack_bn=pbn)
        if c.variant != gc.V2_RING_NN:                            # the 4-wave ring reads B row by row; every 8-wave tile takes the packed image
            assert plan2["b_packed"] == 1, "%s: the packed operand is not taken" % tag
        if plan2["b_packed"]:
            assert torch.equal(win2.view.view(torch.int16), got.view(torch.int16)), "%s: packed B differs from plain B" % tag
            if uw is not None:
                assert torch.equal(uw2.view, uw.view), "%s: packed B differs from plain B in U" % tag
            if cs is not None:
                assert torch.equal(kw["colsum_out"], cs), "%s: packed B differs from plain B in the column sums" % tag


def _params(cases):
    return [pytest.param(c, e, id=gc.case_id(c, e)) for c in cases for e in c.epis]


@pytest.mark.parametrize("c,epi", _params(gc.EPILOGUE_CASES))
def test_variant_epilogues_strided_and_guarded(c, epi):
    run_case(c, epi, strided=True)


@pytest.mark.parametrize("c,epi", _params([gc.CLS_STRIDE_CASE]))
def test_cls_row_stride(c, epi):
    """what nbest_encoder_infer issues on its last layer: A (and the residual) one row per utterance out of [B][S][H]"""
    run_case(c, epi, strided="cls")


@pytest.mark.parametrize("c,epi", _params(gc.SHORT_K_CASES))
def test_variant_short_and_wrapping_k(c, epi):
    """fewer k-stages than the ring is deep (the prologue's and the drain's `nk` guards), one more, and one more than two turns"""
    run_case(c, epi, strided=False)


@pytest.mark.parametrize("c,epi", _params(gc.ROW_TAIL_CASES))
def test_variant_row_tails(c, epi):
    """M mod bm in {1, bm - 1, 0}: the rows of the last tile past M are neither read into the result nor written"""
    run_case(c, epi, strided=False)


def test_fp32_accumulation_term_against_torch_matmul():
    """The accumulation term of the bound, measured on torch's own fp32 matmul with the same inputs and the same fp64 reference: the
    figure a widened constant would have to come from (none is widened: profiles/gemm_variant_parity.txt).  Logged, not asserted: it
    is a statement about another library."""
    c = gc.Case(gc.V2_256x256_S5, 16296, 3072, 2048, 0, 0, (gc.NONE,))
    P = problem(c, True)
    f32 = P["A"].float() @ P["B"].float().t()
    ratio = float(((f32.double() - P["acc"]).abs() / ((c.K + 8) * U23 * P["mag"])).max())
    tk._log("gemm-variant torch fp32 matmul vs fp64, M=%d N=%d K=%d: worst err / ((K + 8) u mag) = %.4f" % (c.M, c.N, c.K, ratio))
    assert ratio == ratio and ratio < float("inf")
