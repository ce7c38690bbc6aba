"""The reference helpers of tests/test_fp8_producers_gpu.py (tests/fp8_producer_ref.py) checked on the CPU, so that a failure on
the GPU points at a kernel: the scale restatement against oracle/bf16sim._fp8_scale, the e4m3 half-ulp bound, the identity
bf16(max |x|) == max |bf16(x)| the LayerNorm-backward amax check rests on, and the slot positions."""
import math

import torch

import nbest_amd  # noqa: F401
from nbest_amd import hipabi as hb
from oracle import bf16sim

import fp8_producer_ref as ref


def test_scale_restatement_matches_the_oracle():
    """2^floor(log2(T / amax)) for both targets over amax = m * 2^k: mantissas well inside a binade of T / amax (at an exact power of
    two the result hangs on how log2 rounds, which neither side promises), exponents across the range the clamp leaves alone"""
    n = 0
    for target in (ref.ACT_TARGET, ref.GRAD_TARGET):
        for k in range(-90, 91, 3):
            for m in (1.03, 1.21, 1.5, 1.68, 1.9):
                amax = m * 2.0 ** k
                if ref.binade_margin(amax, target) < 1e-3:
                    continue
                want = float(bf16sim._fp8_scale(torch.tensor([amax, -amax / 3], dtype=torch.float64), target))
                assert ref.pow2_scale(amax, target) == want, (target, amax)
                n += 1
    assert n > 500
    # the history values the GPU tests use
    assert ref.pow2_scale(3.0, 224.0) == 64.0 and ref.pow2_scale(0.37, 224.0) == 512.0 and ref.pow2_scale(150.0, 224.0) == 1.0
    assert ref.pow2_scale(3.0, 56.0) == 16.0 and ref.pow2_scale(0.37, 56.0) == 128.0 and ref.pow2_scale(150.0, 56.0) == 0.25
    for h in (3.0, 0.37, 150.0):
        assert ref.binade_margin(h, 224.0) > 0.2 and ref.binade_margin(h, 56.0) > 0.2


def test_scale_of_nothing_recorded_and_the_exponent_clamp():
    for target in (ref.ACT_TARGET, ref.GRAD_TARGET):
        for bad in (None, 0.0, -0.0, float("inf"), float("nan"), 1e-40, 2.0 ** -101, 3.2e38):
            assert ref.pow2_scale(bad, target) == 1.0, bad
        assert float(bf16sim._fp8_scale(torch.zeros(3), target)) == 1.0
        assert ref.pow2_scale(2.0 ** -100 * 1.5, target) == 2.0 ** 100               # floor(log2(T / amax)) = 106 / 104: clamped
        assert ref.pow2_scale(2.9e38, target) == 2.0 ** -100                          # -120 / -122: clamped
        assert ref.pow2_scale(1.5 * 2.0 ** -80, target) == 2.0 ** (87 if target == 224.0 else 85)   # inside: not clamped


def test_e4m3_half_ulp_bound():
    """every finite byte code converts to itself; the conversion of any |v| <= 448 lands within max(2^-4 |v|, 2^-10); above, it
    saturates to +-448 and never to a NaN code"""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    finite = ~ref.is_nan_code(codes)
    assert int(finite.sum()) == 254
    vals = ref.dequant(codes)
    assert torch.isnan(vals[~finite]).all() and vals[finite].abs().max().item() == 448.0
    assert torch.equal(ref.e4m3_bytes(vals[finite]), codes[finite])
    # midpoints between neighbouring codes sit exactly ON the bound (ties), so the bound is not loose by a factor
    pos = vals[1:127]                                                             # 2^-9 .. 448, ascending
    mid = (pos[1:] + pos[:-1]) / 2
    err = (ref.dequant(ref.e4m3_bytes(mid)) - mid).abs()
    assert bool((err <= ref.half_ulp_bound(mid)).all()) and bool((err == (pos[1:] - pos[:-1]) / 2).all())
    g = torch.Generator().manual_seed(7)
    for scale in (2.0 ** -9, 0.02, 1.0, 37.0, 448.0):
        v = ((torch.rand(200000, generator=g) * 2 - 1) * scale)
        for x in (v, v.bfloat16().float()):
            b = ref.e4m3_bytes(x)
            assert not bool(ref.is_nan_code(b).any())
            assert bool(((ref.dequant(b) - x).abs() <= ref.half_ulp_bound(x)).all()), scale
    big = torch.tensor([449.0, 463.9, 464.0, 480.0, 1e6, float("inf"), -500.0])
    assert ref.dequant(ref.e4m3_bytes(big)).tolist() == [448.0] * 6 + [-448.0]


def test_fp32_rounded_bound_covers_a_byte_rounded_before_the_bf16_rounding():
    """contract B: q = e4m3(x s) from the fp32 x, compared with v = bf16(x) s"""
    g = torch.Generator().manual_seed(11)
    for s in (0.25, 16.0, 128.0):
        x = torch.randn(200000, generator=g) * 2.5
        q = ref.dequant(ref.e4m3_bytes(x * s))
        v = (x.bfloat16().float() * s).clamp(-448, 448)
        assert bool(((q - v).abs() <= ref.fp32_rounded_bound(v)).all()), s
        # and it is a real condition: a byte one code off breaks it for most elements
        off = ref.dequant((ref.e4m3_bytes(x * s).to(torch.int32) + 1).clamp(max=0x7E).to(torch.uint8))
        assert float(((off - v).abs() > ref.fp32_rounded_bound(v)).float().mean()) > 0.5


def test_bf16_rounding_is_monotone_so_the_max_commutes():
    g = torch.Generator().manual_seed(3)
    for n, s in ((1, 1.0), (7, 1e-3), (4096, 1.0), (100000, 37.0), (100000, 1e4)):
        x = torch.randn(n, generator=g) * s
        assert x.abs().max().bfloat16().item() == x.bfloat16().abs().max().item()
    # ties and neighbours of a bf16 midpoint: 1 + 2^-8 rounds to even (1.0), the next fp32 above it rounds up
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -(1.0 + 2.0 ** -7)])
    assert x.bfloat16().tolist() == [1.0, 1.0, 1.0078125, -1.0078125]
    assert x.abs().max().bfloat16().item() == x.bfloat16().abs().max().item()


def test_slot_positions():
    W = hb.AMAX_TENSOR_WORDS
    pos = ref.slot_positions(W)
    assert len(pos) == ref.SLOTS == 16 and pos[0] == 0 and pos[-1] < W
    assert all(b - a == W // 16 for a, b in zip(pos, pos[1:]))
    assert (W // 16) * 4 == 256                     # 256 bytes apart: one word per memory channel (include/nbest_hip.h)
    assert torch.equal(ref.float_bits(1.0), torch.tensor([0x3F800000], dtype=torch.int32))
    assert math.isinf(ref.float_bits(float("inf")).view(torch.float32).item())
