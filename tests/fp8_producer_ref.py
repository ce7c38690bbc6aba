"""Reference side of the fp8 producer tests (tests/test_fp8_producers_gpu.py), in plain Python / torch on the CPU so that
tests/test_fp8_producers_cpu.py can check it without a GPU: the delayed scale, the e4m3 conversion, the rounding bounds and the
positions of the amax slot words.  Restated from the contract in include/nbest_hip.h ("The fp8 PRODUCERS on their own"), not
imported from the library."""
import math

import torch

ACT_TARGET, GRAD_TARGET = 224.0, 56.0        # forward activations: amax -> (112, 224]; gradients: amax -> (28, 56], 8 x headroom
E4M3_MAX = 448.0
SLOTS = 16
HALF_ULP_REL = 2.0 ** -4                      # e4m3 has 3 mantissa bits: ulp = 2^-3 of the binade's power of two, half of it 2^-4
HALF_ULP_SUB = 2.0 ** -10                     # below 2^-6 the step is the subnormal one, 2^-9
BF16_REL = 2.0 ** -7                          # conservative bound on a bf16 rounding (its half ulp is 2^-9 relative)


def pow2_scale(amax, target):
    """2^floor(log2(target / amax)) with the exponent clamped to +-100; 1 for None (null pointer), for an amax that is zero or
    below 2^-100, and for a non-finite one (the code's test is amax <= 3.0e38, so the top sliver of the fp32 range counts as inf)"""
    if amax is None or not (amax >= 7.8886e-31) or not (amax <= 3.0e38):       # NaN fails both comparisons
        return 1.0
    e = math.floor(math.log2(target / amax))
    return 2.0 ** max(-100, min(100, e))


def binade_margin(amax, target):
    """distance of log2(target / amax) from the nearest integer: the tests keep it large, so that no result depends on how a
    log2 rounds at an exact power of two"""
    f = math.log2(target / amax) % 1.0
    return min(f, 1.0 - f)


def e4m3(x):
    """the reference conversion: round to nearest even, saturating (without the clamp torch gives NaN above 464)"""
    return x.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


def e4m3_bytes(x):
    return e4m3(x).view(torch.uint8)


def dequant(b):
    return b.view(torch.float8_e4m3fn).float()


def is_nan_code(b):
    return (b & 0x7F) == 0x7F                 # 0x7F and 0xFF


def half_ulp_bound(v):
    """|e4m3(v) - v| <= this for |v| <= 448"""
    return torch.maximum(HALF_ULP_REL * v.abs(), torch.full_like(v, HALF_ULP_SUB))


def fp32_rounded_bound(v):
    """bound on |q - v| for a byte q rounded from the fp32 value x while v is the bf16 rounding of x (times the same power-of-two
    scale, clamped to +-448): e4m3's half ulp plus the bf16 rounding of the compared tensor"""
    return half_ulp_bound(v) + BF16_REL * v.abs()


def slot_positions(words):
    """the 16 words of a slot block a producer may raise: words / 16 apart, from word 0"""
    assert words % SLOTS == 0
    return [k * (words // SLOTS) for k in range(SLOTS)]


def float_bits(v):
    """int32 holding the bits of the fp32 value v"""
    return torch.tensor([v], dtype=torch.float32).view(torch.int32)
