"""nbest_wgrad_group: up to 8 weight gradients dW_i = dY_i^T . X_i in one launch without K-splits, against an fp64 reference
(torch.matmul of the bf16 operands in double).  Bar, for every element: |dW - ref| <= (K + 2) 2^-24 (|dY|^T |X| + |dW_old|) - the
textbook bound of a length-K fp32 accumulation in any order (products of two bf16 are exact in fp32; dW_old: the gradient added to
under `accumulate`, else 0), computed from the operands."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

H, F = 768, 3072
# (rows of dW = columns of dY, columns of dW = columns of X) of a bert-base layer: QKV, attention-out, FFN-up, FFN-down
LAYER = [(3 * H, H), (H, H), (F, H), (H, F)]


def _operands(shapes, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).bfloat16()
    return [(r(K, m), r(K, n)) for m, n in shapes]


def _check(problems, outs, K, old=None, tag=""):
    for i, ((dY, X), out) in enumerate(zip(problems, outs)):
        ref = dY.double().t() @ X.double()
        mag = dY.double().abs().t() @ X.double().abs()
        if old is not None:
            ref = ref + old[i].double()
            mag = mag + old[i].double().abs()
        bound = (K + 2) * 2.0 ** -24 * mag
        err = (out.double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print("%s problem %d [%d x %d] K=%d: max |err| %.3e, max err/bound %.3e" % (tag, i, out.shape[0], out.shape[1], K, err.max().item(), worst))
        assert torch.isfinite(out).all()
        assert (err <= bound).all(), "%s problem %d: err/bound %.3e" % (tag, i, worst)


@pytest.mark.parametrize("K", [4096, 32768])
@pytest.mark.parametrize("which", ["two_layers", "two_layers_paired_view", "one_left_out"])
def test_two_bert_base_layers(K, which):
    """the gradients of two bert-base layers as the backward groups them (8 problems, 216 tiles); the same with the attention-output
    gradients left out (6 problems: QKV, FFN-up, FFN-down of each layer); and the 8 with one problem left out (a frozen matrix)"""
    from nbest_amd import hipabi as hb
    shapes = LAYER + LAYER
    if which == "two_layers_paired_view":
        shapes = [s for j, s in enumerate(shapes) if j % 4 != 1]
    elif which == "one_left_out":
        shapes = shapes[:5] + shapes[6:]
    problems = _operands(shapes, K, seed=K + len(shapes))
    outs = hb.wgrad_group(problems)
    torch.cuda.synchronize()
    _check(problems, outs, K, tag=which)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_problem_counts(n):
    from nbest_amd import hipabi as hb
    K = 2048 + 32 * 3      # not a multiple of 64: the last stage pair is partly past the last token row
    shapes = [(256 * (1 + i % 3), 256 * (1 + (i * 2) % 5)) for i in range(n)]
    problems = _operands(shapes, K, seed=n)
    outs = hb.wgrad_group(problems)
    torch.cuda.synchronize()
    _check(problems, outs, K, tag="n=%d" % n)


def test_token_count_not_a_multiple_of_the_stage():
    from nbest_amd import hipabi as hb
    K = 1000                # 31.25 stages of 32 rows: rows past the last token are zero-filled by the range check
    problems = _operands([(256, 512), (512, 256)], K, seed=5)
    outs = hb.wgrad_group(problems)
    torch.cuda.synchronize()
    _check(problems, outs, K, tag="K=1000")


def test_accumulate_on_nonzero_gradient():
    from nbest_amd import hipabi as hb
    K = 4096
    problems = _operands(LAYER, K, seed=3)
    g = torch.Generator(device="cuda").manual_seed(4)
    old = [torch.randn(m, n, device="cuda", generator=g) * 30.0 for m, n in LAYER]
    outs = [o.clone() for o in old]
    hb.wgrad_group(problems, outs=outs, accumulate=True)
    torch.cuda.synchronize()
    _check(problems, outs, K, old=old, tag="accumulate")


def test_matches_split_k_launch_closely_and_is_reproducible():
    """same operands through nbest_gemm (split-K + reduce): both within the bound of the fp64 reference, hence within twice the bound of
    each other; two grouped launches are bit-equal"""
    from nbest_amd import hipabi as hb
    K = 8192
    problems = _operands(LAYER, K, seed=9)
    a = hb.wgrad_group(problems)
    b = hb.wgrad_group(problems)
    torch.cuda.synchronize()
    for (dY, X), x, y in zip(problems, a, b):
        assert torch.equal(x, y)
        s = hb.gemm(dY, X, dY.shape[1], X.shape[1], K, 1, 1, hb.EPI_F32_SPLITK)
        bound = 2 * (K + 2) * 2.0 ** -24 * (dY.double().abs().t() @ X.double().abs())
        assert ((x.double() - s.double()).abs() <= bound).all()


def test_refuses_rows_not_a_multiple_of_256():
    """NBEST_ERR_SHAPE (-2), nothing launched: the output keeps its contents"""
    import ctypes as C
    from nbest_amd import hipabi as hb
    K = 1024
    (dY, X), = _operands([(384, 256)], K, seed=1)
    out = torch.full((384, 256), 7.0, device="cuda")
    with pytest.raises(RuntimeError) as e:
        hb.wgrad_group([(dY, X)], outs=[out])
    torch.cuda.synchronize()
    assert re.search(r"failed \(-2\)", str(e.value)), str(e.value)
    assert (out == 7.0).all()
    # a good problem next to a bad one is not launched either
    good = _operands([(256, 256)], K, seed=2)[0]
    out2 = torch.full((256, 256), 7.0, device="cuda")
    with pytest.raises(RuntimeError):
        hb.wgrad_group([good, (dY, X)], outs=[out2, out])
    torch.cuda.synchronize()
    assert (out2 == 7.0).all() and (out == 7.0).all()
    with pytest.raises(RuntimeError):
        hb.wgrad_group([good] * 9)
    assert C.sizeof(hb.EncoderDesc) % 8 == 0
