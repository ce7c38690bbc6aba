"""CPU: where the bounds of tests/test_optim_kernels_gpu.py come from.  The reference's own fp32 arithmetic (torch CPU ops in the
reference's order, tests/optim_ref.py::leg_step) against the fp64 statement of each rule on the hand-built table, three chained
steps: its worst error ratios are the LEG_WORST the bound factors K = ceil(4 x LEG_WORST) are derived from, and the same leg with
the constants float32(1) - float32(b) - what adam1 of csrc/optim.hip formed before it was given (float)(1 - b) - breaks K."""
import math

import pytest

import optim_ref as R


@pytest.fixture(scope="module")
def tab():
    return R.table()


@pytest.mark.parametrize("rule", R.RULES)
def test_reference_leg_stays_inside_what_the_bounds_assume(rule, tab):
    """every ratio of the fp32 leg is under 16 x 2^-24 (a cap on the reference leg, not on the kernel) and under the LEG_WORST entry the
    kernel test's K is 4 x of"""
    worst = R.run_legs(rule, tab)
    R.log("optim-leg %-8s fp32 reference leg vs fp64, worst ratios in 2^-24: m %.2f  v %.2f  p %.2f   K = 4 x, rounded up: m %d  v %d  p %d"
          % (rule, worst["m"], worst["v"], worst["p"], R.K[rule]["m"], R.K[rule]["v"], R.K[rule]["p"]))
    for q in R.QUANTITIES:
        assert worst[q] < 16, (rule, q, worst[q])
        assert worst[q] <= R.LEG_WORST[rule][q], (rule, q, worst[q])
        assert R.K[rule][q] == math.ceil(4 * R.LEG_WORST[rule][q])
    # a quantity that does not move would make its bound empty
    assert min(worst.values()) > 0.25


def test_float_formed_constants_break_the_bound(tab):
    """BertAdam's leg with 1.f - 0.999f = 0.0009999871 in place of float32(1 - 0.999) = 0.001: v comes out 1.29e-5 (217 x 2^-24) too
    small and the update about 100 x 2^-24 too large - both beyond the kernel test's K, which therefore fails on a kernel that forms
    the constants that way"""
    worst = R.run_legs("bertadam", tab, float_formed=True)
    R.log("optim-leg bertadam with float32(1) - float32(b): m %.2f  v %.2f  p %.2f" % (worst["m"], worst["v"], worst["p"]))
    assert worst["v"] > R.K["bertadam"]["v"] and worst["v"] > 200
    assert worst["p"] > R.K["bertadam"]["p"]
    assert worst["m"] <= R.K["bertadam"]["m"]       # float32(1) - float32(0.9) is 1 ulp from float32(0.1): inside the bound


def test_bound_on_v_resolves_the_constant():
    """K_v 2^-24 <= 1.29e-5 / 4: the bound on v is at most a quarter of the relative error of 1.f - 0.999f"""
    off = abs(float(R.np.float32(1) - R.np.float32(0.999)) - R.f32(1 - 0.999)) / R.f32(1 - 0.999)
    assert 1.28e-5 < off < 1.30e-5
    for rule in R.RULES:
        assert R.K[rule]["v"] * R.EPS <= 1.29e-5 / 4, rule


def test_table_has_the_layout_edges(tab):
    ts = tab.tensors
    assert [t.numel for t in ts] == [1, 3, 4, 255, 16383, 16384, 16385, 40000, 64 * 16384 + 5]
    assert [t.numel for t in ts if t.offset % 4] == [255, 40000]
    assert [t.numel for t in ts if not t.active] == [16385]
    assert [t.numel for t in ts if t.active and t.gnorm == 0.0] == [16384]
    assert any(t.gnorm > 10 for t in ts) and any(0 < t.gnorm < 0.1 for t in ts)
    assert len({t.lr for t in ts}) == 3 and {t.wd for t in ts} == {0.0, 0.01}
    assert (ts[-1].numel + R.CHUNK - 1) // R.CHUNK == 65 and tab.n_blocks == 76
    g, (p, m, v) = R.grad(tab, 100), R.state(tab)
    cov = R.covered(tab)
    assert (g[~cov] == 3 * R.GUARD).all() and (p[~cov] == -R.GUARD).all() and (v[cov] > 0).all()
    partial, coef, clip, total = R.ref_norms(tab, g, 1.0)
    for i, t in enumerate(ts):
        if t.active and t.gnorm:
            assert abs(math.sqrt(partial[t.block_start:t.block_start + (t.numel + R.CHUNK - 1) // R.CHUNK].sum().item()) - t.gnorm) < 1e-4 * t.gnorm
            assert (coef[i] == 1.0) == (t.gnorm < 1.0)
        else:
            assert coef[i] == 1.0 and partial[t.block_start] == 0.0
    assert clip < 0.05 and total > 30
