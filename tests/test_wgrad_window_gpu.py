"""nbest_wgrad_window: a launch that covers sub-ranges of the tiles of up to 16 weight gradients, against nbest_wgrad_group on the same
problems.  It is the same kernel program and the same order over K, a tile by one workgroup: the results are bit-equal, no tolerance.
Shapes: the smallest that cut a problem mid-row and mid-group, K = 200 token rows (6.25 stages of 32: the zero-filled tail)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 200
SHAPES = [(768, 768), (256, 768), (768, 256)]      # 3 x 3, 1 x 3 (wider than tall: groups of 3 tile columns), 3 x 1 tiles
SENTINEL = 7.0


def _tile_coords(t, tiles_m, tiles_n):
    """tile id -> (tile row, tile column) in the order of nbest_wgrad_group (include/nbest_hip.h)"""
    gn = 3 if (tiles_n > tiles_m and tiles_n % 3 == 0) else tiles_n
    g, r = divmod(t, tiles_m * gn)
    return r // gn, g * gn + r % gn


def _operands(shapes, k=K, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).bfloat16()
    return [(r(k, m), r(k, n)) for m, n in shapes]


@pytest.fixture(scope="module")
def problems():
    return _operands(SHAPES)


@pytest.fixture(scope="module")
def grouped(problems):
    from nbest_amd import hipabi as hb
    outs = hb.wgrad_group(problems)
    torch.cuda.synchronize()
    return outs


def _launches(p):
    """three windows that cut the first problem mid-row and the third mid-problem"""
    return [[(0, 0, 5)], [(0, 5, 4), (1, 0, 3), (2, 0, 2)], [(2, 2, 1)]]


def _run(hb, p, outs, launches, accumulate=False):
    for w in launches:
        hb.wgrad_window([(p[i][0], p[i][1], f, c) for i, f, c in w], outs=[outs[i] for i, _, _ in w], accumulate=accumulate)
    torch.cuda.synchronize()


def test_three_windows_equal_the_grouped_launch(problems, grouped):
    from nbest_amd import hipabi as hb
    outs = [torch.full(s, SENTINEL, device="cuda") for s in SHAPES]
    _run(hb, problems, outs, _launches(problems))
    for o, g in zip(outs, grouped):
        assert torch.equal(o, g)


def test_first_window_writes_its_tiles_only(problems, grouped):
    from nbest_amd import hipabi as hb
    outs = [torch.full(s, SENTINEL, device="cuda") for s in SHAPES]
    _run(hb, problems, outs, _launches(problems)[:1])
    inside = {_tile_coords(t, 3, 3) for t in range(5)}
    for tm in range(3):
        for tn in range(3):
            got = outs[0][256 * tm:256 * tm + 256, 256 * tn:256 * tn + 256]
            if (tm, tn) in inside:
                assert torch.equal(got, grouped[0][256 * tm:256 * tm + 256, 256 * tn:256 * tn + 256]), (tm, tn)
            else:
                assert (got == SENTINEL).all(), (tm, tn)
    assert (outs[1] == SENTINEL).all() and (outs[2] == SENTINEL).all()


def test_cut_inside_a_group_of_three_tile_columns():
    """512 x 1536 = 2 x 6 tiles, wider than tall: tile ids run over the 2 x 3 tiles of a column group first, so [0, 4) ends inside the
    first group (tile row 1, column 0) and the untouched tiles keep the sentinel"""
    from nbest_amd import hipabi as hb
    (dY, X), = _operands([(512, 1536)], seed=12)
    ref, = hb.wgrad_group([(dY, X)])
    out = torch.full((512, 1536), SENTINEL, device="cuda")
    hb.wgrad_window([(dY, X, 0, 4)], outs=[out])
    torch.cuda.synchronize()
    inside = {_tile_coords(t, 2, 6) for t in range(4)}
    assert inside == {(0, 0), (0, 1), (0, 2), (1, 0)}
    for tm in range(2):
        for tn in range(6):
            got = out[256 * tm:256 * tm + 256, 256 * tn:256 * tn + 256]
            want = ref[256 * tm:256 * tm + 256, 256 * tn:256 * tn + 256]
            assert torch.equal(got, want) if (tm, tn) in inside else (got == SENTINEL).all(), (tm, tn)
    hb.wgrad_window([(dY, X, 4, 8)], outs=[out])
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_accumulate_adds(problems):
    from nbest_amd import hipabi as hb
    g = torch.Generator(device="cuda").manual_seed(4)
    old = [torch.randn(*s, device="cuda", generator=g) * 30.0 for s in SHAPES]
    want = [o.clone() for o in old]
    hb.wgrad_group(problems, outs=want, accumulate=True)
    outs = [o.clone() for o in old]
    _run(hb, problems, outs, _launches(problems), accumulate=True)
    for o, w, b in zip(outs, want, old):
        assert torch.equal(o, w) and not torch.equal(o, b)


def test_two_runs_are_bit_equal(problems):
    from nbest_amd import hipabi as hb
    a = [torch.full(s, SENTINEL, device="cuda") for s in SHAPES]
    b = [torch.full(s, -SENTINEL, device="cuda") for s in SHAPES]
    _run(hb, problems, a, _launches(problems))
    _run(hb, problems, b, _launches(problems))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_write_nothing(problems):
    """NBEST_ERR_ARG (-1) before anything is enqueued: the outputs keep the sentinel"""
    from nbest_amd import hipabi as hb
    outs = [torch.full(s, SENTINEL, device="cuda") for s in SHAPES]
    p = problems
    e = lambda i, f, c: (p[i][0], p[i][1], f, c)

    def refused(entries, out_ids):
        with pytest.raises(RuntimeError) as err:
            hb.wgrad_window(entries, outs=[outs[i] for i in out_ids])
        torch.cuda.synchronize()
        assert re.search(r"failed \(-1\)", str(err.value)), str(err.value)
        assert all((o == SENTINEL).all() for o in outs)

    refused([e(0, i % 9, 1) for i in range(17)], [0] * 17)                  # a 17th entry
    refused([e(0, 0, 5), e(1, 1, 0)], [0, 1])                               # an empty range
    refused([e(0, 0, 5), e(2, 2, 2)], [0, 2])                               # past the problem's last tile
    refused([e(0, 0, 5), e(2, -1, 2)], [0, 2])                              # before its first
    (dY2, X2), = _operands([(768, 768)], k=K + 64, seed=13)
    refused([e(0, 0, 5), (dY2, X2, 5, 4)], [0, 0])                          # differing K
    # more than 256 tiles: 17 x 16 tiles of one problem
    (dYb, Xb), = _operands([(17 * 256, 16 * 256)], k=64, seed=14)
    big = torch.full((17 * 256, 16 * 256), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError) as err:
        hb.wgrad_window([(dYb, Xb, 0, 257)], outs=[big])
    torch.cuda.synchronize()
    assert re.search(r"failed \(-1\)", str(err.value)), str(err.value)
    assert (big == SENTINEL).all()
    # ... and exactly 256 of them run
    hb.wgrad_window([(dYb, Xb, 0, 256)], outs=[big])
    ref, = hb.wgrad_group([(dYb, Xb)])
    torch.cuda.synchronize()
    assert torch.equal(big[:16 * 256], ref[:16 * 256]) and (big[16 * 256:] == SENTINEL).all()
