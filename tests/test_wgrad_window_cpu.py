"""Weight gradients in rolling windows of 256 tiles (NBEST_WGRAD_GROUP_WINDOW), on the host: the schedule nbest_encoder_wgrad_plan
reports for a backward call - window sizes, the peeled pair, the dY buffer sets, every tile covered exactly once - what the plan
resolves to at the benchmark's and the golden cases' shapes, and the workspace sizes.  Nothing is enqueued: no GPU."""
import ctypes as C
import os

import pytest

NEVER, ALWAYS, WINDOW = 1, 2, 3
BERT = dict(H=768, F=3072)          # 27 + 9 + 36 + 36 = 108 tiles of 256 x 256 per layer
XLMR_LARGE = dict(H=1024, F=4096)   # 48 + 16 + 64 + 64 = 192


def _lib():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    assert os.path.exists(hb.LIB_PATH), "libnbest_hip.so is not built (it builds without a GPU): nothing here may pass without it"
    assert (hb.WGRAD_GROUP_PLAN, hb.WGRAD_GROUP_NEVER, hb.WGRAD_GROUP_ALWAYS, hb.WGRAD_GROUP_WINDOW) == (0, NEVER, ALWAYS, WINDOW)
    return hb, hb.lib()


def _desc(hb, L, B, S, H, F, mode=0, first_trainable=0, skip=None):
    d = hb.EncoderDesc()
    d.dtype = hb.BF16
    d.B, d.S, d.H, d.L, d.heads, d.F = B, S, H, L, H // 64, F
    d.vocab, d.max_pos, d.n_types = 300, 514, 2
    d.pos_pad_id = -1
    d.first_trainable = first_trainable
    d.wgrad_group = mode
    if skip is not None:
        d._skip = (C.c_uint8 * (4 * L))(*skip)      # kept alive with the descriptor
        d.wgrad_skip_host = C.cast(d._skip, C.c_void_p)
    return d


def _matrix_tiles(H, F):
    h, f = H // 256, F // 256
    return [3 * h * h, h * h, f * h, h * f]


def _coverage(plan, lo, hi):
    """tiles of every (layer, matrix) the window launches cover, asserting order and no overlap; launches lie inside the call"""
    seen = {}
    order = []
    for w in plan["launches"]:
        assert lo <= w["after_layer"] < hi
        assert 1 <= len(w["entries"]) <= 16 and w["tiles"] == sum(e[3] for e in w["entries"]) <= 256
        for layer, j, first, count in w["entries"]:
            assert layer >= w["after_layer"], "a window cannot hold tiles of a layer that has not run yet"
            assert count >= 1 and first == seen.get((layer, j), 0), "ranges of a matrix follow each other without gap or overlap"
            seen[(layer, j)] = first + count
            if (layer, j) not in order:
                order.append((layer, j))
    assert order == sorted(order, key=lambda k: (-k[0], k[1])), "highest layer first, QKV | attention-out | FFN-up | FFN-down"
    return seen


def _check_range(hb, d, lo, hi, shape, skip=None, want_peel=None):
    plan = hb.encoder_wgrad_plan(d, lo, hi)
    assert plan["mode"] == WINDOW
    t = _matrix_tiles(**shape)
    seen = _coverage(plan, lo, hi)
    want = {}
    for l in range(lo, hi):
        for j in range(4):
            if skip and skip[4 * l + j]:
                continue
            if l == plan["peel_layer"] and j < 2:
                continue
            want[(l, j)] = t[j]
    assert seen == want
    assert plan["peel_layer"] in (-1, lo), "only the lowest layer of the range is peeled"
    if want_peel is not None:
        assert plan["peel_layer"] == want_peel
    # every launch but those at the end of the call is a full round (skipped matrices: a flush may come early, to free a buffer set)
    for w in plan["launches"]:
        if w["after_layer"] != lo and not skip:
            assert w["tiles"] == 256
    # buffer sets: while layer l writes its dY, the layers above it with unlaunched tiles occupy fewer than `sets` sets
    last = {}
    for w in plan["launches"]:
        for layer, _, _, _ in w["entries"]:
            last[layer] = w["after_layer"]         # the layer at whose end the last tile of `layer` goes out
    for l in range(lo, hi):
        live = [k for k in last if k > l and last[k] <= l]
        assert len(live) < plan["sets"], (l, live)
        assert len({(hi - 1 - k) % plan["sets"] for k in live + [l]}) == len(live) + 1, "two live layers share a buffer set"
    return plan


def test_bert_base_headline_shape():
    hb, lib = _lib()
    for mode in (0, WINDOW):     # the plan takes the windows here
        d = _desc(hb, 12, 256, 128, mode=mode, **BERT)
        plan = _check_range(hb, d, 0, 12, BERT, want_peel=0)
        assert [w["tiles"] for w in plan["launches"]] == [256, 256, 256, 256, 236]
        assert plan["sets"] == 4
        assert lib.nbest_encoder_wgrad_launches_per_layer(C.byref(d)) == 1


def test_xlm_roberta_large():
    hb, lib = _lib()
    for mode in (0, WINDOW):
        d = _desc(hb, 24, 64, 256, mode=mode, **XLMR_LARGE)
        plan = _check_range(hb, d, 0, 24, XLMR_LARGE, want_peel=-1)
        assert [w["tiles"] for w in plan["launches"]] == [256] * 18
        assert plan["sets"] == 2


@pytest.mark.parametrize("L,B,S", [(2, 3, 64), (2, 1, 64), (12, 3, 64)])
def test_golden_shapes_keep_todays_modes_under_the_plan(L, B, S):
    """bert_L2 (M = 192 and 64 token rows) and bert_L12 (M = 192): the fixed cost of a launch dominates, the windows' pair launch
    costs more than it saves - and the schedule and the workspace are those of mode NEVER or ALWAYS"""
    hb, lib = _lib()
    d = _desc(hb, L, B, S, mode=0, **BERT)
    plan = hb.encoder_wgrad_plan(d, 0, L)
    assert plan["mode"] in (NEVER, ALWAYS) and plan["launches"] == [] and plan["peel_layer"] == -1
    same = _desc(hb, L, B, S, mode=plan["mode"], **BERT)
    assert lib.nbest_encoder_ws_bytes(C.byref(d)) == lib.nbest_encoder_ws_bytes(C.byref(same))
    assert lib.nbest_encoder_wgrad_launches_per_layer(C.byref(d)) == lib.nbest_encoder_wgrad_launches_per_layer(C.byref(same))


def test_sub_ranges_flush_inside_their_call():
    hb, _ = _lib()
    d = _desc(hb, 12, 256, 128, mode=WINDOW, **BERT)
    plan = _check_range(hb, d, 1, 12, BERT, want_peel=-1)          # 1 188 tiles: 5 rounds with or without the pair
    assert [w["tiles"] for w in plan["launches"]] == [256, 256, 256, 256, 164]
    plan = _check_range(hb, d, 0, 1, BERT, want_peel=-1)           # 108 tiles: one round either way
    assert [w["tiles"] for w in plan["launches"]] == [108]
    for lo in range(0, 12, 2):                                     # the chunks of the data-parallel reducer: today's 216-tile launch
        plan = _check_range(hb, d, lo, lo + 2, BERT, want_peel=-1)
        assert [w["tiles"] for w in plan["launches"]] == [216]
        assert [e[:2] for e in plan["launches"][0]["entries"]] == [(lo + 1, j) for j in range(4)] + [(lo, j) for j in range(4)]
    assert hb.encoder_wgrad_plan(d, 5, 5)["launches"] == []


def test_frozen_layers_and_a_skipped_matrix():
    hb, _ = _lib()
    # layers 0..5 frozen, embeddings too: the range starts at first_trainable = 6; 648 tiles = 256 + 256 + 136, three sets suffice
    d = _desc(hb, 12, 256, 128, mode=WINDOW, first_trainable=6, **BERT)
    plan = _check_range(hb, d, 6, 12, BERT, want_peel=-1)
    assert [w["tiles"] for w in plan["launches"]] == [256, 256, 136] and plan["sets"] == 3
    # layers 0..5 frozen, embeddings trainable: the backward runs through them, their matrices are skipped
    skip = [1] * 24 + [0] * 24
    d = _desc(hb, 12, 256, 128, mode=WINDOW, skip=skip, **BERT)
    plan = _check_range(hb, d, 0, 12, BERT, skip=skip, want_peel=-1)
    assert [w["tiles"] for w in plan["launches"]] == [256, 256, 136] and plan["sets"] == 4
    assert all(w["after_layer"] >= 6 or w["tiles"] == 136 for w in plan["launches"])
    # FFN-up of layer 7 skipped: 1 260 tiles, five rounds without peeling anything
    skip = [0] * 48
    skip[4 * 7 + 2] = 1
    d = _desc(hb, 12, 256, 128, mode=WINDOW, skip=skip, **BERT)
    plan = _check_range(hb, d, 0, 12, BERT, skip=skip, want_peel=-1)
    assert [w["tiles"] for w in plan["launches"]] == [256, 256, 256, 256, 236]
    # only attention-out of every layer trainable: 9 tiles per layer, many layers pending - no more live layers than buffer sets
    skip = [1, 0, 1, 1] * 12
    d = _desc(hb, 12, 256, 128, mode=WINDOW, skip=skip, **BERT)
    _check_range(hb, d, 0, 12, BERT, skip=skip)


def test_workspace_sizes():
    """NEVER and ALWAYS as before (ALWAYS: one [M][H] buffer and a second set of dY buffers more than NEVER); WINDOW: N sets"""
    hb, lib = _lib()
    B, S, H, F = 256, 128, 768, 3072
    M = B * S
    ws = {mode: lib.nbest_encoder_ws_bytes(C.byref(_desc(hb, 12, B, S, H, F, mode=mode))) for mode in (0, NEVER, ALWAYS, WINDOW)}
    one_set = 2 * M * (5 * H + F)                 # dRd after LN2, dBig, dRd after LN1, dqkv, bf16
    assert ws[ALWAYS] - ws[NEVER] == 2 * M * H + one_set
    assert ws[WINDOW] - ws[NEVER] == 2 * M * H + 3 * one_set
    assert ws[0] == ws[WINDOW]
    assert (ws[NEVER], ws[ALWAYS]) == (1000366336, 1503682816)     # the sizes before the windows existed
    for mode, per_layer in ((NEVER, 3), (ALWAYS, 1), (WINDOW, 1)):
        assert lib.nbest_encoder_wgrad_launches_per_layer(C.byref(_desc(hb, 12, B, S, H, F, mode=mode))) == per_layer
    # xlm-roberta-large: 2 sets, the workspace of ALWAYS there (one layer per launch) plus one set
    B, S, H, F = 64, 256, 1024, 4096
    M = B * S
    ws = {mode: lib.nbest_encoder_ws_bytes(C.byref(_desc(hb, 24, B, S, H, F, mode=mode))) for mode in (NEVER, ALWAYS, WINDOW)}
    assert (ws[NEVER], ws[ALWAYS]) == (700469504, 734023936)
    assert ws[WINDOW] - ws[NEVER] == 2 * M * H + 2 * M * (5 * H + F)


def test_shapes_without_whole_tiles_or_with_the_fp8_forward_fall_back():
    hb, lib = _lib()
    d = _desc(hb, 4, 64, 128, H=640, F=2560, mode=WINDOW)          # 640 is not a multiple of 256
    assert hb.encoder_wgrad_plan(d, 0, 4)["mode"] == NEVER
    d = _desc(hb, 4, 64, 128, H=768, F=3072, mode=WINDOW)
    d.dtype = hb.F32
    assert hb.encoder_wgrad_plan(d, 0, 4)["mode"] == NEVER
    d = _desc(hb, 4, 64, 128, H=1536, F=6144, mode=WINDOW)         # 432 tiles per layer: more than a round
    assert hb.encoder_wgrad_plan(d, 0, 4)["mode"] == NEVER
    with pytest.raises(RuntimeError):
        hb.encoder_wgrad_plan(_desc(hb, 4, 64, 128, H=768, F=3072, mode=WINDOW), 2, 5)
