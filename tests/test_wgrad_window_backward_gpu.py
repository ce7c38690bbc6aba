"""Whole backward with the weight gradients in rolling windows of 256 tiles (NBEST_WGRAD_GROUP_WINDOW) against the grouped launches
(ALWAYS) and the split-K launches (NEVER) on the committed cases' inputs, bf16.  A window launch runs the grouped launch's program,
a tile by one workgroup over the whole K in the same order: its matrices are bit-equal to ALWAYS.  The peeled QKV + attention-out
pair of the range's lowest layer runs the launches of NEVER: bit-equal to NEVER.  Everything else - biases, LayerNorm parameters,
embeddings, the input gradient - does not pass through the changed code: bit-equal to both.  bert_L12 (12 x 108 tiles: five
windows and the peeled pair, the four dY buffer sets wrap twice), xlmrL_L4_S256 (4 x 192 tiles: three full windows, two sets)."""
import functools

import pytest
import torch

from conftest import load_case
from test_wgrad_group_backward_gpu import _is_layer_matrix, _model, _run, _step

pytestmark = pytest.mark.gpu

NEVER, ALWAYS, WINDOW = 1, 2, 3
FROZEN = tuple("bert_encoder.encoder.layer.%d." % l for l in range(6))
SIX_CHUNKS = tuple((l, l + 2) for l in range(0, 12, 2))


@functools.lru_cache(maxsize=None)
def _grads(name, mode, freeze=None, chunks=None, micro_batches=1, drop=0.0):
    """(gradient slots, dhidden) of one run; computed once per configuration, shared by the tests, never modified"""
    from conftest import ROOT  # noqa: F401
    import nbest_amd  # noqa: F401
    from nbest_amd.config import LabelSpace
    import os
    labels = LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
    _, g = _run(name, labels, mode, freeze=list(freeze) if freeze else None, chunks=list(chunks) if chunks else None,
                micro_batches=micro_batches, drop=drop)
    return g


def _peeled(name, layer):
    return (".encoder.layer.%d." % layer) in name and ("attention.self." in name or name.endswith("attention.output.dense.weight"))


def _compare(name, peel_layer, n_matrices, **kw):
    (gn, dhn), (ga, dha), (gw, dhw) = (_grads(name, m, **kw) for m in (NEVER, ALWAYS, WINDOW))
    n_win = n_peel = 0
    for k in gw:
        if not _is_layer_matrix(k):
            assert torch.equal(gw[k], ga[k]) and torch.equal(gw[k], gn[k]), "%s is not bit-equal to both" % k
        elif peel_layer is not None and _peeled(k, peel_layer):
            assert torch.equal(gw[k], gn[k]), "%s (peeled) is not bit-equal to the split-K launches" % k
            n_peel += 1
        else:
            assert torch.equal(gw[k], ga[k]), "%s is not bit-equal to the grouped launch" % k
            n_win += bool(gw[k].abs().max().item() > 0)          # (a frozen matrix: no gradient written by any path)
    assert torch.equal(dhw, dha) and torch.equal(dhw, dhn), "dhidden is not bit-equal"
    assert n_win + n_peel == n_matrices and n_peel == (4 if peel_layer is not None else 0)


def test_launches_per_layer_and_schedule(labels):
    """the descriptor the model builds for bert_L12 resolves to five windows and the peeled pair of layer 0 over four buffer sets"""
    import ctypes as C
    from nbest_amd import hipabi as hb
    assert (hb.WGRAD_GROUP_NEVER, hb.WGRAD_GROUP_ALWAYS, hb.WGRAD_GROUP_WINDOW) == (NEVER, ALWAYS, WINDOW)
    meta, _ = load_case("bert_L12")
    m, _ = _model(meta, labels, WINDOW)
    d = m._desc(meta["B"], meta["S"], 0).desc
    plan = hb.encoder_wgrad_plan(d, 0, 12)
    assert (plan["mode"], plan["sets"], plan["peel_layer"]) == (WINDOW, 4, 0)
    assert [w["tiles"] for w in plan["launches"]] == [256, 256, 256, 256, 236]
    assert hb.lib().nbest_encoder_wgrad_launches_per_layer(C.byref(d)) == 1


def test_whole_range():
    _compare("bert_L12", peel_layer=0, n_matrices=6 * 12)


def test_frozen_lower_layers():
    """layers 0..5 frozen: 648 tiles, three rounds with or without the pair - nothing is peeled"""
    _compare("bert_L12", peel_layer=None, n_matrices=6 * 6, freeze=FROZEN)
    _compare("bert_L12", peel_layer=None, n_matrices=6 * 6, freeze=FROZEN + ("bert_encoder.embeddings.",))


def test_chunked_calls_flush_inside_each_call():
    _compare("bert_L12", peel_layer=None, n_matrices=6 * 12, chunks=((0, 1), (1, 12)))
    _compare("bert_L12", peel_layer=None, n_matrices=6 * 12, chunks=SIX_CHUNKS)


def test_two_accumulating_micro_batches():
    _compare("bert_L12", peel_layer=0, n_matrices=6 * 12, micro_batches=2)


def test_hidden_dropout():
    """the dense-branch gradients out of the LayerNorm backwards are buffers of their own: bert_L2 (two sets), and bert_L12, where the
    layers rotate over all four sets"""
    _compare("bert_L2", peel_layer=None, n_matrices=6 * 2, drop=0.1)
    _compare("bert_L12", peel_layer=0, n_matrices=6 * 12, drop=0.1)


def test_xlm_roberta_large_layers():
    """192 tiles per layer: 768 = 3 x 256, windows cut every layer, two buffer sets; both passes of the step"""
    _compare("xlmrL_L4_S256", peel_layer=None, n_matrices=6 * 4)


def test_bit_reproducible(labels, name="bert_L12"):
    """a second run from the same state, and a second step of the same model: the whole gradient arena is equal"""
    m, _ = _run(name, labels, WINDOW)
    g1 = m.arena.g.clone()
    want, _ = _grads(name, WINDOW)
    for s in m.arena.slots:
        assert torch.equal(m.arena.view(g1, s.name), want[s.name]), s.name
    meta, _ = load_case(name)
    _, b = _model(meta, labels, WINDOW)
    _step(m, b, meta)
    assert torch.equal(m.arena.g, g1)
