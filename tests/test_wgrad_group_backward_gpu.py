"""Whole backward with the weight gradients of two layers grouped into one launch (nbest_encoder_desc.wgrad_group) against the split-K
launches of every layer, on the committed cases' inputs, bf16.  A wiring check, not an accuracy bar (the kernel's bar is in
test_wgrad_group_gpu.py): per weight matrix the relative Frobenius difference is at most 1e-4 - a misplaced tile, a swapped operand or a
stale dY buffer gives a difference of order 1, the other summation order over the tokens one of order 1e-7.  Biases, LayerNorm
parameters, embeddings and the input gradient do not pass through the changed code: bit-equal."""
import pytest
import torch

from conftest import load_case, case_inputs

pytestmark = pytest.mark.gpu

MATRICES = ("attention.self.query.weight", "attention.self.key.weight", "attention.self.value.weight", "attention.output.dense.weight",
            "intermediate.dense.weight", "output.dense.weight")


def _is_layer_matrix(name):
    return ".encoder.layer." in name and name.endswith(MATRICES)


def _model(meta, labels, mode, drop=0.0):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    from nbest_amd.model import NBestSTCModel
    cfg, sd, batch = case_inputs(meta, labels)
    if drop:
        cfg = ncfg.bert_base(num_hidden_layers=meta["L"], hidden_dropout_prob=drop, attention_probs_dropout_prob=drop)
    m = NBestSTCModel(cfg, labels, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0, seed=1, wgrad_group=mode)
    m.load_reference_state(sd)
    m.train()
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    return m, b


def _step(m, b, meta, **kw):
    out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                             trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"], **kw)
    torch.cuda.synchronize()
    return out


def _grads(m):
    return {s.name: m.arena.view(m.arena.g, s.name).clone() for s in m.arena.slots}, m._dh.clone()


def _run(name, labels, mode, freeze=None, chunks=None, micro_batches=1, drop=0.0):
    meta, _ = load_case(name)
    m, b = _model(meta, labels, mode, drop)
    if freeze:
        for n, p in m.named_parameters():
            if any(n.startswith(pre) for pre in freeze):
                p.requires_grad = False
    m.zero_grad()
    for i in range(micro_batches):
        bb = b if i == 0 else {k: v.flip(0).contiguous() for k, v in b.items()}
        _step(m, bb, meta, chunks=chunks, accumulate=i > 0)
    return m, _grads(m)


def _compare(a, b, tag):
    (ga, dha), (gb, dhb) = a, b
    n_mat = 0
    for name in ga:
        x, y = ga[name], gb[name]
        if _is_layer_matrix(name):
            den = x.double().norm().item()
            if den == 0.0:                       # a frozen matrix: no gradient written by either path
                assert torch.equal(x, y), name
                continue
            rel = (x.double() - y.double()).norm().item() / den
            print("%s %-70s rel. Frobenius difference %.3e" % (tag, name, rel))
            assert rel <= 1e-4, "%s %s: %.3e" % (tag, name, rel)
            n_mat += 1
        else:
            assert torch.equal(x, y), "%s %s is not bit-equal" % (tag, name)
    assert torch.equal(dha, dhb), "%s: dhidden is not bit-equal" % tag
    return n_mat


@pytest.mark.parametrize("name", ["bert_L2", "bert_L12"])
def test_grouped_backward_matches_split_k_backward(name, labels):
    from nbest_amd import hipabi as hb
    _, never = _run(name, labels, hb.WGRAD_GROUP_NEVER)
    m, always = _run(name, labels, hb.WGRAD_GROUP_ALWAYS)
    assert _compare(never, always, name) == 6 * m.cfg.num_hidden_layers
    # what the plan chooses for this shape is one of the two, bit for bit
    _, plan = _run(name, labels, hb.WGRAD_GROUP_PLAN)
    same = lambda p, q: all(torch.equal(p[0][k], q[0][k]) for k in p[0])
    assert same(plan, never) or same(plan, always)


def test_grouped_backward_with_frozen_lower_layers(labels):
    """layers 0..5 of bert_L12 frozen: their matrices are not in the table (embeddings trainable: the backward still runs through them)"""
    from nbest_amd import hipabi as hb
    freeze = ["bert_encoder.encoder.layer.%d." % l for l in range(6)]
    _, never = _run("bert_L12", labels, hb.WGRAD_GROUP_NEVER, freeze=freeze)
    _, always = _run("bert_L12", labels, hb.WGRAD_GROUP_ALWAYS, freeze=freeze)
    assert _compare(never, always, "frozen 0..5") == 6 * 6
    # ... and with the embeddings frozen too (first_trainable = 6: the backward stops there)
    freeze = freeze + ["bert_encoder.embeddings."]
    _, never = _run("bert_L12", labels, hb.WGRAD_GROUP_NEVER, freeze=freeze)
    _, always = _run("bert_L12", labels, hb.WGRAD_GROUP_ALWAYS, freeze=freeze)
    assert _compare(never, always, "frozen emb + 0..5") == 6 * 6


@pytest.mark.parametrize("name", ["bert_L2", "bert_L12"])
def test_grouped_backward_odd_layer_range(name, labels):
    """backward calls over [1, L) and [0, 1): a group never crosses a call's range, a layer without a partner goes alone"""
    from nbest_amd import hipabi as hb
    meta, _ = load_case(name)
    chunks = [(0, 1), (1, meta["L"])]
    _, never = _run(name, labels, hb.WGRAD_GROUP_NEVER, chunks=chunks)
    _, always = _run(name, labels, hb.WGRAD_GROUP_ALWAYS, chunks=chunks)
    _compare(never, always, name + " layer_begin=1")
    _, whole = _run(name, labels, hb.WGRAD_GROUP_ALWAYS)
    _compare(whole, always, name + " whole range vs chunks")


@pytest.mark.parametrize("name", ["bert_L2", "bert_L12"])
def test_grouped_backward_accumulates_over_micro_batches(name, labels):
    from nbest_amd import hipabi as hb
    _, never = _run(name, labels, hb.WGRAD_GROUP_NEVER, micro_batches=2)
    _, always = _run(name, labels, hb.WGRAD_GROUP_ALWAYS, micro_batches=2)
    _compare(never, always, name + " two micro-batches")


def test_grouped_backward_with_dropout(labels):
    """hidden dropout > 0: the dense-branch gradients out of the LayerNorm backwards are buffers of their own (the masks are
    regenerated from the seed: the same in both runs)"""
    from nbest_amd import hipabi as hb
    _, never = _run("bert_L2", labels, hb.WGRAD_GROUP_NEVER, drop=0.1)
    _, always = _run("bert_L2", labels, hb.WGRAD_GROUP_ALWAYS, drop=0.1)
    _compare(never, always, "dropout 0.1")


@pytest.mark.parametrize("name", ["bert_L2", "bert_L12"])
def test_grouped_step_is_bit_reproducible(name, labels):
    """two runs of the grouped step from the same state: the whole gradient arena is equal"""
    from nbest_amd import hipabi as hb
    m1, _ = _run(name, labels, hb.WGRAD_GROUP_ALWAYS)
    m2, _ = _run(name, labels, hb.WGRAD_GROUP_ALWAYS)
    assert torch.equal(m1.arena.g, m2.arena.g)
    # ... and a second step of the same model on the same batch, gradients overwritten
    meta, _ = load_case(name)
    _, b = _model(meta, labels, hb.WGRAD_GROUP_ALWAYS)
    g1 = m1.arena.g.clone()
    _step(m1, b, meta)
    assert torch.equal(m1.arena.g, g1)


def test_launch_count_follows_the_plan(labels):
    """nbest_encoder_wgrad_launches_per_layer: 1 where the gradients are grouped, 3 for the paired split-K launches; the workspace
    holds the second set of dY buffers only then"""
    import ctypes as C
    from nbest_amd import hipabi as hb
    meta, _ = load_case("bert_L2")
    sizes = {}
    for mode in (hb.WGRAD_GROUP_NEVER, hb.WGRAD_GROUP_ALWAYS):
        m, _ = _model(meta, labels, mode)
        d = m._desc(256, 128, 0).desc
        sizes[mode] = hb.lib().nbest_encoder_ws_bytes(C.byref(d))
        assert hb.lib().nbest_encoder_wgrad_launches_per_layer(C.byref(d)) == (3 if mode == hb.WGRAD_GROUP_NEVER else 1)
    M, H, F = 256 * 128, 768, 3072
    assert sizes[hb.WGRAD_GROUP_ALWAYS] - sizes[hb.WGRAD_GROUP_NEVER] == 2 * M * (3 * H + F + 3 * H)
