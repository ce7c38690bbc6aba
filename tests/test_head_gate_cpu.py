"""CPU: head gates and head importance - the fp64 reference the GPU tests compare against (a per-utterance gate on the oracle's
attention.self output, its autograd gradient checked by central differences), the exports and descriptor fields, --head_mask
parsing, trainer.prune_lowest, the importance aggregation and the CLI flag errors."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_case
from test_attrib_cpu import oracle_model


# ---- the fp64 reference: a gate on every head's attention output, the training loss restated in oracle/step.py -----------------
def mixed_mask(L, heads):
    """the non-trivial mask of these tests: zeros, a 0.5 and ones in every layer"""
    m = torch.ones(L, heads, dtype=torch.float64)
    for l in range(L):
        m[l, (3 * l + 1) % heads] = 0.0
        m[l, (5 * l + 4) % heads] = 0.0
        m[l, (2 * l + 7) % heads] = 0.5
    return m

def oracle_gated(m, ocfg, labels, ids, seg, y, gate, want_grad=True):
    """The oracle with a gate on every head: ``gate`` [L, B, heads] (or [L, heads], the same for every utterance) multiplies the
    [B, S, H] output of each layer's attention.self (a forward hook), expanded over the head dimension d - HF's head_mask.
    Returns (top, bottoms, final, total loss, grad [L, B, heads] = d total / d gate): the loss is oracle.stc.total_loss as
    oracle/step.py calls it without the MSE term, a sum over utterances, so grad[:, b] is the gradient of utterance b's loss."""
    from oracle import stc
    layers = m.bert_encoder.encoder.layer
    L, heads = len(layers), ocfg.num_attention_heads
    d = ocfg.hidden_size // heads
    B = ids.shape[0]
    g = gate.to(next(m.parameters()).dtype)
    if g.dim() == 2:
        g = g[:, None, :].expand(L, B, heads)
    g = g.detach().clone().requires_grad_(want_grad)
    hooks = [lyr.attention.self.register_forward_hook(lambda mod, inp, out, l=l: out * g[l].repeat_interleave(d, dim=-1)[:, None, :])
             for l, lyr in enumerate(layers)]
    try:
        top, bottoms, final, asr, _ = m(ids, None, seg_ids=seg)
    finally:
        for h in hooks:
            h.remove()
    b2t = stc.bottom2top_matrix(labels.top2bottom).to(top.dtype)
    _, total, _ = stc.total_loss(top, bottoms, final, y.to(top.dtype), labels.top2bottom, b2t)
    grad = torch.autograd.grad(total, g)[0].detach() if want_grad else None
    return top.detach(), {k: v.detach() for k, v in bottoms.items()}, final.detach(), total.detach(), grad

def case_tensors(meta, batch):
    ids = torch.from_numpy(batch["ids"])
    seg = torch.from_numpy(batch["seg"]) if meta["seg"] else None
    return ids, seg, torch.from_numpy(batch["labels"])

def test_oracle_gate_gradient_matches_central_difference(labels):
    """autograd w.r.t. the per-utterance gate against a central difference in fp64, entry by entry: within 1e-6 of the entry's own
    size plus 1e-8 absolute.  h = 1e-5: the truncation error is O(h^2) = 1e-10 times the third derivative, the cancellation error
    about 2.2e-16 |L| / (2 h) = 1e-11 |L| with a loss |L| of order 1e2, so 1e-9 absolute - the floor is ten times that.  At a
    mask with values 0, 0.5 and 1; entries probed: a pruned head, the 0.5 head and kept heads of both layers, several utterances"""
    meta, _ = load_case("bert_L2")
    m, ocfg, cfg, _, batch = oracle_model(meta, labels)
    ids, seg, y = case_tensors(meta, batch)
    L, heads, B = ocfg.num_hidden_layers, ocfg.num_attention_heads, ids.shape[0]
    mask = mixed_mask(L, heads)
    gate = mask[:, None, :].expand(L, B, heads).clone()
    _, _, _, _, grad = oracle_gated(m, ocfg, labels, ids, seg, y, gate)
    assert grad.shape == (L, B, heads)
    zero_head, half_head = (1, 7)
    assert mask[0, zero_head] == 0.0 and mask[0, half_head] == 0.5
    h = 1e-5
    with torch.no_grad():
        for l, b, hd in ((0, 0, zero_head), (0, 2, half_head), (0, 1, 0), (1, 3, 4), (1, 0, 9), (1, 2, 11)):
            lo, hi = gate.clone(), gate.clone()
            lo[l, b, hd] -= h
            hi[l, b, hd] += h
            fd = (oracle_gated(m, ocfg, labels, ids, seg, y, hi, False)[3] - oracle_gated(m, ocfg, labels, ids, seg, y, lo, False)[3]) / (2 * h)
            err, ref = abs(fd.item() - grad[l, b, hd].item()), abs(grad[l, b, hd].item())
            print("gate (%d, %d, %d): autograd %.6e, central difference %.6e, |diff| %.2e" % (l, b, hd, grad[l, b, hd].item(), fd.item(), err))
            assert err <= 1e-6 * ref + 1e-8, (l, b, hd, fd.item(), grad[l, b, hd].item())
    assert grad[0, :, zero_head].abs().max().item() > 0.0, "the gradient of a pruned head is generally non-zero"
    # a per-utterance gate only moves its own utterance's loss: the [L, heads] form gives the same per-utterance gradients
    g2 = oracle_gated(m, ocfg, labels, ids, seg, y, mask)[4]
    assert torch.allclose(g2, grad, rtol=1e-12, atol=1e-14)

# ---- exports, descriptor --------------------------------------------------------------------------------------------------------
def test_head_gate_symbols_exported():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    lib = C.CDLL(hb.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nbest_hip.h")).read()
    for name in ("nbest_head_gate_fwd", "nbest_head_gate_bwd"):
        assert name in hb.EXPORTS and hasattr(lib, name) and name in hdr
    assert "head_gate_grad" in hdr
    assert callable(hb.head_gate_fwd) and callable(hb.head_gate_bwd)

def test_encoder_desc_has_head_gate_fields():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    fields = [f for f, _ in hb.EncoderDesc._fields_]
    i = fields.index("head_gate")
    # the two pointers follow wgrad_skip_host, as in include/nbest_hip.h (the attribution fields stay the descriptor's last four)
    assert fields[i - 1:i + 3] == ["wgrad_skip_host", "head_gate", "head_gate_grad", "base_ids"]
    assert C.sizeof(hb.EncoderDesc) % 8 == 0
    assert hb.EncoderDesc.head_gate.offset % 8 == 0 and hb.EncoderDesc.head_gate_grad.offset == hb.EncoderDesc.head_gate.offset + 8
    assert hb.EncoderDesc.base_ids.offset == hb.EncoderDesc.head_gate_grad.offset + 8
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nbest_hip.h")).read()
    assert hdr.index("wgrad_skip_host;") < hdr.index("const float* head_gate;") < hdr.index("float* head_gate_grad;") < hdr.index("const int64_t* base_ids;")
    d = hb.EncoderDesc()
    assert d.head_gate is None and d.head_gate_grad is None          # zero = no gate
    d.wgrad_group = 2
    assert d.wgrad_group == 2 and d.head_gate is None

# ---- --head_mask files ------------------------------------------------------------------------------------------------------------
def test_read_head_mask(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer
    p = tmp_path / "m.json"
    good = [[1, 0, 0.5], [1.0, 1, 0]]
    p.write_text(json.dumps(good))
    got = trainer.read_head_mask(str(p), 2, 3)
    assert got == [[1.0, 0.0, 0.5], [1.0, 1.0, 0.0]] and all(isinstance(x, float) for r in got for x in r)
    for bad, L, heads, word in ((good, 3, 3, "shape"), (good, 2, 4, "shape"), ([[1, 0, 0.5], [1, 1]], 2, 3, "shape"),
                                ([1, 0, 1], 1, 3, "rows"), ({"mask": good}, 2, 3, "rows"), ([[1, "x", 0], [1, 1, 1]], 2, 3, "number"),
                                ([[1, True, 0], [1, 1, 1]], 2, 3, "number")):
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError, match=word):
            trainer.read_head_mask(str(p), L, heads)
    p.write_text("[[1, 0, NaN], [1, 1, 1]]")
    with pytest.raises(ValueError, match="finite"):
        trainer.read_head_mask(str(p), 2, 3)
    p.write_text("not json")
    with pytest.raises(ValueError):
        trainer.read_head_mask(str(p), 2, 3)
    with pytest.raises(ValueError):
        trainer.read_head_mask(str(tmp_path / "missing.json"), 2, 3)

# ---- prune_lowest -------------------------------------------------------------------------------------------------------------------
def test_prune_lowest():
    import nbest_amd  # noqa: F401
    from nbest_amd.trainer import prune_lowest
    imp = [[0.5, 0.1, 0.3, 0.1], [0.2, 0.1, 0.9, 0.05]]
    ones = [[1.0] * 4 for _ in range(2)]
    assert prune_lowest(imp, None, 0) == ones
    assert prune_lowest(imp, None, 1) == [[1, 1, 1, 1], [1, 1, 1, 0]]
    # ties (0.1 three times) go by (layer, head) index
    assert prune_lowest(imp, None, 2) == [[1, 0, 1, 1], [1, 1, 1, 0]]
    assert prune_lowest(imp, None, 3) == [[1, 0, 1, 0], [1, 1, 1, 0]]
    assert prune_lowest(imp, None, 4) == [[1, 0, 1, 0], [1, 0, 1, 0]]
    # already-masked heads are skipped (and stay as they are; a 0.5 gate counts as kept)
    mask = [[1.0, 0.0, 1.0, 1.0], [0.5, 1.0, 1.0, 0.0]]
    assert prune_lowest(imp, mask, 2) == [[1, 0, 1, 0], [0.5, 0, 1, 0]]
    assert mask == [[1.0, 0.0, 1.0, 1.0], [0.5, 1.0, 1.0, 0.0]] and imp[0][1] == 0.1, "prune_lowest must not modify its arguments"
    # at least one head per layer: layer 0 holds the five lowest scores, its last kept head is passed over
    imp2 = [[0.01, 0.02, 0.03, 0.04], [0.5, 0.6, 0.7, 0.8]]
    assert prune_lowest(imp2, None, 4) == [[0, 0, 0, 1], [0, 1, 1, 1]]
    assert prune_lowest(imp2, None, 6) == [[0, 0, 0, 1], [0, 0, 0, 1]]
    with pytest.raises(ValueError, match="one head kept per layer"):
        prune_lowest(imp2, None, 7)
    with pytest.raises(ValueError):
        prune_lowest(imp2, [[1.0] * 3] * 2, 1)
    assert prune_lowest(torch.tensor(imp), torch.tensor(ones), 2) == [[1, 0, 1, 1], [1, 1, 1, 0]]

# ---- importance aggregation ---------------------------------------------------------------------------------------------------------
def test_head_importance_table():
    import nbest_amd  # noqa: F401
    from nbest_amd.trainer import head_importance_table
    g1 = torch.tensor([[[1.0, -2.0], [3.0, 0.0]],                   # [L = 2, B = 2, heads = 2]
                       [[0.0, 0.0], [0.0, 0.0]]])
    g2 = torch.tensor([[[-2.0, 4.0]],                                # a second batch of one utterance
                       [[0.0, -6.0]]])
    t = head_importance_table(iter([g1, g2]))
    assert t["utterances"] == 3
    assert t["importance"] == [[2.0, 2.0], [0.0, 2.0]]
    r = 2.0 / (8.0 ** 0.5)
    assert t["normalized"][0] == pytest.approx([r, r], abs=1e-15) and t["normalized"][1] == [0.0, 1.0]
    z = head_importance_table([torch.zeros(1, 2, 3)])
    assert z["importance"] == [[0.0, 0.0, 0.0]] and z["normalized"] == [[0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        head_importance_table([])

# ---- CLI flag errors ------------------------------------------------------------------------------------------------------------------
def test_head_mask_cli_flags(tmp_path, monkeypatch):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    src = tmp_path / "in.txt"
    src.write_text(open(os.path.join(GOLDEN, "valid_head.txt")).read())
    mask = tmp_path / "mask.json"
    mask.write_text(json.dumps([[1.0] * 12] * 2))
    out = str(tmp_path / "imp.json")
    base = ["--dataset", "dstc2", "--dataroot", str(tmp_path), "--deviceId", "0"]
    for bad in (["--prune_heads", "3"],                                              # without --head_importance
                ["--head_mask", str(mask)],                                          # a training run
                ["--testing", "--head_mask", str(tmp_path / "missing.json")],
                ["--head_importance", out, "--prune_heads", "-1"],
                ["--head_importance", out, "--testing"],
                ["--head_importance", out, "--predict", str(src)]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + bad)
    opt = cli.parse_arguments(base + ["--head_importance", out, "--prune_heads", "3", "--head_mask", str(mask)])
    assert opt.head_importance == out and opt.prune_heads == 3 and opt.head_mask == str(mask)
    for ok in (["--testing"], ["--predict", str(src)]):
        assert cli.parse_arguments(base + ok + ["--head_mask", str(mask)]).head_mask == str(mask)
    opt = cli.parse_arguments(base)
    assert opt.head_mask is None and opt.head_importance is None and opt.prune_heads is None
    monkeypatch.setenv("WORLD_SIZE", "2")                                            # torchrun: refused, as --predict
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--head_importance", out])

def test_set_head_mask_shape_and_device_free_checks():
    """set_head_mask's shape check runs before anything touches the device"""
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    m = NBestSTCModel.__new__(NBestSTCModel)

    class _Cfg:
        num_hidden_layers, num_attention_heads = 2, 12
    m.__dict__.update(cfg=_Cfg(), _head_mask="sentinel")
    with pytest.raises(ValueError, match=r"\[L=2, heads=12\]"):
        NBestSTCModel.set_head_mask(m, torch.ones(12, 2))
    with pytest.raises(ValueError):
        NBestSTCModel.set_head_mask(m, [1.0] * 24)
    assert m.__dict__["_head_mask"] == "sentinel"
    NBestSTCModel.set_head_mask(m, None)
    assert m.head_mask is None
