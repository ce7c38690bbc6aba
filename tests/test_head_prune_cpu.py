"""CPU: compact pruned heads - the torch restatement (nbest_amd/prune.py) against the fp64 oracle under the same mask, the exports,
the host plan and the --compact_heads flag errors."""
import ctypes as C
import json
import math
import os

import pytest
import torch

from conftest import GOLDEN, load_case
from test_attrib_cpu import oracle_model
from test_head_gate_cpu import case_tensors, mixed_mask, oracle_gated


def prune_masks(L, heads):
    """the masks of these tests: mixed_mask (zeros, a 0.5, ones), all ones, one head kept per layer, one layer all zeros"""
    one = torch.zeros(L, heads, dtype=torch.float64)
    for l in range(L):
        one[l, (5 * l + 3) % heads] = 1.0
    dead = torch.ones(L, heads, dtype=torch.float64)
    dead[L - 1] = 0.0
    dead[0, 2] = 0.0
    return {"mixed": mixed_mask(L, heads), "ones": torch.ones(L, heads, dtype=torch.float64), "one_head": one, "dead_layer": dead}


def compact_oracle_final(om, ocfg, ids, seg, layers, rw=lambda t: t, ract=lambda t: t, ln=lambda x, mod: mod(x), attn=None, gelu=None):
    """The oracle's forward with every attention block rebuilt from ``layers`` = compact_layer_tensors(...): k-head attention on
    Wqkv' / bqkv', then Wo' (bias and residual as always); embeddings, LayerNorms, FFN and the STC heads are the oracle's own modules.
    Returns final.  The hooks (identity by default) are the rounding points of a bf16-storage leg: ``rw`` on weight matrices, ``ract``
    on stored activations, ``ln`` / ``attn`` / ``gelu`` the leg's LayerNorm, attention core and GELU."""
    import torch.nn.functional as F
    from oracle.encoder import position_ids_for
    enc = om.bert_encoder
    E = enc.embeddings
    B, S = ids.shape
    d = 64
    km = ids > 0
    s0 = torch.zeros_like(ids) if (seg is None or ocfg.family == "xlm-roberta") else seg
    pos = position_ids_for(ocfg, ids)
    e = rw(E.word_embeddings.weight[ids]) + F.embedding(s0, rw(E.token_type_embeddings.weight)) + F.embedding(pos, rw(E.position_embeddings.weight))
    x = ract(ln(e, E.LayerNorm))
    for lyr, (idx, wqkv, bqkv, wo) in zip(enc.encoder.layer, layers):
        k = len(idx)
        ao = lyr.attention.output
        qkv = ract(F.linear(x, rw(wqkv), bqkv))                              # [B, S, 3 64k]
        q, kk, v = (t.view(B, S, k, d).transpose(1, 2) for t in qkv.split(k * d, dim=-1))
        if attn is None:
            sc = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(d)
            sc = sc.masked_fill(~km[:, None, None, :], float("-inf"))
            ctx = torch.matmul(torch.softmax(sc, dim=-1), v)
        else:
            ctx = attn(q, kk, v, km, 1.0 / math.sqrt(d))
        ctx = ract(ctx.transpose(1, 2).reshape(B, S, k * d))
        r1 = ract(F.linear(ctx, wo, ao.dense.bias) + x)                      # (wo: rounded by the caller - its rounding point is its own)
        x1 = ract(ln(r1, ao.LayerNorm))
        u = F.linear(x1, rw(lyr.intermediate.dense.weight), lyr.intermediate.dense.bias)
        hact = 0.5 * u * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0)))) if gelu is None else gelu(u)
        r2 = ract(F.linear(hact, rw(lyr.output.dense.weight), lyr.output.dense.bias) + x1)
        x = ract(ln(r2, lyr.output.LayerNorm))
    return om.clf(x[:, 0, :])[2].detach()


@pytest.mark.parametrize("which", ["mixed", "ones", "one_head", "dead_layer"])
def test_restatement_matches_gated_oracle(which, labels):
    """fp64 both ways; the only difference is where the gate multiplies (the context, or the columns of Wo): 1e-10 on the final scores"""
    import nbest_amd  # noqa: F401
    from nbest_amd.prune import compact_layer_tensors, kept_heads
    meta, _ = load_case("bert_L2")
    om, ocfg, cfg, _, batch = oracle_model(meta, labels)
    ids, seg, y = case_tensors(meta, batch)
    L, heads = ocfg.num_hidden_layers, ocfg.num_attention_heads
    mask = prune_masks(L, heads)[which]
    fin_ref = oracle_gated(om, ocfg, labels, ids, seg, y, mask, want_grad=False)[2]
    sd = {k: v.detach() for k, v in om.state_dict().items()}
    layers = compact_layer_tensors(sd, mask)
    kept = kept_heads(mask)
    for l, (idx, wqkv, bqkv, wo) in enumerate(layers):
        want = [h for h in range(heads) if mask[l, h] != 0] or [0]
        assert idx == want == kept[l]
        k = len(idx)
        assert wqkv.shape == (3 * 64 * k, ocfg.hidden_size) and bqkv.shape == (3 * 64 * k,) and wo.shape == (ocfg.hidden_size, 64 * k)
        assert wqkv.dtype == torch.float64
        wq = sd["bert_encoder.encoder.layer.%d.attention.self.query.weight" % l]
        assert torch.equal(wqkv[64 * (k - 1):64 * k], wq[64 * idx[-1]:64 * idx[-1] + 64])
        if which == "ones":
            assert torch.equal(wo, sd["bert_encoder.encoder.layer.%d.attention.output.dense.weight" % l])
    if which == "dead_layer":
        assert layers[-1][0] == [0] and bool((layers[-1][3] == 0).all()), "a layer without a kept head: Wo' is zeros through the gate"
    fin = compact_oracle_final(om, ocfg, ids, seg, layers)
    err = (fin - fin_ref).abs().max().item()
    print("compact restatement vs gated oracle, %s mask: |final - ref| %.3e" % (which, err))
    assert err <= 1e-10, err
    if which != "ones":
        plain = om(ids, None, seg_ids=seg)[2].detach()
        assert (plain - fin_ref).abs().max().item() > 1e-3, "the mask changed nothing"


def test_kept_heads_even_rule():
    from nbest_amd.prune import kept_heads
    m = torch.tensor([[1.0, 0.0, 0.5, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, -1.3, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    assert kept_heads(m) == [[0, 2], [0], [0, 1], [0, 1, 2, 3]]
    # an odd count carries the lowest-numbered pruned head (gate 0: zero columns in Wo')
    assert kept_heads(m[:3, :3], even=True) == [[0, 2], [0, 1], [0, 1]]
    assert kept_heads(torch.tensor([[0.0, 0.0, 1.0, 0.0]]), even=True) == [[0, 2]]
    assert kept_heads(torch.tensor([[0.0, 0.0, 0.0, 0.0]]), even=True) == [[0, 1]]
    with pytest.raises(ValueError):
        kept_heads(torch.tensor([[1.0, 1.0, 1.0]]), even=True)


def test_head_prune_symbols_exported():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    lib = C.CDLL(hb.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nbest_hip.h")).read()
    for name in ("nbest_head_prune_plan", "nbest_head_prune_pack", "nbest_encoder_infer_pruned"):
        assert name in hb.EXPORTS and hasattr(lib, name) and name in hdr, name
    assert C.sizeof(hb.HeadPruneLayer) == 6 * 8 + 2 * 4 + 4 * hb.HEAD_PRUNE_MAX_HEADS
    assert "NBEST_HEAD_PRUNE_MAX_HEADS %d" % hb.HEAD_PRUNE_MAX_HEADS in hdr
    for f in ("head_prune_plan", "head_prune_pack", "encoder_infer_pruned"):
        assert callable(getattr(hb, f))
    # the descriptor did not move
    assert [f for f, _ in hb.EncoderDesc._fields_][-4:] == ["base_ids", "alpha", "no_param_grad", "pad5"]


@pytest.mark.parametrize("heads", [12, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_head_prune_plan_layout(heads, dtype):
    """the host plan: tensors back to back, Wqkv' of all layers then Wo' of all layers, sizes as stated, for every k"""
    from nbest_amd import hipabi as hb
    H, esz = heads * 64, 2 if dtype == torch.bfloat16 else 4
    kept = [list(range(k)) for k in range(1, heads + 1)]
    tab, (qb, ob, bb) = hb.head_prune_plan(kept, heads, dtype)
    q = o = b = 0
    for k, t in zip(range(1, heads + 1), tab):
        assert t.k == k and list(t.idx)[:k] == list(range(k))
        assert (t.dst_wqkv, t.dst_bqkv) == (q, b) and t.dst_wo == qb // esz + o
        q += 3 * 64 * k * H
        b += 3 * 64 * k
        o += H * 64 * k
    assert (qb, ob, bb) == (q * esz, o * esz, b * 4)
    for bad in ([[]], [list(range(heads + 1))]):
        with pytest.raises(RuntimeError, match="head_prune_plan"):
            hb.head_prune_plan(bad, heads, dtype)


def test_compact_heads_cli_flags(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    src = tmp_path / "in.txt"
    src.write_text(open(os.path.join(GOLDEN, "valid_head.txt")).read())
    mask = tmp_path / "mask.json"
    mask.write_text(json.dumps([[1.0] * 12] * 2))
    base = ["--dataset", "dstc2", "--dataroot", str(tmp_path), "--deviceId", "0"]
    pm = ["--predict", str(src), "--head_mask", str(mask)]
    opt = cli.parse_arguments(base + pm + ["--compact_heads"])
    assert opt.compact_heads and opt.head_mask == str(mask)
    assert cli.exp_dir(opt) == cli.exp_dir(cli.parse_arguments(base + pm)), "exp_dir must not depend on --compact_heads"
    assert not cli.parse_arguments(base + pm).compact_heads
    for bad in (["--compact_heads"],                                                           # a training run
                ["--predict", str(src), "--compact_heads"],                                    # without --head_mask
                ["--testing", "--head_mask", str(mask), "--compact_heads"],
                ["--head_importance", str(tmp_path / "imp.json"), "--head_mask", str(mask), "--compact_heads"],
                pm + ["--compact_heads", "--predict_attention", str(tmp_path / "a.jsonl")],
                pm + ["--compact_heads", "--predict_attribution", str(tmp_path / "b.jsonl")]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + bad)


def test_set_head_mask_compact_refusals_need_no_device(labels):
    """compact=True without a mask or with trainable=True: ValueError before anything touches the device"""
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel

    class Dummy:
        cfg = type("c", (), {"num_hidden_layers": 2, "num_attention_heads": 12})()
        _head_mask = None
    with pytest.raises(ValueError, match="compact"):
        NBestSTCModel.set_head_mask(Dummy(), None, compact=True)
    with pytest.raises(ValueError, match="compact"):
        NBestSTCModel.set_head_mask(Dummy(), torch.ones(2, 12), trainable=True, compact=True)
