"""Compact pruned heads, restated in torch: which heads a mask keeps and the per-layer tensors of the compact encoder
(nbest_head_prune_pack builds the same images on the device; include/nbest_hip.h).

A layer that keeps the heads ``idx`` (k of them, ascending; a head is kept when its gate != 0) is an ordinary layer with
``Wqkv' [3 64k, H]`` (row ``(t k + i) 64 + r`` = row ``(t heads + idx[i]) 64 + r`` of the fused Q|K|V matrix), ``bqkv' [3 64k]``
(the same rows of the fused bias) and ``Wo' [H, 64k]`` (column ``i 64 + r`` = ``gate[idx[i]]`` x column ``idx[i] 64 + r``: the gate
is folded into the output matrix, so any float mask works).  A layer with no kept head is ``idx = [0]``: its gate is 0, so its
``Wo'`` is all zeros and the layer's attention block reduces to the bias and the residual, as under the gate.
"""
import torch

HEAD_DIM = 64


def kept_heads(mask, even=False):
    """per layer, the ascending indices of the heads ``mask`` [L, heads] keeps (gate != 0); ``[0]`` for a layer that keeps none.
    ``even``: a layer with an odd count also carries its lowest-numbered pruned head (gate 0: its Wo' columns are zeros, the result
    is unchanged) - the bf16 GEMM tiles need 64 k to be a multiple of 128."""
    m = torch.as_tensor(mask).detach().to("cpu", torch.float32)
    out = []
    for row in m:
        idx = [h for h, g in enumerate(row.tolist()) if g != 0.0]
        if not idx:
            idx = [0]
        if even and len(idx) % 2:
            spare = [h for h, g in enumerate(row.tolist()) if g == 0.0 and h not in idx]
            if not spare:
                raise ValueError("nbest_amd prune: a layer keeps an odd number of heads (%d) and has no pruned head to pair it with"
                                 % len(idx))
            idx = sorted(idx + spare[:1])
        out.append(idx)
    return out


def compact_layer_tensors(state_dict, mask, kept=None):
    """``state_dict``: reference-keyed (``bert_encoder.encoder.layer.N.attention...``), tensors or arrays of any float dtype, on
    any device; ``mask`` [L, heads].  Returns one ``(idx, Wqkv', bqkv', Wo')`` per layer by the rule above, in the dtypes of the
    inputs: the rows are copies, ``Wo' = T(gate * float(Wo))`` with the product formed in fp32 (fp64 for fp64 weights).
    ``kept``: the index lists to use instead of ``kept_heads(mask)``."""
    m = torch.as_tensor(mask).detach()
    idxs = kept_heads(m) if kept is None else kept
    out = []
    for l, idx in enumerate(idxs):
        pre = "bert_encoder.encoder.layer.%d.attention." % l
        get = lambda n: torch.as_tensor(state_dict[pre + n])
        rows = torch.tensor([h * HEAD_DIM + r for h in idx for r in range(HEAD_DIM)], dtype=torch.long)
        ws = [get("self.%s.weight" % n) for n in ("query", "key", "value")]
        bs = [get("self.%s.bias" % n) for n in ("query", "key", "value")]
        wo = get("output.dense.weight")
        r = rows.to(wo.device)
        wqkv = torch.cat([w[r.to(w.device)] for w in ws], 0).contiguous()
        bqkv = torch.cat([b[r.to(b.device)] for b in bs], 0).contiguous()
        acc = torch.float64 if wo.dtype == torch.float64 else torch.float32
        g = m[l].to(device=wo.device, dtype=acc)[torch.tensor(idx, device=wo.device)].repeat_interleave(HEAD_DIM)
        wo_c = (wo[:, r].to(acc) * g[None, :]).to(wo.dtype).contiguous()
        out.append((idx, wqkv, bqkv, wo_c))
    return out
