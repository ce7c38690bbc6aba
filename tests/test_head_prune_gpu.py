"""GPU: compact pruned heads - nbest_head_prune_pack against the torch restatement (nbest_amd/prune.py), compact predict
(nbest_encoder_infer_pruned) against the fp64 oracle under the same mask, against the gated predict and against the plain one, the edge
masks, the training state it must leave alone, the fp8w model, the refusals and --compact_heads end to end."""
import json
import os
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_attrib_cpu import oracle_model
from test_head_gate_cpu import case_tensors, mixed_mask, oracle_gated
from test_head_gate_gpu import _hip_model, _scaled_ok
from test_head_prune_cpu import compact_oracle_final, prune_masks
from test_infer_gpu import _batch, _model, _same_state, _state
from test_model_gpu import _cmp, _log

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256     # elements on either side of an image


def _masks(L, heads):
    m = dict(prune_masks(L, heads))
    f = torch.ones(L, heads, dtype=torch.float64)          # float gates: 0.5 and -1.3 next to a 0 and ones
    for l in range(L):
        f[l, (l + 1) % heads], f[l, (l + 4) % heads], f[l, (l + 6) % heads] = 0.5, -1.3, 0.0
    m["floats"] = f
    return m


# ---- 1. the pack kernel against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mixed", "ones", "one_head", "dead_layer", "floats"])
@pytest.mark.parametrize("heads", [12, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_kernel_matches_restatement(dtype, heads, which):
    """a two-layer arena of random matrices at offsets of its own: Wqkv' and bqkv' bit-equal to the restatement's gather, Wo' columns with
    gate 1 bit-equal, the others by the rule of test_head_gate_gpu._scaled_ok; two runs bit-identical; the guard bands around the
    images untouched and every byte inside them written"""
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    from nbest_amd.prune import compact_layer_tensors, kept_heads
    L, H = 2, heads * 64
    mask = _masks(L, heads)[which]
    g = torch.Generator(device="cpu").manual_seed(heads + len(which))
    # arena: [pad 64 | Wqkv0 | Wo0 | pad 128 | Wqkv1 | Wo1 | pad 128]; the biases in an fp32 arena with gaps of its own
    offs, o, sd = [], 64, {}
    for l in range(L):
        offs.append(dict(wqkv=o, wo=o + 3 * H * H, bqkv=64 + (3 * H + 64) * l))
        o += 4 * H * H + 128
    wts = (torch.randn(o, generator=g) * 0.05).to(dtype).to(DEV)
    prm = torch.randn(64 + (3 * H + 64) * L, generator=g).to(DEV)
    for l, f in enumerate(offs):
        pre = "bert_encoder.encoder.layer.%d.attention." % l
        for j, n in enumerate(("query", "key", "value")):
            sd[pre + "self.%s.weight" % n] = wts[f["wqkv"] + j * H * H:f["wqkv"] + (j + 1) * H * H].view(H, H)
            sd[pre + "self.%s.bias" % n] = prm[f["bqkv"] + j * H:f["bqkv"] + (j + 1) * H]
        sd[pre + "output.dense.weight"] = wts[f["wo"]:f["wo"] + H * H].view(H, H)
    kept = kept_heads(mask)
    ref = compact_layer_tensors(sd, mask)
    tab, (qb, ob, bb) = hb.head_prune_plan(kept, heads, dtype)
    for l, f in enumerate(offs):
        tab[l].src_wqkv, tab[l].src_bqkv, tab[l].src_wo = f["wqkv"], f["bqkv"], f["wo"]
    esz = wts.element_size()
    gate = mask.float().to(DEV)
    runs = []
    for sentinel in (7.0, -3.0):
        wbuf = torch.full(((qb + ob) // esz + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
        bbuf = torch.full((bb // 4 + 2 * GUARD,), sentinel, dtype=torch.float32, device=DEV)
        hb.head_prune_pack(wts, prm, gate, tab, heads, wbuf[GUARD:-GUARD], bbuf[GUARD:-GUARD])
        torch.cuda.synchronize()
        for buf in (wbuf, bbuf):
            assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all()), "a guard band was written"
        runs.append((wbuf[GUARD:-GUARD].clone(), bbuf[GUARD:-GUARD].clone()))
    # (two runs over different sentinels: bit-identical only if every byte of the images is written, and written the same)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ / bytes left unwritten"
    w, b = runs[0]
    for l, (idx, wqkv, bqkv, wo) in enumerate(ref):
        k, t = len(idx), tab[l]
        assert torch.equal(w[t.dst_wqkv:t.dst_wqkv + 3 * 64 * k * H].view(3 * 64 * k, H), wqkv), "Wqkv' layer %d" % l
        assert torch.equal(b[t.dst_bqkv:t.dst_bqkv + 3 * 64 * k], bqkv), "bqkv' layer %d" % l
        got = w[t.dst_wo:t.dst_wo + H * 64 * k].view(H, k, 64)
        src = sd["bert_encoder.encoder.layer.%d.attention.output.dense.weight" % l].view(H, heads, 64)
        for i, h in enumerate(idx):
            gv = float(gate[l, h])                           # the fp32 gate the kernel multiplies by
            if gv == 1.0:
                assert torch.equal(got[:, i], src[:, h]), "Wo' layer %d head %d: a gate of 1 must copy the bits" % (l, h)
            else:
                assert _scaled_ok(got[:, i], src[:, h].double() * gv, dtype), "Wo' layer %d head %d (gate %g)" % (l, h, gv)
            if gv == 0.0:
                assert bool((got[:, i] == 0).all())
        if dtype == torch.float32:
            assert torch.equal(got.reshape(H, 64 * k), wo), "fp32 Wo' must equal the restatement bit for bit"


def test_pack_refuses_a_table_outside_its_buffers():
    """the host checks of nbest_head_prune_pack: nothing is launched for a table whose images do not fit, or whose indices do not ascend"""
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    heads, H = 12, 768
    wts = torch.zeros(64 + 4 * H * H, device=DEV)
    prm = torch.zeros(64 + 3 * H, device=DEV)
    gate = torch.ones(1, heads, device=DEV)
    tab, (qb, ob, bb) = hb.head_prune_plan([[0, 3, 5]], heads, torch.float32)
    tab[0].src_wqkv, tab[0].src_bqkv, tab[0].src_wo = 64, 64, 64 + 3 * H * H
    w = torch.full(((qb + ob) // 4,), 7.0, device=DEV)
    b = torch.full((bb // 4,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="head_prune_pack"):
        hb.head_prune_pack(wts, prm, gate, tab, heads, w[:-4], b)
    with pytest.raises(RuntimeError, match="head_prune_pack"):
        hb.head_prune_pack(wts, prm, gate, tab, heads, w, b[:-4])
    tab[0].idx[1] = 7                                                     # 0, 7, 5: not ascending
    with pytest.raises(RuntimeError, match="ascend"):
        hb.head_prune_pack(wts, prm, gate, tab, heads, w, b)
    torch.cuda.synchronize()
    assert bool((w == 7.0).all()) and bool((b == 7.0).all()), "a refused call wrote something"


# ---- 2. compact predict against the fp64 oracle -------------------------------------------------------------------------------------------
def _compact_final(m, meta, batch, mask):
    ids, seg, _ = (None if t is None else t.to(DEV) for t in case_tensors(meta, batch))
    m.set_head_mask(mask, compact=True)
    assert m.head_mask_compact
    fin = m.predict(ids, seg_ids=seg)["final"].double().cpu()
    torch.cuda.synchronize()
    return fin


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2"])
def test_compact_predict_matches_oracle_fp32(name, labels):
    """fp32 under mixed_mask: final within 1e-4 absolute of the gated fp64 oracle (the bar of
    test_masked_scores_and_gate_grad_match_oracle_fp32); the un-masked scores are off by more than 1e-3"""
    meta, _ = load_case(name)
    om, ocfg, cfg, _, batch = oracle_model(meta, labels)
    m, _, _ = _hip_model(meta, labels, torch.float32)
    ids, seg, y = case_tensors(meta, batch)
    mask = mixed_mask(ocfg.num_hidden_layers, ocfg.num_attention_heads)
    fin_ref = oracle_gated(om, ocfg, labels, ids, seg, y, mask, want_grad=False)[2]
    fin = _compact_final(m, meta, batch, mask)
    err = (fin - fin_ref).abs().max().item()
    print("fp32 compact predict %s: |final - ref| %.3e" % (name, err))
    assert err <= 1e-4, "%s: |final - ref| = %.3e > 1e-4" % (name, err)
    m.set_head_mask(None)
    assert not m.head_mask_compact
    plain = m.predict(*(None if t is None else t.to(DEV) for t in (ids, seg)))["final"].double().cpu()
    assert (plain - fin_ref).abs().max().item() > 1e-3


def _bf16_leg_compact(om32, ocfg, ids, seg, mask, kept):
    """the bf16-storage leg of THIS path (oracle/bf16sim.py's rounding points): the context of the kept heads only - no gated copy is
    ever stored - and the gate inside the output matrix, whose columns are bf16(gate * bf16(Wo)).  Returns final in fp64."""
    from oracle import bf16sim as bs
    from nbest_amd.prune import compact_layer_tensors
    with torch.no_grad():
        sd = {k: v.detach() for k, v in om32.state_dict().items()}
        for l in range(ocfg.num_hidden_layers):
            key = "bert_encoder.encoder.layer.%d.attention.output.dense.weight" % l
            sd[key] = bs._r(sd[key])
        layers = [(idx, wqkv, bqkv, bs._r(wo)) for idx, wqkv, bqkv, wo in compact_layer_tensors(sd, mask.float(), kept=kept)]
        fin = compact_oracle_final(om32, ocfg, ids, seg, layers, rw=bs.rw, ract=bs.ract, ln=bs._ln,
                                   attn=lambda q, k, v, km, s: bs._AttnCore.apply(q, k, v, km, s), gelu=lambda u: bs._GeluStore.apply(u, True))
    return fin.double()


@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2"])
def test_compact_predict_matches_oracle_bf16(name, labels):
    """bf16 against the gated fp64 oracle: the bar is 2 x the floor of the bf16-storage leg of the compact path, the maximum over
    five draws (the weights as they are and four copies jittered by 2^-12 relative), drawn exactly as
    test_masked_scores_and_gate_grad_match_oracle_bf16 draws them.  HIP / floor ratios seen on an MI355X: DESIGN.md section 4
    (compact pruned heads)."""
    from nbest_amd.prune import kept_heads
    meta, _ = load_case(name)
    om64, ocfg, cfg, _, batch = oracle_model(meta, labels)
    om32 = oracle_model(meta, labels, dtype=torch.float32)[0]
    m, _, _ = _hip_model(meta, labels, torch.bfloat16)
    ids, seg, y = case_tensors(meta, batch)
    mask = mixed_mask(ocfg.num_hidden_layers, ocfg.num_attention_heads)
    kept = kept_heads(mask, even=True)                      # what the bf16 model runs
    fin_ref = oracle_gated(om64, ocfg, labels, ids, seg, y, mask, want_grad=False)[2]
    fin_floor = 0.0
    word = om32.bert_encoder.embeddings.word_embeddings.weight
    rows = torch.unique(ids)
    params = list(om32.parameters())
    saved = [(p[rows] if p is word else p).detach().clone() for p in params]
    for draw in range(5):
        if draw:
            gj = torch.Generator().manual_seed(1000003 * meta["seed"] + draw)
            with torch.no_grad():
                for p, q in zip(params, saved):
                    jit = q * (1.0 + 2.0 ** -12 * (2.0 * torch.rand(q.shape, generator=gj) - 1.0))
                    if p is word:
                        p[rows] = jit
                    else:
                        p.copy_(jit)
        fin_floor = max(fin_floor, (_bf16_leg_compact(om32, ocfg, ids, seg, mask, kept) - fin_ref).abs().max().item())
    fin = _compact_final(m, meta, batch, mask)
    assert m._prune.kept == kept
    err = (fin - fin_ref).abs().max().item()
    msg = "bf16 compact heads %s: HIP / floor: final (compact predict) %.2f; floor %.2e" % (name, err / fin_floor, fin_floor)
    print(msg)
    _log(msg)
    assert err <= 2.0 * fin_floor, "%s compact predict: |final - ref| %.3e > 2 x floor %.3e" % (name, err, fin_floor)


# ---- 3. compact against gated and plain predict ------------------------------------------------------------------------------------------
def _agree(tag, got, ref, f32):
    """the tolerances of test_masked_predict_agrees_with_masked_eval_forward"""
    _cmp(tag + "cls", got["cls"], ref["cls"].float().cpu(), rtol=1e-5 if f32 else 2.0 ** -7)
    _cmp(tag + "final", got["final"], ref["final"].cpu(), atol=1e-6 if f32 else 2e-3)


@pytest.mark.parametrize("B,S", [(3, 40), (4, 48), (2, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compact_predict_agrees_with_gated_predict(B, S, dtype, labels):
    m, cfg, _ = _model(labels, "bert", dtype=dtype)
    if S == 1:      # (the synthetic n-best rows need 8 tokens: S = 1 is their first column, the [CLS] token alone)
        b = {k: v[:, :1].contiguous() for k, v in _batch(cfg, labels, B, 8).items() if k in ("ids", "seg")}
    else:
        b = _batch(cfg, labels, B, S)
    m.eval()
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    m.set_head_mask(mask)
    gated = m.predict(b["ids"], seg_ids=b["seg"])
    m.set_head_mask(mask, compact=True)
    comp = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    _agree("compact vs gated B=%d S=%d %s " % (B, S, "f32" if f32 else "bf16"), comp, gated, f32)
    if f32:
        assert torch.equal(comp["pred"], gated["pred"])
    m.set_head_mask(None)
    plain = m.predict(b["ids"], seg_ids=b["seg"])
    assert not torch.equal(plain["cls"], comp["cls"]), "the mask changed nothing"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_ones_compact_mask_agrees_with_plain_predict(dtype, labels):
    m, cfg, _ = _model(labels, "bert", dtype=dtype)
    b = _batch(cfg, labels, 4, 48)
    m.eval()
    plain = m.predict(b["ids"], seg_ids=b["seg"])
    m.set_head_mask(torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads), compact=True)
    comp = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    same = torch.equal(comp["cls"], plain["cls"]) and torch.equal(comp["final"], plain["final"])
    msg = "all-ones compact mask vs plain predict %s: bits of cls and final %s" % ("f32" if f32 else "bf16", "IDENTICAL" if same else "differ")
    print(msg)
    _log(msg)
    _agree("all-ones compact vs plain %s " % ("f32" if f32 else "bf16"), comp, plain, f32)
    if f32:
        assert torch.equal(comp["pred"], plain["pred"])


@pytest.mark.parametrize("which", ["one_head", "dead_layer", "uneven"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compact_predict_edge_masks(which, dtype, labels):
    """one head kept per layer; one layer without a kept head (packed as k = 1 with zero Wo'); different k in the two layers (9 and 4
    kept: an odd count, which bf16 pairs with a pruned head) - each against the gated path"""
    m, cfg, _ = _model(labels, "bert", dtype=dtype)
    L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
    if which == "uneven":
        mask = torch.ones(L, heads)
        mask[0, [1, 5, 10]] = 0.0
        mask[1, [0, 1, 2, 4, 6, 7, 9, 11]] = 0.0
    else:
        mask = prune_masks(L, heads)[which]
    b = _batch(cfg, labels, 3, 40)
    m.eval()
    m.set_head_mask(mask)
    gated = m.predict(b["ids"], seg_ids=b["seg"])
    m.set_head_mask(mask, compact=True)
    ks = [len(ix) for ix in m._prune.kept]
    f32 = dtype == torch.float32
    if which == "one_head":
        assert ks == ([1, 1] if f32 else [2, 2])
    elif which == "dead_layer":
        assert ks[-1] == (1 if f32 else 2)
    else:
        assert ks == ([9, 4] if f32 else [10, 4])
    comp = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    _agree("compact vs gated, %s mask %s " % (which, "f32" if f32 else "bf16"), comp, gated, f32)
    if f32:
        assert torch.equal(comp["pred"], gated["pred"])


# ---- 4. state -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_compact_predict_leaves_training_state_alone(mode, labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, dtype=torch.float32 if mode == "f32" else torch.bfloat16)
    m.train()
    b = _batch(cfg, labels, 4, 48)
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    for _ in range(2):
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        opt.step()
    torch.cuda.synchronize()
    before = _state(m)
    m.set_head_mask(mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads), compact=True)
    out = m.predict(b["ids"], seg_ids=b["seg"])
    m.set_head_mask(None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["final"]).all())
    _same_state(before, _state(m))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_after_compact_predict_is_unchanged(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_cp in (False, True):
        m, cfg, _ = _model(labels, dtype=dtype)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_cp:
            m.set_head_mask(mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads), compact=True)
            m.predict(b["ids"], seg_ids=b["seg"])
            m.set_head_mask(None)
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after a compact predict() differs"


def test_compact_rebuilds_its_images_from_the_current_weights(labels):
    """no cache: after the weights change, the next compact predict follows them (fp32 reads the master weights directly)"""
    m, cfg, sd = _model(labels, dtype=torch.float32)
    b = _batch(cfg, labels, 3, 40)
    m.eval()
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    m.set_head_mask(mask, compact=True)
    first = m.predict(b["ids"], seg_ids=b["seg"])["cls"].clone()
    sd2 = {k: v.copy() for k, v in sd.items()}
    sd2["bert_encoder.encoder.layer.0.attention.output.dense.weight"] *= 0.5
    m.load_reference_state(sd2)
    comp = m.predict(b["ids"], seg_ids=b["seg"])
    m.set_head_mask(mask)
    gated = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    assert not torch.equal(first, comp["cls"])
    _agree("compact vs gated after a weight change ", comp, gated, True)


def test_fp8w_model_compact_predict(labels):
    """an fp8w model's predict runs its bf16 copy: under a compact mask it equals the bf16 model's compact predict bit for bit"""
    m8, cfg, _ = _model(labels, dtype=torch.bfloat16, fp8=True)
    mb, _, _ = _model(labels, dtype=torch.bfloat16)
    b = _batch(cfg, labels, 4, 48)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    m8.eval()
    m8.set_head_mask(mask, compact=True)
    mb.set_head_mask(mask, compact=True)
    o8, ob = m8.predict(b["ids"], seg_ids=b["seg"]), mb.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    for k in ("cls", "final", "pred"):
        assert torch.equal(o8[k], ob[k]), k


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_compact_refusals(labels):
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, dtype=torch.bfloat16)
    m.eval()
    L, heads, H = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.hidden_size
    b = _batch(cfg, labels, 2, 16)
    mask = mixed_mask(L, heads)
    ref = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    before = _state(m)
    with pytest.raises(ValueError, match="compact"):
        m.set_head_mask(mask, trainable=True, compact=True)
    with pytest.raises(ValueError, match="compact"):
        m.set_head_mask(None, compact=True)
    assert m.head_mask is None and not m.head_mask_compact and not m.head_mask_trainable
    m.set_head_mask(mask, compact=True)
    with pytest.raises(ValueError, match="return_attns"):
        m.predict(b["ids"], seg_ids=b["seg"], return_attns=True)
    # the entry point with desc.head_gate set: NBEST_ERR_ARG, cls_out untouched
    comp = m.predict(b["ids"], seg_ids=b["seg"])
    d = m._desc(2, 16, "infer").desc
    ids, seg, pos, km = m._inputs(b["ids"], b["seg"])
    cls = torch.full((2, H), 7.0, dtype=torch.bfloat16, device=DEV)
    gate = torch.ones(L, heads, device=DEV)
    d.head_gate = gate.data_ptr()
    pr = m._prune
    with pytest.raises(RuntimeError, match="head_gate"):
        hb.encoder_infer_pruned(d, m.arena.weights, m.arena.p, ids, seg, pos, km, m._infer_ws, cls, pr.tab, pr.w, None, pr.b)
    d.head_gate = None
    # bf16 and an odd kept count: refused by the entry point (the model never builds such a table)
    tab, _ = hb.head_prune_plan([[0, 1, 2], [0, 1]], heads, torch.bfloat16, m.arena.layer_offsets)
    with pytest.raises(RuntimeError, match="even"):
        hb.encoder_infer_pruned(d, m.arena.weights, m.arena.p, ids, seg, pos, km, m._infer_ws, cls, tab, pr.w, None, pr.b)
    torch.cuda.synchronize()
    assert bool((cls == 7.0).all()), "a refused call enqueued something"
    m.set_head_mask(None)
    _same_state(before, _state(m))
    again = m.predict(b["ids"], seg_ids=b["seg"])
    assert torch.equal(again["cls"], ref["cls"]) and not torch.equal(comp["cls"], ref["cls"])


# ---- 6. --compact_heads end to end ----------------------------------------------------------------------------------------------------------
def test_cli_compact_heads(tmp_path):
    """the set-up of test_cli_head_importance_and_head_mask (f32, 2 layers, trained on valid_200 so that it predicts labels): the .pred
    file of --predict --head_mask pruned.json --compact_heads is byte-identical to the one without --compact_heads"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--lr", "1e-3", "--bert_lr", "1e-4", "--batchSize", "16", "--max_epoch", "4", "--experiment", exp,
              "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", "f32",
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "3", "--resume"]
    assert cli.main(common) == 0
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    n_in = len(open(src).read().strip("\n").split("\n"))
    L, heads = 2, 12
    pruned = [[1.0] * heads for _ in range(L)]
    for l, h in ((0, 3), (0, 8), (1, 0), (1, 5), (1, 11)):
        pruned[l][h] = 0.0
    pruned_path = str(tmp_path / "pruned.json")
    json.dump(pruned, open(pruned_path, "w"))
    gated_out, comp_out, plain_out = (str(tmp_path / n) for n in ("gated.pred", "compact.pred", "plain.pred"))
    assert cli.main(common + ["--predict", src, "--predict_output", gated_out, "--head_mask", pruned_path]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", comp_out, "--head_mask", pruned_path, "--compact_heads"]) == 0
    ga, co = open(gated_out).read().split("\n"), open(comp_out).read().split("\n")
    assert len(co) - 1 == n_in and len(ga) == len(co)
    diff = [i for i, (x, y) in enumerate(zip(ga, co)) if x != y]
    for i in diff:
        print("line %d differs:\n  gated   %s\n  compact %s" % (i, ga[i], co[i]))
    assert open(gated_out, "rb").read() == open(comp_out, "rb").read(), ".pred differs under --compact_heads (%d lines)" % len(diff)
    assert any(ln.split("\t<=>\t")[1] for ln in co[:-1]), "the model predicts no label at all"
