"""CPU: training under a head mask (nbest_encoder_desc.head_gate_stash, set_head_mask(trainable=True), --train_head_mask) on the
host - the descriptor field, the stash layout and the refused combinations (nothing is enqueued: null pointers do), the fp64
reference of the parameter gradients under a gate that the GPU tests compare against, the CLI flag and the model's checks."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN
from test_attrib_cpu import oracle_model
from test_cls_top_cpu import HEADER, _header_fields
from test_head_gate_cpu import case_tensors
from test_wgrad_window_cpu import _lib, _desc, BERT, NEVER, ALWAYS, WINDOW


# ---- 1. the descriptor field -----------------------------------------------------------------------------------------------------
DESC_BYTES = 320      # sizeof(nbest_encoder_desc) before the field took the padding slot after fp8_bwd


def test_descriptor_field_takes_the_padding_slot():
    hb, _ = _lib()
    names = [n for n, _ in hb.EncoderDesc._fields_]
    assert "head_gate_stash" in names and "pad2" not in names
    assert names[names.index("head_gate_stash") - 1] == "fp8_bwd"
    assert hb.EncoderDesc.head_gate_stash.offset == hb.EncoderDesc.fp8_bwd.offset + 4
    assert hb.EncoderDesc.head_gate_stash.size == 4
    assert hb.EncoderDesc.wpk.offset == hb.EncoderDesc.fp8_bwd.offset + 8             # nothing moved
    assert C.sizeof(hb.EncoderDesc) == DESC_BYTES
    hdr = [n for _, n in _header_fields()]
    assert hdr[hdr.index("fp8_bwd") + 1] == "head_gate_stash" and "pad2" not in hdr
    assert "head_gate_stash" in open(HEADER).read()
    assert hb.EncoderDesc().head_gate_stash == 0                                       # zero = today's behaviour


# ---- 2. layout and refusals --------------------------------------------------------------------------------------------------------
def _al(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("K", [0, 1, 3])
def test_stash_grows_by_one_region_per_stashed_layer(K, dtype):
    """act_bytes with the flag minus without = (L - K) al(M H esz), K = first_trainable in {0, 1, L}; the workspace does not change;
    the flag without a gate pointer changes no size.  (At the supported widths M H esz is a multiple of the 256-byte alignment, so the
    al() here states the layout's rule without being able to tell it from an unaligned region.)"""
    hb, lib = _lib()
    L, B, S = 3, 5, 33
    esz = 2 if dtype == "bf16" else 4
    for mode in (0, NEVER, ALWAYS, WINDOW):
        d = _desc(hb, L, B, S, mode=mode, first_trainable=K, **BERT)
        d.dtype = hb.BF16 if dtype == "bf16" else hb.F32
        act0, ws0 = lib.nbest_encoder_act_bytes(C.byref(d)), lib.nbest_encoder_ws_bytes(C.byref(d))
        d.head_gate_stash = 1
        assert lib.nbest_encoder_act_bytes(C.byref(d)) == act0 and lib.nbest_encoder_ws_bytes(C.byref(d)) == ws0
        d.head_gate = C.c_void_p(256)
        assert lib.nbest_encoder_act_bytes(C.byref(d)) - act0 == (L - K) * _al(B * S * BERT["H"] * esz), (mode, K, dtype)
        assert lib.nbest_encoder_ws_bytes(C.byref(d)) == ws0
        d.head_gate_stash = 0                                                          # a gate alone: today's stash
        assert lib.nbest_encoder_act_bytes(C.byref(d)) == act0


def test_act_view_offsets_do_not_move():
    """gctx comes after every other region: the qkv / lse pointers of every stashed layer are where they are without the flag"""
    hb, lib = _lib()
    L = 3
    lay = (hb.LayerOffsets * L)()
    for K in (0, 1):
        d = _desc(hb, L, 4, 24, first_trainable=K, **BERT)
        d.layers_host = lay
        views = []
        for flag in (0, 1):
            d.head_gate_stash = flag
            d.head_gate = C.c_void_p(256) if flag else None
            row = []
            for l in range(K, L):
                q, s = C.c_void_p(), C.c_void_p()
                assert lib.nbest_encoder_act_view(C.byref(d), C.c_void_p(4096), l, C.byref(q), C.byref(s)) == 0, hb.last_error()
                row.append((q.value, s.value))
            views.append(row)
        assert views[0] == views[1]


def _calls(lib, d):
    null = C.c_void_p()
    return {
        "forward": lambda: lib.nbest_encoder_forward(C.byref(d), null, null, null, null, null, null, null, 0, null, 0, None, null),
        "backward": lambda: lib.nbest_encoder_backward(C.byref(d), null, null, null, null, null, null, null, null, null, 0, null, null, 0,
                                                       0, d.first_trainable, d.L, 0, null),
    }


def test_refused_combinations():
    """every combination of the header's list is refused by the forward and the backward with a message that names head_gate_stash,
    before any pointer is looked at"""
    hb, lib = _lib()
    lay = (hb.LayerOffsets * 4)()
    one = C.c_void_p(256)

    def desc(**kw):
        d = _desc(hb, 4, 3, 16, **BERT)
        d.layers_host = lay
        d.head_gate_stash, d.head_gate = 1, one
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for word, kw in (("without head_gate", dict(head_gate=None)), ("fp8", dict(w8=one, w8_inv_scale=one)), ("emb_delta", dict(emb_delta=one)),
                     ("base_ids", dict(base_ids=one, alpha=one)), ("no_param_grad", dict(no_param_grad=1)),
                     ("head_gate_grad", dict(head_gate_grad=one))):
        d = desc(**kw)
        for what, call in _calls(lib, d).items():
            rc = call()
            msg = hb.last_error()
            assert rc < 0 and "head_gate_stash" in msg and word in msg, (what, word, rc, msg)


def test_accepted_combinations():
    """the flag alone, with cls_top, with first_trainable = 1 and = L, in both dtypes and every weight-gradient mode: the descriptor
    checks pass - the forward and the backward get as far as their null pointers; without the flag the two pinned refusals stand"""
    hb, lib = _lib()
    lay = (hb.LayerOffsets * 4)()
    one = C.c_void_p(256)
    for kw in ({}, {"cls_top": 1}, {"first_trainable": 1}, {"first_trainable": 1, "cls_top": 1}, {"first_trainable": 4, "cls_top": 1},
               {"dtype": hb.F32, "cls_top": 1}, {"wgrad_group": WINDOW}, {"wgrad_group": ALWAYS}):
        d = _desc(hb, 4, 3, 16, **BERT)
        d.layers_host = lay
        d.head_gate_stash, d.head_gate = 1, one
        for k, v in kw.items():
            setattr(d, k, v)
        for what, call in _calls(lib, d).items():
            assert call() < 0
            assert "null pointer" in hb.last_error(), (kw, what, hb.last_error())
        d.head_gate_stash = 0
        if kw.get("cls_top") or kw.get("first_trainable"):
            assert _calls(lib, d)["forward"]() < 0 and "head_gate" in hb.last_error() and "null pointer" not in hb.last_error()
        assert _calls(lib, d)["backward"]() < 0 and "head_gate" in hb.last_error() and "null pointer" not in hb.last_error()


def test_inference_ignores_the_flag():
    hb, lib = _lib()
    lay = (hb.LayerOffsets * 2)()
    d = _desc(hb, 2, 3, 16, **BERT)
    d.layers_host = lay
    d.head_gate_stash = 1                                   # (no gate: a training entry point refuses this)
    assert lib.nbest_encoder_infer(C.byref(d), None, None, None, None, None, None, None, 0, None, None) < 0
    assert "head_gate_stash" not in hb.last_error() and "null pointer" in hb.last_error()
    a = lib.nbest_encoder_infer_ws_bytes(C.byref(d))
    d.head_gate_stash = 0
    assert lib.nbest_encoder_infer_ws_bytes(C.byref(d)) == a


# ---- 3. the fp64 reference: parameter gradients under a gate -----------------------------------------------------------------------
def train_mask(L, heads):
    """the non-power-of-two mask of the parity tests: two zeros, a 0.3 and a 1.7 next to ones, at other heads in every layer (the four
    index formulas must not collide for the L in use: checked, every row holds all four values)"""
    m = torch.ones(L, heads, dtype=torch.float64)
    for l in range(L):
        picks = [(3 * l + 1) % heads, (7 * l + 10) % heads, (5 * l + 3) % heads, (2 * l + 7) % heads]
        assert len(set(picks)) == 4, "train_mask: head indices collide in layer %d of %d heads" % (l, heads)
        for h, v in zip(picks, (0.0, 0.0, 0.3, 1.7)):
            m[l, h] = v
        assert sorted(set(m[l].tolist())) == [0.0, 0.3, 1.0, 1.7] and int((m[l] == 0).sum()) == 2
    return m


def test_train_mask_has_every_gate_in_every_layer():
    for L in (1, 2, 3):
        m = train_mask(L, 12)
        for l in range(L):
            assert sorted(set(m[l].tolist())) == [0.0, 0.3, 1.0, 1.7], (L, l)
            assert int((m[l] == 0.3).sum()) == 1 and int((m[l] == 1.7).sum()) == 1 and int((m[l] == 0).sum()) == 2


def oracle_gated_loss(m, ocfg, labels, ids, seg, y, gate):
    """the graph-attached total loss of the oracle under ``gate`` [L, heads]: the forward hook of test_head_gate_cpu.oracle_gated (the
    gate on each layer's attention.self output, expanded over d), the loss of oracle/step.py without the MSE term"""
    from oracle import stc
    layers = m.bert_encoder.encoder.layer
    d = ocfg.hidden_size // ocfg.num_attention_heads
    g = gate.to(next(m.parameters()).dtype)
    hooks = [lyr.attention.self.register_forward_hook(lambda mod, inp, out, l=l: out * g[l].repeat_interleave(d)[None, None, :])
             for l, lyr in enumerate(layers)]
    try:
        top, bottoms, final, _, _ = m(ids, None, seg_ids=seg)
    finally:
        for h in hooks:
            h.remove()
    b2t = stc.bottom2top_matrix(labels.top2bottom).to(top.dtype)
    _, total, _ = stc.total_loss(top, bottoms, final, y.to(top.dtype), labels.top2bottom, b2t)
    return total, (top.detach(), {k: v.detach() for k, v in bottoms.items()}, final.detach())


def oracle_gated_param_grads(m, ocfg, labels, ids, seg, y, gate):
    """(total loss, {parameter name: d total / d parameter}, scores) of the oracle under ``gate``: total.backward() through the hook"""
    for p in m.parameters():
        p.grad = None
    total, scores = oracle_gated_loss(m, ocfg, labels, ids, seg, y, gate)
    total.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    return total.detach(), grads, scores


def test_oracle_parameter_gradients_under_a_gate_match_central_differences(labels):
    """1 layer, B 4, S 24, gates 0 / 0.3 / 1 / 1.7: autograd against a central difference in fp64 on entries of Wo, Wq and W1, within
    1e-6 of the entry's size plus 1e-8 (the bound and its reasoning are those of
    test_head_gate_cpu.test_oracle_gate_gradient_matches_central_difference: h = 1e-5, truncation O(h^2), cancellation about
    1e-11 |L|).  The Wo columns and the Q / K / V rows (weights and biases) of a gate-0 head are exactly zero"""
    meta = dict(family="bert", L=1, seed=11, B=4, S=24, n_best=3, St=8, seg=True)
    m, ocfg, cfg, _, batch = oracle_model(meta, labels)
    ids, seg, y = case_tensors(meta, batch)
    heads = ocfg.num_attention_heads
    gate = train_mask(1, heads)
    assert sorted(set(gate[0].tolist())) == [0.0, 0.3, 1.0, 1.7]
    zero_head, frac_head, big_head = 1, 3, 7
    assert gate[0, zero_head] == 0.0 and gate[0, frac_head] == 0.3 and gate[0, big_head] == 1.7
    _, grads, _ = oracle_gated_param_grads(m, ocfg, labels, ids, seg, y, gate)
    pre = "bert_encoder.encoder.layer.0."
    named = dict(m.named_parameters())
    h = 1e-5
    col = lambda hd, k: hd * 64 + k
    probes = [(pre + "attention.output.dense.weight", (5, col(frac_head, 3))), (pre + "attention.output.dense.weight", (700, col(big_head, 60))),
              (pre + "attention.output.dense.weight", (123, col(0, 17))), (pre + "attention.self.query.weight", (col(frac_head, 9), 40)),
              (pre + "attention.self.query.weight", (col(big_head, 0), 767)), (pre + "attention.self.query.weight", (col(2, 33), 5)),
              (pre + "intermediate.dense.weight", (100, 300)), (pre + "intermediate.dense.weight", (3000, 7))]
    with torch.no_grad():
        for n, idx in probes:
            p = named[n]
            keep = p[idx].item()
            p[idx] = keep + h
            hi = oracle_gated_loss(m, ocfg, labels, ids, seg, y, gate)[0].item()
            p[idx] = keep - h
            lo = oracle_gated_loss(m, ocfg, labels, ids, seg, y, gate)[0].item()
            p[idx] = keep
            fd, ag = (hi - lo) / (2 * h), grads[n][idx].item()
            print("%s%s: autograd %.6e, central difference %.6e, |diff| %.2e" % (n, list(idx), ag, fd, abs(fd - ag)))
            assert abs(fd - ag) <= 1e-6 * abs(ag) + 1e-8, (n, idx, fd, ag)
    sl = slice(zero_head * 64, zero_head * 64 + 64)
    assert grads[pre + "attention.output.dense.weight"][:, sl].abs().max().item() == 0.0
    assert grads[pre + "attention.output.dense.weight"][:, :64].abs().max().item() > 0.0
    for part in ("query", "key", "value"):
        assert grads[pre + "attention.self.%s.weight" % part][sl].abs().max().item() == 0.0, part
        assert grads[pre + "attention.self.%s.bias" % part][sl].abs().max().item() == 0.0, part
        assert grads[pre + "attention.self.%s.weight" % part][:64].abs().max().item() > 0.0, part


# ---- 4. the CLI ----------------------------------------------------------------------------------------------------------------------
PINNED_MASK = [[1, 0, 0.5] + [1] * 9, [1.0] * 11 + [0]]
PINNED_DIGEST = "23106a69"


def test_head_mask_digest_is_pinned():
    """sha1 of the entries as little-endian fp32, row-major, first 8 hex digits - restated here with struct and hashlib"""
    import hashlib
    import struct
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer
    raw = b"".join(struct.pack("<f", float(x)) for r in PINNED_MASK for x in r)
    assert trainer.head_mask_digest(PINNED_MASK) == hashlib.sha1(raw).hexdigest()[:8] == PINNED_DIGEST
    assert trainer.head_mask_digest([[1.0] * 12] * 2) != PINNED_DIGEST


def test_train_head_mask_cli_flags(tmp_path, monkeypatch):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    src = tmp_path / "in.txt"
    src.write_text(open(os.path.join(GOLDEN, "valid_head.txt")).read())
    mask = tmp_path / "mask.json"
    mask.write_text(json.dumps(PINNED_MASK))
    out = str(tmp_path / "imp.json")
    base = ["--dataset", "dstc2", "--dataroot", str(tmp_path), "--deviceId", "0"]
    opt = cli.parse_arguments(base + ["--train_head_mask", str(mask)])
    assert opt.train_head_mask == str(mask) and opt.head_mask is None
    plain = cli.parse_arguments(base)
    assert plain.train_head_mask is None
    # the experiment directory: __hm_<digest> last, only with the flag
    assert cli.exp_dir(opt) == cli.exp_dir(plain) + "__hm_" + PINNED_DIGEST
    assert "hm_" not in cli.exp_dir(plain)
    both = cli.parse_arguments(base + ["--train_head_mask", str(mask), "--rdrop_alpha", "0.5", "--freeze_layers", "1", "--ema_decay", "0.99"])
    assert cli.exp_dir(both).endswith("__rdrop_0.5__hm_" + PINNED_DIGEST)
    other = tmp_path / "other.json"
    other.write_text(json.dumps([[1.0] * 12] * 2))
    assert cli.exp_dir(cli.parse_arguments(base + ["--train_head_mask", str(other)])) != cli.exp_dir(opt)
    # combines with the other training flags
    for ok in (["--distill_from", str(mask)], ["--add_l2_loss"], ["--optim_choice", "adamw", "--restated_adamw"], ["--optim_choice", "adam"], ["--freeze_embeddings"],
               ["--resume"]):
        assert cli.parse_arguments(base + ["--train_head_mask", str(mask)] + ok).train_head_mask == str(mask)
    for bad in (["--testing"], ["--predict", str(src)], ["--head_importance", out], ["--head_mask", str(mask)],
                ["--testing", "--head_mask", str(mask)], ["--dtype", "fp8w"], ["--adv_epsilon", "1.0"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + ["--train_head_mask", str(mask)] + bad)
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--train_head_mask", str(tmp_path / "missing.json")])
    notjson = tmp_path / "bad.json"
    notjson.write_text("not json")
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--train_head_mask", str(notjson)])
    with pytest.raises(SystemExit):                                                    # --head_mask on a training run: still refused
        cli.parse_arguments(base + ["--head_mask", str(mask)])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--train_head_mask", str(mask)])


# ---- 5. the model's checks, device-free ----------------------------------------------------------------------------------------------
def _bare_model(**kw):
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    m = NBestSTCModel.__new__(NBestSTCModel)

    class _Cfg:
        num_hidden_layers, num_attention_heads = 2, 12
    m.__dict__.update(cfg=_Cfg(), _head_mask="sentinel", **kw)
    return NBestSTCModel, m


def test_set_head_mask_trainable_checks_need_no_device():
    M, m = _bare_model()
    assert m.head_mask_trainable is False
    with pytest.raises(ValueError, match=r"\[L=2, heads=12\]"):            # the shape check comes first, before the device is touched
        M.set_head_mask(m, torch.ones(12, 2), trainable=True)
    with pytest.raises(ValueError, match="trainable"):
        M.set_head_mask(m, None, trainable=True)
    assert m.__dict__["_head_mask"] == "sentinel" and m.head_mask_trainable is False
    M.set_head_mask(m, None)
    assert m.head_mask is None and m.head_mask_trainable is False
    with pytest.raises(AttributeError):                                      # read-only
        m.head_mask_trainable = True


def test_model_gates_under_a_trainable_mask():
    """_cls_top_ok and _refuse_training_under_mask, device-free: a trainable mask keeps the CLS-row top layer and lets
    forward_backward through; the bridge and an fp8w model stay refused; a plain mask refuses as before"""
    M, m = _bare_model(fp8_forward=False, cls_top=True)
    assert not M._cls_top_ok(m, True, 16, None)
    with pytest.raises(RuntimeError, match="head mask"):
        M._refuse_training_under_mask(m, "forward_backward(need_grad=True)")
    m.__dict__["_head_mask_trainable"] = True
    assert M._cls_top_ok(m, True, 16, None) and not M._cls_top_ok(m, False, 16, None) and not M._cls_top_ok(m, True, 1, None)
    M._refuse_training_under_mask(m, "forward_backward(need_grad=True)")
    with pytest.raises(RuntimeError, match="head mask"):
        M._refuse_training_under_mask(m, "the training forward (autograd bridge)", bridge=True)
    m.__dict__["fp8_forward"] = True
    with pytest.raises(RuntimeError, match="fp8w"):
        M._refuse_training_under_mask(m, "forward_backward(need_grad=True)")
    m.__dict__["_head_mask"] = None
    M._refuse_training_under_mask(m, "forward_backward(need_grad=True)")


def test_train_step_refuses_a_world_above_one(monkeypatch):
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer

    class _M:
        head_mask_trainable = True
    monkeypatch.setattr(trainer, "dist_info", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="head mask"):
        trainer.train_step(_M(), None, {})
