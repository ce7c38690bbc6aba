"""The top encoder layer on the CLS rows only (nbest_encoder_desc.cls_top), on the host: the descriptor field and its ctypes mirror,
the combinations the library refuses before anything is enqueued, what the flag does to the grouped / window queue, and the model's
choice of the flag.  Nothing is enqueued: no GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import GOLDEN
from test_wgrad_window_cpu import _lib, _desc, _coverage, _matrix_tiles, BERT, WINDOW, NEVER

HEADER = os.path.join(os.path.dirname(GOLDEN), "..", "include", "nbest_hip.h")


def _header_fields():
    """(type, name) of every member of nbest_encoder_desc in include/nbest_hip.h, comments stripped, in order"""
    hdr = open(HEADER).read()
    body = hdr[hdr.index("typedef struct nbest_encoder_desc {"):hdr.index("} nbest_encoder_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body.split("{", 1)[1], flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(.*?[\s\*])(\w+(?:\s*,\s*\w+)*)$", decl)
        typ, names = m.group(1).strip(), [n.strip() for n in m.group(2).split(",")]
        out += [(typ, n) for n in names]
    return out


def test_descriptor_mirror_order_and_size():
    """hipabi.EncoderDesc against the header, member by member: same names in the same order (the mirror calls the padding members
    pad2 / pad5, pad5 = wgrad_group), each with the size of its C type, so every offset and the struct size agree; cls_top sits in
    what was padding after fp8_act - ahead of base_ids, and the last four fields stay where tests/test_attrib_cpu.py pins them"""
    hb, _ = _lib()
    hdr = _header_fields()
    mirror = list(hb.EncoderDesc._fields_)
    alias = {"pad5": "wgrad_group"}
    assert [alias.get(n, n) for n, _ in mirror] == [n for _, n in hdr]
    size_of = lambda t: 8 if "*" in t or t in ("int64_t", "uint64_t") else 4
    assert all(t in ("int32_t", "uint32_t", "float", "int64_t", "uint64_t") or "*" in t for t, _ in hdr), hdr
    off = 0
    for (typ, name), (mname, ctype) in zip(hdr, mirror):
        sz = size_of(typ)
        assert C.sizeof(ctype) == sz, (name, typ, ctype)
        off = (off + sz - 1) // sz * sz                      # natural alignment, as the C compiler lays the struct out
        assert getattr(hb.EncoderDesc, mname).offset == off, (name, off)
        off += sz
    assert C.sizeof(hb.EncoderDesc) == (off + 7) // 8 * 8
    names = [n for n, _ in mirror]
    i = names.index("cls_top")
    assert names[i - 1] == "fp8_act" and names[i + 1] == "first_trainable" and i < names.index("base_ids")
    assert hb.EncoderDesc.cls_top.offset == hb.EncoderDesc.fp8_act.offset + 4
    assert hb.EncoderDesc.first_trainable.offset == hb.EncoderDesc.cls_top.offset + 4      # the slot was padding: nothing moved
    assert names[-4:] == ["base_ids", "alpha", "no_param_grad", "pad5"]
    assert hb.EncoderDesc().cls_top == 0                                                   # zero = today's launches


def _refused(hb, lib, d, word):
    """forward, backward, act_view and wgrad_plan all refuse ``d`` with a message that names the flag and ``word``; the descriptor
    checks run before any pointer is looked at, so null pointers do"""
    null = C.c_void_p()
    calls = {
        "forward": lambda: lib.nbest_encoder_forward(C.byref(d), null, null, null, null, null, null, null, 0, null, 0, None, null),
        "backward": lambda: lib.nbest_encoder_backward(C.byref(d), null, null, null, null, null, null, null, null, null, 0, null, null, 0,
                                                       0, 0, d.L, 0, null),
        "act_view": lambda: lib.nbest_encoder_act_view(C.byref(d), C.c_void_p(256), d.first_trainable if d.first_trainable < d.L else 0,
                                                       C.byref(C.c_void_p()), C.byref(C.c_void_p())),
        "wgrad_plan": lambda: lib.nbest_encoder_wgrad_plan(C.byref(d), min(d.first_trainable, d.L), d.L, None, 0),
    }
    for what, call in calls.items():
        rc = call()
        msg = hb.last_error()
        assert rc < 0, (what, rc)
        assert "cls_top" in msg and word in msg, (what, msg)


def test_refused_combinations():
    hb, lib = _lib()
    lay = (hb.LayerOffsets * 4)()

    def desc(**kw):
        d = _desc(hb, 4, 3, 16, **BERT)
        d.layers_host = lay
        d.cls_top = 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    one = C.c_void_p(256)
    _refused(hb, lib, desc(w8=one, w8_inv_scale=one), "fp8")
    _refused(hb, lib, desc(head_gate=one), "head_gate")
    _refused(hb, lib, desc(base_ids=one, alpha=one), "base_ids")
    _refused(hb, lib, desc(no_param_grad=1), "no_param_grad")
    _refused(hb, lib, desc(S=1), "S >= 2")
    # first_trainable == L is accepted (an all-frozen encoder's heads must see the CLS rows a trainable one gives them, bit for bit:
    # tests/test_freeze_gpu.py): the forward gets as far as its null pointers
    d = desc(first_trainable=4)
    assert lib.nbest_encoder_forward(C.byref(d), None, None, None, None, None, None, None, 0, None, 0, None, None) < 0
    assert "null pointer" in hb.last_error()
    # the flag alone passes the descriptor checks: the forward then stops at its null pointers, the plan answers
    d = desc()
    assert lib.nbest_encoder_forward(C.byref(d), None, None, None, None, None, None, None, 0, None, 0, None, None) < 0
    assert "null pointer" in hb.last_error()
    assert hb.encoder_wgrad_plan(d, 0, 4)["mode"] in (NEVER, 2, WINDOW)
    # ... and fp32 is allowed
    d.dtype = hb.F32
    assert lib.nbest_encoder_forward(C.byref(d), None, None, None, None, None, None, None, 0, None, 0, None, None) < 0
    assert "null pointer" in hb.last_error()
    # act_view: the top layer of such a stash has no lse; the layers below are served as ever
    d = desc()
    q, l = C.c_void_p(), C.c_void_p()
    assert lib.nbest_encoder_act_view(C.byref(d), C.c_void_p(256), 3, C.byref(q), C.byref(l)) < 0
    assert "cls_top" in hb.last_error()
    assert lib.nbest_encoder_act_view(C.byref(d), C.c_void_p(256), 2, C.byref(q), C.byref(l)) == 0


def test_inference_ignores_the_flag():
    """nbest_encoder_infer with the flag set stops where it stops without it: at its null pointers, not at a cls_top refusal -
    also in a combination the training entry points refuse"""
    hb, lib = _lib()
    lay = (hb.LayerOffsets * 2)()
    for kw in ({}, {"first_trainable": 2}):
        d = _desc(hb, 2, 3, 16, **BERT)
        d.layers_host = lay
        d.cls_top = 1
        for k, v in kw.items():
            setattr(d, k, v)
        assert lib.nbest_encoder_infer(C.byref(d), None, None, None, None, None, None, None, 0, None, None) < 0
        assert "cls_top" not in hb.last_error() and "null pointer" in hb.last_error()
        d.cls_top = 0
        a = hb.lib().nbest_encoder_infer_ws_bytes(C.byref(d))
        d.cls_top = 1
        assert hb.lib().nbest_encoder_infer_ws_bytes(C.byref(d)) == a


def test_sizes_do_not_depend_on_the_flag():
    """the flag is set per call on a descriptor whose stash and workspace were sized before: both sizes ignore it"""
    hb, lib = _lib()
    for mode in (0, NEVER, 2, WINDOW):
        for dtype in (hb.BF16, hb.F32):
            d = _desc(hb, 4, 4, 128, mode=mode, **BERT)
            d.dtype = dtype
            sizes = []
            for flag in (0, 1):
                d.cls_top = flag
                sizes.append((lib.nbest_encoder_act_bytes(C.byref(d)), lib.nbest_encoder_ws_bytes(C.byref(d)),
                              lib.nbest_encoder_wgrad_launches_per_layer(C.byref(d))))
            assert sizes[0] == sizes[1], (mode, dtype, sizes)


def test_window_queue_leaves_out_the_top_layers_small_gradients():
    """WINDOW at the 4-layer bert-base-width shape: a call that ends at L queues the top layer's QKV gradient only (its other three
    are plain launches over the B CLS rows); every other (layer, matrix) is covered exactly once, as without the flag; a call that
    ends below L is untouched"""
    hb, _ = _lib()
    L, tiles = 4, _matrix_tiles(**BERT)
    d = _desc(hb, L, 4, 128, mode=WINDOW, **BERT)
    base = {(lo, hi): hb.encoder_wgrad_plan(d, lo, hi) for (lo, hi) in ((0, 4), (3, 4), (0, 3), (2, 4))}
    d.cls_top = 1
    for (lo, hi), was in base.items():
        plan = hb.encoder_wgrad_plan(d, lo, hi)
        assert plan["mode"] == WINDOW and plan["sets"] == was["sets"]
        if hi < L:
            assert plan == was
            continue
        seen = _coverage(plan, lo, hi)
        peel = plan["peel_layer"]
        for l in range(lo, hi):
            for j in range(4):
                if l == L - 1 and j > 0:
                    assert (l, j) not in seen
                elif l == peel and j < 2:
                    assert (l, j) not in seen
                else:
                    assert seen[(l, j)] == tiles[j], (l, j)
    # a caller's own skip flags still count
    skip = [0] * (4 * L)
    skip[4 * 3 + 0] = skip[4 * 1 + 2] = 1
    d = _desc(hb, L, 4, 128, mode=WINDOW, skip=skip, **BERT)
    d.cls_top = 1
    seen = _coverage(hb.encoder_wgrad_plan(d, 0, 4), 0, 4)
    assert not any(k[0] == 3 for k in seen) and (1, 2) not in seen and seen[(1, 3)] == tiles[3]


def test_model_sets_the_flag_for_training_passes_only():
    """_cls_top_ok, device-free: on for a training pass whatever is frozen, off for eval passes, when switched off, under the fp8
    forward, under a head mask and at S = 1"""
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    m = NBestSTCModel.__new__(NBestSTCModel)

    class _Cfg:
        num_hidden_layers = 2

    class _Plan:
        def __init__(self, ft):
            self.first_trainable = ft

    m.__dict__.update(cfg=_Cfg(), _head_mask=None, fp8_forward=False, cls_top=True)
    ok = NBestSTCModel._cls_top_ok
    assert ok(m, True, 16, None) and ok(m, True, 2, _Plan(1)) and ok(m, True, 16, _Plan(2))
    assert not ok(m, False, 16, None)
    assert not ok(m, True, 1, None)
    for k, v in (("cls_top", False), ("fp8_forward", True), ("_head_mask", object())):
        keep = m.__dict__[k]
        m.__dict__[k] = v
        assert not ok(m, True, 16, None), k
        m.__dict__[k] = keep
    assert ok(m, True, 16, None)
