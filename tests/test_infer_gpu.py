"""GPU: forward-only inference (nbest_encoder_infer, NBestSTCModel.predict, --predict) - its kernels against the training-path
kernels, its outputs against the reference goldens and the eval forward, and the training state it must leave alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from test_model_gpu import FLOOR_FACTOR, SMALL_FACTOR, _build, _cmp, _cmp_floor, _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rnd(*shape, dtype=torch.float32, s=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * s).to(dtype).to(DEV)


# ---- 1. CLS-query attention against row 0 of the full attention forward --------------------------------------------------------
def _mask(kind, B, S, seed):
    g = np.random.default_rng(seed)
    m = np.ones((B, S), dtype=np.uint8)
    if kind == "bert":                              # right padding, row 0 full
        for b in range(1, B):
            m[b, int(g.integers(1, S + 1)):] = 0
    else:                                           # XLM-R under Q1: <s> (id 0) masked, <pad> (id 1) attended
        m[:, 0] = 0
    return torch.from_numpy(m).to(DEV)


CLS_CASES = [(S, heads, kind) for S in (1, 2, 5, 64, 128, 129, 256, 300, 512) for heads in (12, 16) for kind in ("bert", "xlmr")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S,heads,kind", CLS_CASES)
def test_cls_attention_matches_row0(S, heads, kind, dtype):
    from nbest_amd import hipabi as hb
    B, H = 3, heads * 64
    qkv = _rnd(B * S, 3 * H, dtype=dtype, s=1.5, seed=S * 31 + heads)
    mask = _mask(kind, B, S, S)
    ctx, _ = hb.attention_fwd(qkv, mask, B, S, heads)
    full = ctx.float()
    ref = full.view(B, S, H)[:, 0, :]
    got = hb.attention_cls_fwd(qkv, S * 3 * H, qkv[:, H:], 3 * H, mask, B, S, heads).float()
    torch.cuda.synchronize()
    # S = 1 under XLM-R masks the only key: the full-attention kernels give 0 (fp32) and NaN (bf16) there - matched as is
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "NaN pattern differs"
    ok = ~torch.isnan(ref)
    err = (got[ok] - ref[ok]).abs().max().item() if ok.any() else 0.0
    scale = full[~torch.isnan(full)].abs().max().item() if ok.any() else 0.0      # max|ctx| over the whole attention output
    bar = (1e-6 if dtype == torch.float32 else 2.0 ** -8) * scale
    assert err <= bar, "S=%d heads=%d %s %s: |err| %.3e > %.3e" % (S, heads, kind, dtype, err, bar)


# ---- 2. GELU epilogue without U ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,dtype", [(256, 3072, 768, torch.bfloat16), (32768, 3072, 768, torch.bfloat16),
                                         (8192, 4096, 1024, torch.bfloat16), (300, 3072, 768, torch.float32)])
def test_gelu_epilogue_without_u_is_bit_identical(M, N, K, dtype):
    from nbest_amd import hipabi as hb
    A, W, bias = _rnd(M, K, dtype=dtype, seed=1), _rnd(N, K, dtype=dtype, s=0.05, seed=2), _rnd(N, seed=3)
    variants = [dict()]
    if dtype == torch.bfloat16:
        Wp, bn = hb.pack_weight(W)
        assert Wp is not None
        variants.append(dict(B_packed=Wp, b_pack_bn=bn))
    for kw in variants:
        ref, U = hb.gemm(A, W, M, N, K, epilogue=hb.EPI_BIAS_GELU, bias=bias, **kw)
        got = hb.gemm(A, W, M, N, K, epilogue=hb.EPI_BIAS_GELU, bias=bias, want_u=False, **kw)
        assert torch.equal(got, ref), "C differs without U: M=%d N=%d K=%d %s packed=%s" % (M, N, K, dtype, bool(kw))


# ---- 3. parity with the reference goldens --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2", "bert_L12", "xlmr_L12", "xlmrL_L4_S256"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_predict_matches_reference_outputs(name, dtype, labels):
    meta, z = load_case(name)
    m, b = _build(meta, labels, dtype)
    out = m.predict(b["ids"], seg_ids=b["seg"] if meta["seg"] else None)
    torch.cuda.synchronize()
    tag = "predict %s/%s " % (name, "f32" if dtype == torch.float32 else "bf16")
    for key, val in (("top", out["top"]), ("final", out["final"]), ("bottoms", out["bott"])):
        if dtype == torch.float32:
            _cmp(tag + key, val, z[key], atol=1e-4)
        else:
            _cmp_floor(tag + key, val, z[key], z["floor/" + key], factor=SMALL_FACTOR)
    if dtype == torch.float32:
        _cmp(tag + "asr_cls", out["cls"], z["asr_cls"], atol=2e-4 if meta["L"] <= 2 else 4e-4)
        assert np.array_equal(out["pred"].cpu().numpy(), z["decode"]), "decoded label indices differ from the reference"
    else:
        _cmp_floor(tag + "asr_cls", out["cls"], z["asr_cls"], z["floor/asr_cls"], factor=FLOOR_FACTOR)


# ---- 4. agreement with the eval forward on the same model ----------------------------------------------------------------------
def _model(labels, family="bert", L=2, dtype=torch.float32, seed=7, fp8=False):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    mk = {"bert": ncfg.bert_base, "xlm-roberta": ncfg.xlmr_base}[family]
    cfg = mk(num_hidden_layers=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    sd = synth.model_state(cfg, labels, seed=seed)
    m = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=dtype, dropout=0.3, seed=seed, fp8_forward=fp8)
    m.load_reference_state(sd)
    return m, cfg, sd


def _batch(cfg, labels, B, S, seed=3, row0_shortest=False):
    from nbest_amd import synth
    bt = synth.nbest_batch(cfg, labels, B, S, n_best=5 if S >= 32 else 1, seed=seed, ragged=S >= 8, trans_len=16,
                           row0_shortest=row0_shortest)
    return {k: torch.from_numpy(v).to(DEV) for k, v in bt.items()}


AGREE = [("bert", 1, 5, False), ("bert", 3, 40, False), ("bert", 256, 128, False), ("bert", 2, 512, False),
         ("xlm-roberta", 3, 40, True), ("xlm-roberta", 16, 128, True)]


@pytest.mark.parametrize("family,B,S,row0_shortest", AGREE)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_predict_agrees_with_eval_forward(family, B, S, row0_shortest, dtype, labels):
    m, cfg, _ = _model(labels, family, dtype=dtype)
    b = _batch(cfg, labels, B, S, row0_shortest=row0_shortest)
    seg = b["seg"] if family == "bert" else None
    m.eval()
    ev = m.forward_backward(b["ids"], b["labels"], seg_ids=seg, need_grad=False)
    pr = m.predict(b["ids"], seg_ids=seg)
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    tag = "agree %s B=%d S=%d %s " % (family, B, S, "f32" if f32 else "bf16")
    same = torch.equal(pr["cls"], ev["asr_cls"]) and torch.equal(pr["final"], ev["final"])
    _log(tag + "bits of cls and final %s" % ("IDENTICAL" if same else "differ"))
    _cmp(tag + "cls", pr["cls"], ev["asr_cls"].float().cpu(), rtol=1e-5 if f32 else 2.0 ** -7)
    _cmp(tag + "final", pr["final"], ev["final"].cpu(), atol=1e-6 if f32 else 2e-3)
    if f32:
        assert torch.equal(pr["pred"], m.decode(ev["top"], ev["bott"])), "decoded labels differ from the eval forward"


# ---- 5. no side effects ----------------------------------------------------------------------------------------------------------
def _state(m, opt=None):
    a = m.arena
    snap = {"p": a.p.clone(), "g": a.g.clone(), "weights": a.weights.clone(), "step": m.step_counter}
    for k in ("m", "v", "aamax", "aamax_slots", "gamax", "gamax_slots"):
        t = getattr(a, k, None)
        if t is not None:
            snap[k] = t.clone()
    snap["stash"] = {k: (v.data_ptr(), v.numel(), v.clone()) for k, v in m._stash.items()}
    snap["dh"] = None if m._dh is None else (m._dh.data_ptr(), m._dh.clone())
    snap["stash_gen"] = dict(m._stash_gen)
    snap["valid"] = (m._aamax_valid, m._gamax_valid)
    return snap


def _same_state(s1, s2):
    assert s1.keys() == s2.keys()
    for k in s1:
        if k == "stash":
            assert s1[k].keys() == s2[k].keys()
            for slot in s1[k]:
                p1, n1, c1 = s1[k][slot]
                p2, n2, c2 = s2[k][slot]
                assert (p1, n1) == (p2, n2) and torch.equal(c1, c2), "stash of slot %s changed" % slot
        elif k == "dh":
            assert (s1[k] is None) == (s2[k] is None)
            if s1[k] is not None:
                assert s1[k][0] == s2[k][0] and torch.equal(s1[k][1], s2[k][1]), "_dh changed"
        elif isinstance(s1[k], torch.Tensor):
            assert torch.equal(s1[k], s2[k]), "%s changed" % k
        else:
            assert s1[k] == s2[k], "%s changed" % k


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8w"])
def test_predict_leaves_training_state_alone(mode, labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, dtype=torch.float32 if mode == "f32" else torch.bfloat16, fp8=mode == "fp8w")
    m.train()
    b = _batch(cfg, labels, 4, 48)
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    for _ in range(2):
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        opt.step()
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
    torch.cuda.synchronize()
    before = _state(m)
    m.predict(b["ids"], seg_ids=b["seg"])
    m.predict(b["ids"][:3, :40].contiguous(), seg_ids=b["seg"][:3, :40].contiguous())
    torch.cuda.synchronize()
    _same_state(before, _state(m))


def test_predict_between_bridge_forward_and_backward(labels):
    outs = []
    for with_predict in (False, True):
        m, cfg, _ = _model(labels, dtype=torch.float32)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        m.zero_grad()
        top, bottoms, fin, asr_cls, _ = m(None, b["ids"], seg_ids=b["seg"])
        if with_predict:
            m.predict(b["ids"], seg_ids=b["seg"])
        (fin.sum() + 0.5 * top.sum() + 0.1 * asr_cls.sum()).backward()
        torch.cuda.synchronize()
        outs.append(m.arena.g.clone())
    assert torch.equal(outs[0], outs[1]), "gradients differ when predict() runs between forward() and backward()"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_after_predict_is_unchanged(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_predict in (False, True):
        m, cfg, _ = _model(labels, dtype=dtype)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_predict:
            m.predict(b["ids"], seg_ids=b["seg"])
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after predict() differs"


# ---- 6. fp8w model predicts with its bf16 weights ----------------------------------------------------------------------------------
def test_fp8w_predict_equals_bf16_predict(labels):
    m8, cfg, sd = _model(labels, dtype=torch.bfloat16, fp8=True)
    mb, _, _ = _model(labels, dtype=torch.bfloat16)
    b = _batch(cfg, labels, 16, 64)
    o8, ob = m8.predict(b["ids"], seg_ids=b["seg"]), mb.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    for k in ("cls", "top", "bott", "final", "pred"):
        assert torch.equal(o8[k], ob[k]), k


# ---- 7. memory ---------------------------------------------------------------------------------------------------------------------
def test_predict_peak_memory(labels):
    import gc
    incs = {}
    for leg in ("eval", "predict"):
        m, cfg, _ = _model(labels, L=12, dtype=torch.bfloat16)
        m.eval()
        b = _batch(cfg, labels, 256, 128)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        if leg == "eval":
            m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)
        else:
            m.predict(b["ids"], seg_ids=b["seg"])
        torch.cuda.synchronize()
        incs[leg] = torch.cuda.max_memory_allocated() - base
        del m, b
        gc.collect()
        torch.cuda.empty_cache()
    _log("peak memory increase: eval %.1f MB, predict %.1f MB (ratio %.1f)" % (incs["eval"] / 2**20, incs["predict"] / 2**20,
                                                                               incs["eval"] / max(incs["predict"], 1)))
    assert 8 * incs["predict"] <= incs["eval"], incs


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(labels):
    from nbest_amd import hipabi as hb
    m, cfg, _ = _model(labels, dtype=torch.bfloat16)
    ids = torch.full((2, 520), 5, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="S=520"):
        m.predict(ids)
    b = _batch(cfg, labels, 2, 16)
    ps = m._desc(2, 16, "refusal")
    ids, seg, pos, mask = m._inputs(b["ids"], b["seg"])
    ws = torch.empty(hb.lib().nbest_encoder_infer_ws_bytes(C.byref(ps.desc)), dtype=torch.uint8, device=DEV)
    cls = torch.empty(2, cfg.hidden_size, dtype=torch.bfloat16, device=DEV)
    call = lambda: hb.lib().nbest_encoder_infer(C.byref(ps.desc), hb.ptr(m.arena.weights), hb.ptr(m.arena.p), hb.ptr(ids), hb.ptr(seg),
                                                hb.ptr(pos), hb.ptr(mask), hb.ptr(ws), ws.numel(), hb.ptr(cls), hb.stream_ptr())
    d = ps.desc
    d.hidden_drop, d.attn_drop = 0.1, 0.0
    assert call() == -1 and "dropout" in hb.last_error()
    d.hidden_drop, d.attn_drop = 0.0, 0.1
    assert call() == -1 and "dropout" in hb.last_error()
    d.attn_drop = 0.0
    m8, _, _ = _model(labels, dtype=torch.bfloat16, fp8=True)
    d.w8, d.w8_inv_scale = m8.arena.w8.data_ptr(), m8.arena.w8_inv_scale.data_ptr()
    assert call() == -1 and "fp8" in hb.last_error()
    d.w8 = d.w8_inv_scale = None
    assert call() == 0
    torch.cuda.synchronize()


# ---- 9. CLI end to end ---------------------------------------------------------------------------------------------------------------
def test_cli_predict_matches_eval_pred_column(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--lr", "3e-5", "--bert_lr", "3e-5", "--batchSize", "16", "--max_epoch", "1", "--experiment", exp,
              "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", "f32",
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "5", "--resume"]
    assert cli.main(common) == 0
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):     # written on a new best valid F1 only: the epoch's weights are in last.pt
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    assert cli.main(common + ["--predict", src]) == 0
    got = open(os.path.join(d, "valid.pred")).read().split("\n")[:-1]
    ref = open(os.path.join(d, "valid.iter0")).read().split("\n")[:-1]
    n_in = len(open(src).read().strip("\n").split("\n"))
    assert len(got) == n_in == len(ref)
    for g, r in zip(got, ref):
        gf, rf = g.split("\t<=>\t"), r.split("\t<=>\t")
        assert len(gf) == 2 and gf[0] == rf[0] and gf[1] == rf[1], (g, r)
    asr_only = tmp_path / "asr_only.txt"
    asr_only.write_text("".join(l.split("\t<=>\t")[0] + "\n" for l in open(src).read().strip("\n").split("\n")))
    out2 = str(tmp_path / "asr_only.pred")
    assert cli.main(common + ["--predict", str(asr_only), "--predict_output", out2]) == 0
    assert open(out2).read().split("\n")[:-1] == got
