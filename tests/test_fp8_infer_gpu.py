"""fp8 inference on the GPU: the NBEST_EPI_BIAS_GELU_Q8 epilogue against BIAS_GELU byte for byte, nbest_fp8_amax_fold_max, the calibration
pass, predict(fp8=True) against the reference goldens (the committed floor8/ entries) and the oracle's fp8 leg, reproducibility,
training state, refusals and the command line."""
import ctypes as C
import os
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_infer_gpu import _batch, _model, _same_state, _state
from test_model_gpu import FLOOR_FACTOR, SMALL_FACTOR, _build, _cmp_floor, _oracle_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_KEYS = ("cls", "top", "bott", "final", "pred")


def _bits(v):
    return torch.tensor([v], dtype=torch.float32).view(torch.int32).to(DEV)


# ---- 1. the epilogue: the bytes of BIAS_GELU ---------------------------------------------------------------------------------------
# (N, K) of the issue - at M <= 300 every one of them takes the 128-column tile (nbest_gemm_fp8's rule: N ceil(M / 256) <= 98 304 and
# K <= 1024) - plus the FFN-down shape (768, 3072), whose K > 1024 takes the 256-column tile at any M: both widths run.
NK = [(768, 768), (3072, 768), (256, 64), (4096, 1024), (768, 3072)]
PAD = 4096


def test_q8_cases_run_both_tile_widths():
    from nbest_amd import hipabi as hb
    assert {hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU_Q8)["bn"] for M in (40, 300) for N, K in NK} == {128, 256}


class Guarded:
    """an [M, N] byte matrix inside a buffer of 0xA5 bytes: the windows before and after it must stay as they are"""

    def __init__(self, M, N):
        self.buf = torch.full((2 * PAD + M * N,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.buf[PAD:PAD + M * N].view(M, N)

    def windows_intact(self):
        n = self.t.numel()
        return bool((self.buf[:PAD] == 0xA5).all()) and bool((self.buf[PAD + n:] == 0xA5).all())


@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("M", [40, 300])
def test_q8_writes_the_bytes_of_bias_gelu(M, N, K):
    from nbest_amd import hipabi as hb
    g = torch.Generator().manual_seed(1000 * M + N + K)
    A8 = hb.cast_fp8(torch.randn(M, K, generator=g).to(DEV).bfloat16())
    W8 = hb.cast_fp8(torch.randn(N, K, generator=g).to(DEV).bfloat16())
    bias = (0.5 * torch.randn(N, generator=g)).to(DEV)
    osd = torch.tensor([2.0 / K ** 0.5], device=DEV)            # pre-activations of a few units: both tails and the middle of gelu
    a_amax, c_prev = _bits(3.0), _bits(0.7)
    Wp, pbn = hb.pack_weight_fp8(W8)
    plan = hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU_Q8)
    assert plan == hb.gemm_fp8_plan_shape(M, N, K, epilogue=hb.EPI_BIAS_GELU)
    for prev, packed in ((None, False), (c_prev, True), (c_prev, False)):
        kw = dict(bias=bias, out_scale_dev=osd, a_amax=a_amax, c8_amax_prev=prev)
        if packed:
            kw.update(B_packed=Wp, b_pack_bn=pbn)
        _, _, ref8 = hb.gemm_fp8(A8, W8, M, N, K, epilogue=hb.EPI_BIAS_GELU, **kw)
        out = Guarded(M, N)
        hb.gemm_fp8(A8, W8, M, N, K, epilogue=hb.EPI_BIAS_GELU_Q8, C8=out.t, want_c=False, **kw)
        torch.cuda.synchronize()
        assert out.windows_intact(), "Q8 wrote outside C8"
        assert torch.equal(out.t, ref8), "C8 of Q8 differs from BIAS_GELU's (%d bytes; history %s, packed %s)" % (
            int((out.t != ref8).sum()), prev is not None, packed)
        assert bool((ref8 != 0).any()), "a degenerate case: every byte is zero"


def test_q8_refused_calls_write_nothing():
    from nbest_amd import hipabi as hb
    M, N, K = 40, 256, 64
    A8 = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    W8 = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    bias = torch.ones(N, device=DEV)
    out = Guarded(M, N)
    out.t.fill_(0x5A)
    slots = torch.zeros(hb.AMAX_TENSOR_WORDS, dtype=torch.int32, device=DEV)
    U = torch.full((M, N), 0x5A, dtype=torch.uint8, device=DEV)
    Cb = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=DEV)
    for kw in (dict(want_c=True, out=Cb), dict(want_c=False, U=U), dict(want_c=False, c8_amax_slots=slots), dict(want_c=False, bias=None)):
        kw.setdefault("bias", bias)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            hb.gemm_fp8(A8, W8, M, N, K, epilogue=hb.EPI_BIAS_GELU_Q8, C8=out.t, **kw)
    g = hb.GemmFp8Args()
    g.A, g.B, g.bias = A8.data_ptr(), W8.data_ptr(), bias.data_ptr()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.ldc8, g.epilogue, g.out_scale = M, N, K, K, K, N, N, hb.EPI_BIAS_GELU_Q8, 1.0
    assert hb.lib().nbest_gemm_fp8(C.byref(g), hb.stream_ptr()) == -1                      # C8 == NULL
    torch.cuda.synchronize()
    assert out.windows_intact() and bool((out.t == 0x5A).all()) and bool((U == 0x5A).all()) and bool((Cb == 3.0).all())
    assert not bool(slots.any())


# ---- 2. nbest_fp8_amax_fold_max ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 48])
def test_amax_fold_max(n):
    from nbest_amd import hipabi as hb
    W = hb.AMAX_TENSOR_WORDS
    g = torch.Generator().manual_seed(n)
    slots = torch.randn(n, W, generator=g).abs().view(torch.int32).to(DEV)
    used = torch.arange(16, device=DEV) * (W // 16)
    smax = slots[:, used].view(torch.float32).max(dim=1).values
    factor = torch.where(torch.arange(n, device=DEV) % 2 == 0, 0.5, 2.0)           # every other entry below / above its slot maximum
    out = (smax * factor).view(torch.int32).clone()
    want = torch.maximum(out.view(torch.float32), smax).view(torch.int32)
    before = slots.clone()
    flat = slots.view(-1)
    hb.fp8_amax_fold_max(flat, out)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert not bool(slots[:, used].any()), "the 16 slot words are not zeroed"
    keep = torch.ones(W, dtype=torch.bool, device=DEV)
    keep[used] = False
    assert torch.equal(slots[:, keep], before[:, keep]), "words outside the 16 slots changed"


# ---- 3. calibration pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,B,S,row0", [("bert", 16, 64, False), ("xlm-roberta", 3, 40, True)])
def test_calibration_pass(family, B, S, row0, labels):
    m, cfg, _ = _model(labels, family, dtype=torch.bfloat16, fp8=True)
    bA, bB = _batch(cfg, labels, B, S, seed=3, row0_shortest=row0), _batch(cfg, labels, B, S, seed=4, row0_shortest=row0)
    seg = lambda b: b["seg"] if family == "bert" else None
    assert m.fp8_calibrated == 0
    ref = m.predict(bA["ids"], seg_ids=seg(bA))
    got = m.fp8_calibrate(bA["ids"], seg_ids=seg(bA))
    for k in OUT_KEYS:
        assert torch.equal(got[k], ref[k]), k
    calA = m.fp8_calibration()
    m.fp8_calibrate(bB["ids"], seg_ids=seg(bB))
    calAB = m.fp8_calibration()
    assert m.fp8_calibrated == 2
    m.fp8_calibrate(bB["ids"], seg_ids=seg(bB), reset=True)
    calB = m.fp8_calibration()
    assert m.fp8_calibrated == 1
    assert torch.equal(calAB, torch.maximum(calA, calB)) and not torch.equal(calA, calB)
    L = cfg.num_hidden_layers
    live = torch.cat([calA[:L - 1].reshape(-1), calA[L - 1, :1]])
    assert bool(torch.isfinite(live).all()) and bool((live > 0).all()), calA
    assert calA.dtype == torch.float32 and tuple(calA.shape) == (L, 4)
    m.load_fp8_calibration(calA.cpu())
    assert m.fp8_calibrated == 1 and torch.equal(m.fp8_calibration(), calA)


# ---- 4. parity with the reference goldens ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2", "bert_L12", "xlmrL_L4_S256"])
def test_fp8_predict_matches_reference_outputs(name, labels):
    meta, z = load_case(name)
    m, b = _build(meta, labels, "fp8w")
    seg = b["seg"] if meta["seg"] else None
    m.fp8_calibrate(b["ids"], seg_ids=seg)               # the scales are then the own-amax scales of the oracle's fp8 leg
    out = m.predict(b["ids"], seg_ids=seg, fp8=True)
    torch.cuda.synchronize()
    tag = "predict fp8 %s " % name
    errs = []
    for key, val, factor in (("top", out["top"], SMALL_FACTOR), ("final", out["final"], SMALL_FACTOR), ("bottoms", out["bott"], SMALL_FACTOR),
                             ("asr_cls", out["cls"], FLOOR_FACTOR)):
        try:
            _cmp_floor(tag + key, val, z[key], z["floor8/" + key], factor=factor)      # (logs HIP / floor)
        except AssertionError as e:
            errs.append(str(e))
    assert not errs, "\n".join(errs)


# ---- 5. edge shapes against a floor computed here ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L,B,S,row0", [("bert", 1, 1, 5, False), ("bert", 2, 3, 40, False), ("xlm-roberta", 2, 8, 64, True),
                                               ("bert", 2, 2, 512, False)])
def test_fp8_predict_edge_shapes_match_oracle(family, L, B, S, row0, labels):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, synth
    from nbest_amd.model import NBestSTCModel
    from oracle import bf16sim
    mk = {"bert": ncfg.bert_base, "xlm-roberta": ncfg.xlmr_base}[family]
    cfg = mk(num_hidden_layers=L, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=31)
    batch = synth.nbest_batch(cfg, labels, B, S, n_best=2 if S < 16 else 5, seed=S, ragged=True, trans_len=8, row0_shortest=row0)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    with torch.no_grad():
        top, _, final, _, _ = om(t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"])
        stop, _, sfin, _, _ = bf16sim.forward(om, t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"], fp8=True)
    mr = lambda d: (d.abs().max().item(), d.pow(2).mean().sqrt().item())
    m = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=torch.bfloat16, dropout=0.0, fp8_forward=True)
    m.load_reference_state(sd)
    ids, seg = t["ids"].to(DEV), t["seg"].to(DEV)
    m.fp8_calibrate(ids, seg_ids=seg)
    out = m.predict(ids, seg_ids=seg, fp8=True)
    torch.cuda.synchronize()
    tag = "edge predict fp8 %s L=%d B=%d S=%d " % (family, L, B, S)
    _cmp_floor(tag + "top", out["top"], top, mr(stop - top), factor=SMALL_FACTOR)
    _cmp_floor(tag + "final", out["final"], final, mr(sfin - final), factor=SMALL_FACTOR)


# ---- 6. reproducible ---------------------------------------------------------------------------------------------------------------------
def test_fp8_predict_is_reproducible(labels):
    m, cfg, _ = _model(labels, dtype=torch.bfloat16, fp8=True)
    b = _batch(cfg, labels, 16, 64)
    m.fp8_calibrate(b["ids"], seg_ids=b["seg"])
    o1 = m.predict(b["ids"], seg_ids=b["seg"], fp8=True, return_logits=True)
    o2 = m.predict(b["ids"], seg_ids=b["seg"], fp8=True, return_logits=True)
    ob = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    for k in OUT_KEYS + ("logits",):
        assert torch.equal(o1[k], o2[k]), k
    assert not torch.equal(o1["cls"], ob["cls"]), "predict(fp8=True) returned the bits of the bf16 path: did the fp8 GEMMs run?"


# ---- 7. training state -----------------------------------------------------------------------------------------------------------------
def _train(m, b, opt, steps):
    for _ in range(steps):
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        opt.step()
    return out


def test_fp8_inference_leaves_training_state_alone(labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_infer in (False, True):
        m, cfg, _ = _model(labels, dtype=torch.bfloat16, fp8=True)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        _train(m, b, opt, 2)
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)
        torch.cuda.synchronize()
        assert m._aamax_valid and m._gamax_valid
        if with_infer:
            before = _state(m, opt)
            m.fp8_calibrate(b["ids"], seg_ids=b["seg"])
            m.fp8_calibrate(b["ids"][:3, :40].contiguous(), seg_ids=b["seg"][:3, :40].contiguous())
            m.predict(b["ids"], seg_ids=b["seg"], fp8=True)
            torch.cuda.synchronize()
            _same_state(before, _state(m, opt))
        opt.step()
        out = _train(m, b, opt, 1)
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone(), m.arena.aamax.clone(), m.arena.gamax.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after fp8_calibrate + predict(fp8=True) differs"


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_fp8_predict_refusals(labels):
    from nbest_amd import hipabi as hb
    m8, cfg, sd = _model(labels, dtype=torch.bfloat16, fp8=True)
    mb, _, _ = _model(labels, dtype=torch.bfloat16)
    b = _batch(cfg, labels, 2, 16)
    with pytest.raises(RuntimeError, match="fp8_calibrate"):
        m8.predict(b["ids"], seg_ids=b["seg"], fp8=True)
    with pytest.raises(RuntimeError, match="fp8_forward"):
        mb.predict(b["ids"], seg_ids=b["seg"], fp8=True)
    m8.fp8_calibrate(b["ids"], seg_ids=b["seg"])
    with pytest.raises(ValueError, match="return_attns"):
        m8.predict(b["ids"], seg_ids=b["seg"], fp8=True, return_attns=True)
    ones = [[1.0] * cfg.num_attention_heads for _ in range(cfg.num_hidden_layers)]
    for compact in (False, True):
        m8.set_head_mask(ones, compact=compact)
        with pytest.raises(RuntimeError, match="head mask"):
            m8.predict(b["ids"], seg_ids=b["seg"], fp8=True)
    m8.set_head_mask(None)
    assert m8.fp8_calibrated == 1
    m8.load_reference_state(sd)
    assert m8.fp8_calibrated == 0 and not bool(m8.arena.iamax.any())

    # the C entry point: the stated code, nothing enqueued - the cls buffer keeps its sentinel
    a = m8.arena
    d = m8._desc(2, 16, "refusal8").desc
    ids, seg, pos, mask = m8._inputs(b["ids"], b["seg"])
    d.w8, d.w8_inv_scale = a.w8.data_ptr(), a.w8_inv_scale.data_ptr()
    need = hb.lib().nbest_encoder_infer_fp8_ws_bytes(C.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    cls = torch.full((2, cfg.hidden_size), 7.0, dtype=torch.bfloat16, device=DEV)
    gate = torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads, device=DEV)

    def call(entry=None, n=need):
        f = entry or hb.lib().nbest_encoder_infer_fp8
        return f(C.byref(d), hb.ptr(a.weights), hb.ptr(a.p), hb.ptr(ids), hb.ptr(seg), hb.ptr(pos), hb.ptr(mask), hb.ptr(ws), n, hb.ptr(cls),
                 hb.stream_ptr())

    def calib():
        d.hidden_drop = d.attn_drop = 0.0
        d.w8, d.w8_inv_scale = a.w8.data_ptr(), a.w8_inv_scale.data_ptr()
        d.fp8_act, d.aamax_prev, d.aamax_new, d.head_gate = 0, None, a.iamax_slots.data_ptr(), None

    calib()
    d.hidden_drop = 0.1
    assert call() == -1 and "dropout" in hb.last_error()
    calib()
    d.w8 = None
    assert call() == -1
    calib()
    d.fp8_act, d.aamax_prev = 1, None
    assert call() == -1 and "aamax_prev" in hb.last_error()
    calib()
    d.aamax_new = None
    assert call() == -1 and "aamax_new" in hb.last_error()
    calib()
    d.head_gate = gate.data_ptr()
    assert call() == -1 and "head_gate" in hb.last_error()
    calib()
    assert call(n=need - 1) == -6                                                    # NBEST_ERR_WORKSPACE
    assert call(hb.lib().nbest_encoder_infer, n=need) == -1 and "fp8" in hb.last_error()    # the bf16 entry point still refuses w8
    torch.cuda.synchronize()
    assert bool((cls == 7.0).all()), "a refused call wrote cls_out"
    assert not bool(a.iamax_slots.any()), "a refused call recorded an amax"
    assert call() == 0
    torch.cuda.synchronize()
    a.iamax_slots.zero_()


# ---- 9. command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_predict_fp8(tmp_path, capsys):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    common = lambda dt: ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
                         "--bert_dropout", "0.1", "--lr", "3e-5", "--bert_lr", "3e-5", "--batchSize", "16", "--max_epoch", "1",
                         "--experiment", exp, "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", dt,
                         "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "5", "--resume"]
    assert cli.main(common("fp8w")) == 0
    d8, db = cli.exp_dir(cli.parse_arguments(common("fp8w"))), cli.exp_dir(cli.parse_arguments(common("bf16")))
    if not os.path.exists(os.path.join(d8, "model.pt")):     # written on a new best valid F1 only: the epoch's weights are in last.pt
        torch.save(torch.load(os.path.join(d8, "last.pt"), weights_only=True)["model"], os.path.join(d8, "model.pt"))
    if db != d8:
        os.makedirs(db, exist_ok=True)
        shutil.copy(os.path.join(d8, "model.pt"), os.path.join(db, "model.pt"))
    src = str(root / "valid")
    lines = open(src).read().strip("\n").split("\n")
    outs = {}
    capsys.readouterr()
    for tag, argv in (("fp8", common("fp8w") + ["--predict_fp8", "--fp8_calib_batches", "2"]), ("fp8w", common("fp8w")), ("bf16", common("bf16"))):
        path = str(tmp_path / (tag + ".pred"))
        assert cli.main(argv + ["--predict", src, "--predict_output", path]) == 0
        outs[tag] = (open(path, "rb").read(), capsys.readouterr().out)
    got = outs["fp8"][0].decode().split("\n")[:-1]
    assert len(got) == len(lines)
    for g, l in zip(got, lines):
        f = g.split("\t<=>\t")
        assert len(f) == 2 and f[0] == l.split("\t<=>\t")[0], (g, l)
    cal = [l for l in outs["fp8"][1].split("\n") if l.startswith("fp8 calibration:")]
    assert len(cal) == 1 and "2 batches, 24 utterances" in cal[0] and all(k in cal[0] for k in ("x ", "ctx ", "x1 ", "gelu ")), outs["fp8"][1]
    assert "fp8 calibration" not in outs["fp8w"][1]
    assert outs["fp8w"][0] == outs["bf16"][0], "--dtype fp8w --predict without --predict_fp8 is no longer the bf16 path"
