"""GPU: attention probabilities as an output - nbest_attention_probs / nbest_attention_cls_probs against fp64 torch and against
what the forward computed, the model's return_attns 6-tuple against the oracle's softmax, predict(return_attns=True) against the
eval forward, the refusals, and --predict_attention end to end."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, case_inputs, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rnd(*shape, dtype=torch.float32, s=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * s).to(dtype).to(DEV)


def _mask(B, S, seed):
    """row 0 the shortest, the others ragged, the last utterance fully masked (B >= 3)"""
    g = np.random.default_rng(seed)
    m = np.zeros((B, S), dtype=np.uint8)
    n0 = max(1, S // 3)
    m[0, :n0] = 1
    for b in range(1, B - 1):
        m[b, :int(g.integers(n0, S + 1))] = 1
    if S > 4:
        m[1, 2] = 0                               # a hole inside a row
    return torch.from_numpy(m).to(DEV)


def _ref64(qkv, mask, lse, B, S, heads):
    """fp64 exp(scale q.k - lse) on unmasked keys from the same stored Q, K and LSE"""
    H = heads * 64
    x = qkv.double().view(B, S, 3, heads, 64)
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)          # [B, h, S, 64]
    s = torch.matmul(q, k.transpose(-1, -2)) / 8.0
    p = torch.exp(s - lse.double()[..., None])
    return torch.where(mask.bool()[:, None, None, :], p, torch.zeros_like(p)), x[:, :, 2].transpose(1, 2)


SEQ = [1, 7, 64, 96, 128, 200, 256, 384, 512]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", SEQ)
def test_attention_probs_against_fp64(S, dtype):
    """Bounds.  fp32 (values s = 0.5): a score is one fp32 fma chain of 64 products; the partial sums stay below ~4, so each
    rounding is < 2.4e-7 and the chain's error, random-walk over 64 steps and times scale 1/8, stays near 1e-7 - times p <= 1, plus
    expf's ~1 ulp: 1e-6 absolute.  bf16 (s = 1): bf16 x bf16 products are exact in fp32, the MFMA accumulates in fp32 in its own
    order (partial sums ~30: < 2e-6 per rounding, ~2e-6 in the scaled score) - 1e-4 absolute is the issue's bar with a wide
    margin.  Masked keys exactly 0, a fully masked utterance all 0, rows sum to 1, two runs bit-equal, every element written.
    Tie to the forward: probs @ V in fp64 reproduces the forward's ctx - fp32 within 1e-5 x max|V| (the same probabilities up to
    the fp32 rounding above), bf16 within 2^-7 x max|V| (the forward rounds P to bf16, 2^-9 relative, then ctx to bf16)."""
    from nbest_amd import hipabi as hb
    f32 = dtype == torch.float32
    B, heads = 4, 2
    H = heads * 64
    qkv = _rnd(B * S, 3 * H, dtype=dtype, s=0.5 if f32 else 1.0, seed=S)
    mask = _mask(B, S, S)
    ctx, lse = hb.attention_fwd(qkv, mask, B, S, heads)
    out = torch.full((B, heads, S, S), float("nan"), device=DEV)
    got = hb.attention_probs(qkv, mask, lse, B, S, heads, out=out)
    again = hb.attention_probs(qkv, mask, lse, B, S, heads)
    torch.cuda.synchronize()
    assert not torch.isnan(got).any(), "an element of the output was not written"
    assert torch.equal(got, again), "two runs differ"
    ref, v = _ref64(qkv, mask, lse, B, S, heads)
    keys = mask.bool()[:, None, None, :].expand(B, heads, S, S)
    assert (got[~keys] == 0).all(), "a masked key has a non-zero probability"
    assert (got[B - 1] == 0).all(), "the fully masked utterance is not all 0"
    live = slice(0, B - 1)
    err = (got[live].double() - ref[live]).abs().max().item()
    bar = 1e-6 if f32 else 1e-4
    assert err <= bar, "S=%d %s: |P - fp64| %.3e > %.1e" % (S, dtype, err, bar)
    rows = got[live].double().sum(-1)
    assert (rows - 1).abs().max().item() <= 1e-5, "rows do not sum to 1"
    o = torch.matmul(got[live].double(), v[live])                          # [B-1, h, S, 64]
    c = ctx.view(B, S, heads, 64)[live].transpose(1, 2).double()
    vmax = v[live].abs().max().item()
    e2 = (o - c).abs().max().item()
    bar2 = (1e-5 if f32 else 2.0 ** -7) * vmax
    assert e2 <= bar2, "S=%d %s: |P V - ctx| %.3e > %.3e" % (S, dtype, e2, bar2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", SEQ)
def test_cls_probs_equal_row0(S, dtype):
    """nbest_attention_cls_probs normalises its own row (sequential fp32 fma scores, its own max and sum) where
    nbest_attention_probs uses the forward's LSE: the two agree to fp32 rounding - 2e-6 (fp32 values s = 0.5) and 1e-5 (bf16
    values s = 1: a different summation order of exact products, then exp2 / log-sum in log2 units for S <= 256)"""
    from nbest_amd import hipabi as hb
    f32 = dtype == torch.float32
    B, heads = 4, 3
    H = heads * 64
    qkv = _rnd(B * S, 3 * H, dtype=dtype, s=0.5 if f32 else 1.0, seed=100 + S)
    mask = _mask(B, S, S + 1)
    _, lse = hb.attention_fwd(qkv, mask, B, S, heads)
    full = hb.attention_probs(qkv, mask, lse, B, S, heads)
    cls = hb.attention_cls_probs(qkv, S * 3 * H, qkv[:, H:], 3 * H, mask, B, S, heads)
    torch.cuda.synchronize()
    assert not torch.isnan(cls).any()
    assert (cls[B - 1] == 0).all() and (cls[~mask.bool()[:, None, :].expand(B, heads, S)] == 0).all()
    err = (cls - full[:, :, 0, :]).abs().max().item()
    bar = 2e-6 if f32 else 1e-5
    assert err <= bar, "S=%d %s: |cls - row 0| %.3e > %.1e" % (S, dtype, err, bar)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _build(name, labels, dtype):
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    meta, _ = load_case(name)
    cfg, sd, batch = case_inputs(meta, labels)
    fp8 = dtype == "fp8w"
    m = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=torch.bfloat16 if fp8 else dtype, dropout=0.0, seed=1, fp8_forward=fp8)
    m.load_reference_state(sd)
    m.eval()
    b = {k: torch.from_numpy(v).to(DEV) for k, v in batch.items()}
    return m, cfg, sd, meta, b


def _oracle_probs(cfg, sd, ids, seg, family):
    """the oracle encoder's softmax probabilities, captured by wrapping torch.softmax around its forward (fp32, CPU)"""
    from oracle.encoder import EncoderConfig, OracleEncoder
    ocfg = EncoderConfig(**{k: v for k, v in cfg.to_dict().items() if k in EncoderConfig.__dataclass_fields__})
    enc = OracleEncoder(ocfg)
    pre = "bert_encoder."
    enc.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)})
    enc.eval()
    got, real = [], torch.softmax

    def spy(x, *a, **kw):
        y = real(x, *a, **kw)
        got.append(y.detach().clone())
        return y

    ids_c = ids.cpu()
    torch.softmax = spy
    try:
        with torch.no_grad():
            if family == "xlm-roberta":
                enc(input_ids=ids_c, attention_mask=ids_c > 0)
            else:
                enc(input_ids=ids_c, attention_mask=ids_c > 0, token_type_ids=seg.cpu())
    finally:
        torch.softmax = real
    return got


def _scores_equal(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), "top / final differ"
    assert a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1]), "bottoms differ"


@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_eval_forward_attns_match_oracle(name, labels):
    m, cfg, sd, meta, b = _build(name, labels, torch.float32)
    seg = b["seg"] if meta["seg"] else None
    opt = type("O", (), {})()
    plain = m(opt, b["ids"], b["tids"], seg_ids=seg, trans_seg_ids=b.get("tseg"))
    six = m(opt, b["ids"], b["tids"], seg_ids=seg, trans_seg_ids=b.get("tseg"), return_attns=True)
    torch.cuda.synchronize()
    assert len(plain) == 5 and len(six) == 6
    top, bott, fin, attns, asr_cls, trans_cls = six
    _scores_equal(plain, six)
    assert torch.equal(plain[3], asr_cls) and torch.equal(plain[4], trans_cls)
    B, S, heads = b["ids"].shape[0], b["ids"].shape[1], cfg.num_attention_heads
    assert isinstance(attns, tuple) and len(attns) == cfg.num_hidden_layers
    ref = _oracle_probs(cfg, sd, b["ids"], seg, cfg.family)
    assert len(ref) == cfg.num_hidden_layers
    for l, (a, r) in enumerate(zip(attns, ref)):
        assert a.dtype == torch.float32 and a.shape == (B, heads, S, S)
        ok = torch.isfinite(r)
        err = (a.cpu()[ok] - r[ok]).abs().max().item()
        assert err <= 1e-5, "%s layer %d: |attns - oracle softmax| %.3e" % (name, l, err)


@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_fp8w_attns_after_calibration(name, labels):
    """fp8w: qkv and lse are stashed in bf16 / fp32 in the calibration pass and in the fp8 passes after it.  The scores of a
    return_attns forward are the bits of the same forward without it (two models, the same call sequence); the maps are
    probabilities (masked keys 0, rows sum to 1) close to the bf16 model's (0.05: the fp8 GEMMs perturb qkv by a few %)"""
    m1, cfg, _, meta, b = _build(name, labels, "fp8w")
    m2, _, _, _, _ = _build(name, labels, "fp8w")
    mb, _, _, _, _ = _build(name, labels, torch.bfloat16)
    seg = b["seg"] if meta["seg"] else None
    opt = type("O", (), {})()
    cal = m1(opt, b["ids"], seg_ids=seg, return_attns=True)               # calibration pass: bf16 GEMMs, maps from its stash
    m2(opt, b["ids"], seg_ids=seg)
    assert m1._aamax_valid and m2._aamax_valid
    six = m1(opt, b["ids"], seg_ids=seg, return_attns=True)
    five = m2(opt, b["ids"], seg_ids=seg)
    ref = mb(opt, b["ids"], seg_ids=seg, return_attns=True)[3]
    torch.cuda.synchronize()
    _scores_equal(five, six)
    mask = (b["ids"] > 0)[:, None, None, :]
    for attns in (cal[3], six[3]):
        for a, r in zip(attns, ref):
            assert (a.masked_select(~mask.expand_as(a)) == 0).all()
            assert (a.double().sum(-1) - 1).abs().max().item() <= 1e-5
            assert (a - r).abs().max().item() <= 0.05


def test_predict_cls_attn_matches_eval_forward(labels):
    """cls_attn[l] = row 0 of the eval forward's attns[l].  Layers 0 .. L-2 see the same qkv bits: fp32 rounding of the two
    normalisations (2e-6 fp32, 1e-5 bf16).  The last layer projects the CLS-row Q and K|V in GEMMs of their own: within
    test_predict_agrees_with_eval_forward's bar for the outputs (1e-5 fp32, 2^-7 bf16).  Every other output of predict is the
    same bits with and without return_attns; nbest_encoder_infer's cls_out equals nbest_encoder_infer_attn's."""
    from nbest_amd import hipabi as hb
    for name in ("bert_L2", "xlmr_L2"):
        for dtype in (torch.float32, torch.bfloat16):
            f32 = dtype == torch.float32
            m, cfg, _, meta, b = _build(name, labels, dtype)
            seg = b["seg"] if meta["seg"] else None
            attns = m(type("O", (), {})(), b["ids"], seg_ids=seg, return_attns=True)[3]
            p0 = m.predict(b["ids"], seg_ids=seg)
            p1 = m.predict(b["ids"], seg_ids=seg, return_attns=True)
            torch.cuda.synchronize()
            assert set(p1) == set(p0) | {"cls_attn"}
            for k in p0:
                assert torch.equal(p0[k], p1[k]), "%s %s: predict %s differs with return_attns" % (name, dtype, k)
            L, B, S = cfg.num_hidden_layers, b["ids"].shape[0], b["ids"].shape[1]
            ca = p1["cls_attn"]
            assert ca.shape == (L, B, cfg.num_attention_heads, S) and ca.dtype == torch.float32
            for l in range(L):
                err = (ca[l] - attns[l][:, :, 0, :]).abs().max().item()
                bar = (2e-6 if f32 else 1e-5) if l + 1 < L else (1e-5 if f32 else 2.0 ** -7)
                assert err <= bar, "%s %s layer %d: |cls_attn - attns row 0| %.3e > %.1e" % (name, dtype, l, err, bar)
            assert (ca.double().sum(-1) - 1).abs().max().item() <= 1e-5


def test_refusals(labels):
    from nbest_amd import hipabi as hb
    m, cfg, _, meta, b = _build("bert_L2", labels, torch.float32)
    m.train()
    with pytest.raises(RuntimeError, match="eval / predict"):
        m(type("O", (), {})(), b["ids"], seg_ids=b["seg"], return_attns=True)
    m.eval()
    B, S = b["ids"].shape
    ps = m._desc(B, S, 0, first_trainable=1)
    act = torch.empty(ps.act_bytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="first_trainable"):
        hb.encoder_act_view(ps.desc, act, 0)
    q, l = hb.encoder_act_view(ps.desc, act, 1)
    assert act.data_ptr() <= q < act.data_ptr() + act.numel() and act.data_ptr() <= l < act.data_ptr() + act.numel()
    S2, heads = 513, 1
    qkv = torch.zeros(S2, 3 * 64, dtype=torch.bfloat16, device=DEV)
    mask = torch.ones(1, S2, dtype=torch.uint8, device=DEV)
    lse = torch.zeros(1, heads, S2, device=DEV)
    with pytest.raises(RuntimeError, match="512"):
        hb.attention_probs(qkv, mask, lse, 1, S2, heads, out=torch.empty(1, device=DEV))
    with pytest.raises(RuntimeError, match="512"):
        hb.attention_cls_probs(qkv, S2 * 192, qkv[:, 64:], 192, mask, 1, S2, heads, out=torch.empty(1, 1, 1, device=DEV))
    torch.cuda.synchronize()


def test_cli_predict_attention(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    common = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
              "--bert_dropout", "0.1", "--lr", "3e-5", "--bert_lr", "3e-5", "--batchSize", "8", "--max_epoch", "1", "--experiment", exp,
              "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
              "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "3", "--resume"]
    assert cli.main(common) == 0
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    plain, with_attn, attn = str(tmp_path / "a.pred"), str(tmp_path / "b.pred"), str(tmp_path / "b.attn.jsonl")
    assert cli.main(common + ["--predict", src, "--predict_output", plain]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", with_attn, "--predict_attention", attn]) == 0
    assert open(plain, "rb").read() == open(with_attn, "rb").read(), ".pred differs with --predict_attention"
    n_in = len(open(src).read().strip("\n").split("\n"))
    recs = [json.loads(l) for l in open(attn).read().strip("\n").split("\n")]
    assert [r["line"] for r in recs] == list(range(1, n_in + 1))
    for r in recs:
        assert r["segments"][:2] == ["cls", "sys"] and 1 <= len(r["segments"]) - 2 <= 3
        assert len(r["tokens"]) == len(r["segments"]) and len(r["mass"]) == 2
        for row in r["mass"]:
            assert len(row) == len(r["segments"]) and abs(sum(row) - 1.0) < 1e-4
