"""GPU: attention rollout - nbest_attention_rollout_step against fp64 arithmetic on nbest_attention_probs' own output, its
refusals, model.attention_rollout against trainer.rollout_reference of the eval forward's maps (fp32, bf16, fp8w), the training
state it must leave alone, the model's refusals and --predict_rollout end to end."""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_attn_probs_gpu import _build, _rnd
from test_head_gate_cpu import mixed_mask
from test_infer_gpu import _batch, _model, _same_state, _state

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG = os.environ.get("NBEST_ROLLOUT_PARITY_LOG")     # a file that receives one line per measured figure (profiles/rollout_parity.txt)
GUARD = 64          # floats on either side of r_out
REL = 1e-4          # |got - expected| <= REL x max_j expected[b]: fp32 summation of <= S heads <= 1536 non-negative terms, (n - 1) 2^-24


def _log(msg):
    if LOG:
        with open(LOG, "a") as f:
            f.write(msg + "\n")


def _key_mask(B, S, trailing_only=False):
    """ragged rows (at least a third of the keys), a hole inside one of them, the last utterance fully masked when B >= 3;
    ``trailing_only``: no hole"""
    g = np.random.default_rng(1000 * B + S)
    m = np.zeros((B, S), dtype=np.uint8)
    for b in range(B):
        m[b, :int(g.integers(max(1, S // 3), S + 1))] = 1
    if S > 4 and not trailing_only:
        m[min(1, B - 1), 2] = 0
    if B >= 3:
        m[B - 1] = 0
    return torch.from_numpy(m).to(DEV)


def _row_vectors(B, S):
    """random, non-negative, about a fifth exact zeros, sum 1 per utterance"""
    g = torch.Generator(device="cpu").manual_seed(77 * B + S)
    r = torch.rand(B, S, generator=g, dtype=torch.float64) ** 2
    r[torch.rand(B, S, generator=g) < 0.2] = 0.0
    r[:, S // 2] += 0.25
    return (r / r.sum(-1, keepdim=True)).float().to(DEV)


@functools.lru_cache(maxsize=None)
def _problem(B, S, heads, f32, trailing_only=False):
    """inputs of one shape and what the expected value is made of: mix = mean_h (r_in @ P_h) in fp64, P from nbest_attention_probs"""
    from nbest_amd import hipabi as hb
    dtype = torch.float32 if f32 else torch.bfloat16
    qkv = _rnd(B * S, 3 * heads * 64, dtype=dtype, s=0.5 if f32 else 1.0, seed=S + 7 * heads)
    mask = _key_mask(B, S, trailing_only)
    _, lse = hb.attention_fwd(qkv, mask, B, S, heads)
    r_in = _row_vectors(B, S)
    P = hb.attention_probs(qkv, mask, lse, B, S, heads)
    mix = torch.einsum("bi,bhij->bj", r_in.double(), P.double()) / heads
    torch.cuda.synchronize()
    return qkv, mask, lse, r_in, mix


def _step(qkv, mask, lse, r_in, rho, B, S, heads):
    """the kernel into the middle of a NaN-filled buffer -> (r_out, the whole buffer)"""
    from nbest_amd import hipabi as hb
    buf = torch.full((B * S + 2 * GUARD,), float("nan"), device=DEV)
    out = buf[GUARD:GUARD + B * S].view(B, S)
    hb.attention_rollout_step(qkv, mask, lse, r_in, rho, B, S, heads, out=out)
    return out, buf


SHAPES = [(1, 1, 1), (3, 5, 2), (3, 64, 12), (3, 65, 3), (3, 128, 12), (2, 200, 4), (2, 512, 2)]


@pytest.mark.parametrize("rho", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_rollout_step_against_fp64(B, S, heads, dtype, rho):
    """expected = rho r_in + (1 - rho) mean_h (r_in @ P_h) in fp64 with P = nbest_attention_probs on the same inputs.  Both
    kernels form each probability the same way, so what remains is the fp32 summation of at most S heads <= 1536 non-negative
    terms, worst case (n - 1) 2^-24 ~ 9.2e-5 relative: |got - expected| <= 1e-4 max_j expected[b] per utterance (derived, not
    measured).  Exact: rho r_in on masked keys and on a fully masked utterance, r_in itself at rho = 1; two runs bit-equal; every
    element written, the guard bands on both sides untouched; under a trailing-only mask the row sums are kept within 2e-4.
    The shapes reach the three workgroup sizes of both kernels (4 / 8 / 16 waves: bf16 at heads x ceil(S / 16) < 32, < 64 and
    above; fp32 at heads x S < 128, < 256 and above), the element-wise store path (S % 4 != 0) and key blocks cut by S."""
    f32 = dtype == torch.float32
    qkv, mask, lse, r_in, mix = _problem(B, S, heads, f32)
    got, buf = _step(qkv, mask, lse, r_in, rho, B, S, heads)
    again, _ = _step(qkv, mask, lse, r_in, rho, B, S, heads)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + B * S:]).all(), "a guard band was written"
    assert not torch.isnan(got).any(), "an element of r_out was not written"
    assert torch.equal(got, again), "two runs differ"
    want = rho * r_in.double() + (1.0 - rho) * mix
    top = want.max(dim=-1).values
    err = (got.double() - want).abs().max(dim=-1).values
    ratio = max((e / t if t > 0 else (0.0 if e == 0 else float("inf"))) for e, t in zip(err.tolist(), top.tolist()))
    print("rollout_step %s B=%d S=%d heads=%d rho=%.1f: max |got - fp64| / max expected = %.3e" % ("f32" if f32 else "bf16", B, S, heads, rho, ratio))
    _log("rollout_step %-4s B=%d S=%-3d heads=%-2d rho=%.1f  err/max_expected=%.3e bound=%.1e %s"
         % ("f32" if f32 else "bf16", B, S, heads, rho, ratio, REL, "OK" if ratio <= REL else "FAIL"))
    assert (err <= REL * top).all(), "B=%d S=%d heads=%d %s rho=%g: |got - fp64| / max expected %.3e > %.1e" % (B, S, heads, dtype, rho, ratio, REL)
    exact = torch.tensor(rho, dtype=torch.float32, device=DEV) * r_in           # the fp32 product rho r_in
    dead = ~mask.bool()
    assert torch.equal(got[dead], exact[dead]), "a masked key holds more than rho r_in"
    if B >= 3:
        assert torch.equal(got[B - 1], exact[B - 1]), "the fully masked utterance is not rho r_in"
    if rho == 1.0:
        assert torch.equal(got.view(torch.int32), r_in.view(torch.int32)), "rho = 1: r_out is not r_in bit for bit"
    # row sums under a mask that covers only trailing positions
    qkv, mask, lse, r_in, _ = _problem(B, S, heads, f32, True)
    got, _ = _step(qkv, mask, lse, r_in, rho, B, S, heads)
    torch.cuda.synchronize()
    live = mask.bool().any(-1)
    d = (got.double().sum(-1) - r_in.double().sum(-1)).abs()[live]
    assert d.numel() > 0 and d.max().item() <= 2e-4, "the row sums moved by %.3e" % d.max().item()


def test_rollout_step_refusals():
    """each refusal returns its code, sets nbest_last_error and leaves a sentinel-filled r_out as it was"""
    from nbest_amd import hipabi as hb
    L = hb.lib()
    B, S, heads = 2, 24, 2
    qkv = _rnd(B * S + 1, 3 * heads * 64, dtype=torch.bfloat16, seed=1)
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    lse = torch.zeros(B, heads, 600, device=DEV)
    r_in = torch.full((B, 600), 0.25, device=DEV)
    r_out = torch.full((B, 600), -7.0, device=DEV)
    ARG, SHAPE, DTYPE, ALIGN = -1, -2, -3, -4
    p = lambda t: C.c_void_p(t.data_ptr())
    nul = C.c_void_p(0)
    good = dict(qkv=p(qkv), mask=p(mask), lse=p(lse), r_in=p(r_in), r_out=p(r_out), rho=0.5, B=B, S=S, heads=heads, d=64, dtype=hb.BF16)

    def call(**kw):
        a = dict(good, **kw)
        return L.nbest_attention_rollout_step(a["qkv"], a["mask"], a["lse"], a["r_in"], a["r_out"], a["rho"], a["B"], a["S"], a["heads"],
                                              a["d"], a["dtype"], hb.stream_ptr())

    cases = [(dict(qkv=nul), ARG), (dict(mask=nul), ARG), (dict(lse=nul), ARG), (dict(r_in=nul), ARG), (dict(r_out=nul), ARG),
             (dict(r_in=p(r_out)), ARG), (dict(d=32), SHAPE), (dict(d=128), SHAPE), (dict(S=0), SHAPE), (dict(S=513), SHAPE),
             (dict(dtype=2), DTYPE), (dict(dtype=-1), DTYPE), (dict(qkv=C.c_void_p(qkv.data_ptr() + 2)), ALIGN),
             (dict(qkv=C.c_void_p(qkv.data_ptr() + 8)), ALIGN), (dict(rho=-0.1), ARG), (dict(rho=1.5), ARG), (dict(rho=float("nan")), ARG),
             (dict(rho=float("inf")), ARG)]
    for kw, code in cases:
        rc = call(**kw)
        assert rc == code, "%s: returned %d, not %d" % (kw, rc, code)
        assert "attention_rollout_step" in hb.last_error(), "%s: nbest_last_error says %r" % (kw, hb.last_error())
    torch.cuda.synchronize()
    assert bool((r_out == -7.0).all()), "a refused call wrote r_out"
    assert call() == 0                                         # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((r_out.view(-1)[:B * S] != -7.0).all()) and bool((r_out.view(-1)[B * S:] == -7.0).all())
    with pytest.raises(RuntimeError, match="residual"):
        hb.attention_rollout_step(qkv, mask, lse, r_in, 2.0, B, S, heads, out=r_out)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _check_against_maps(tag, lay, attns, rho, mask):
    """every layer of ``lay`` [L, B, S] against rollout_reference of the maps, with test 1's bound times the layers applied so far"""
    from nbest_amd import trainer
    ref = trainer.rollout_reference(attns, rho)
    L = len(attns)
    assert lay.shape == ref.shape and lay.dtype == torch.float32
    for l in range(L):
        n = L - l
        top = ref[l].max(dim=-1).values
        err = (lay[l].double() - ref[l]).abs().max(dim=-1).values
        ratio = (err / top).max().item()
        print("%s layer %d (%d applied): max |got - reference| / max reference = %.3e" % (tag, l, n, ratio))
        _log("%-40s layer %d applied %d  err/max_ref=%.3e bound=%.1e %s" % (tag, l, n, ratio, n * REL, "OK" if ratio <= n * REL else "FAIL"))
        assert (err <= n * REL * top).all(), "%s layer %d: |got - reference| / max reference %.3e > %.1e" % (tag, l, ratio, n * REL)
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["bert_L2", "bert_L2_noseg", "xlmr_L2"])
def test_model_rollout_against_maps(name, dtype, labels):
    m, cfg, _, meta, b = _build(name, labels, dtype)
    seg = b["seg"] if meta["seg"] else None
    rho = 0.5
    top, bott, fin, attns, _, _ = m(type("O", (), {})(), b["ids"], seg_ids=seg, return_attns=True)
    out = m.attention_rollout(b["ids"], seg_ids=seg, residual=rho)
    torch.cuda.synchronize()
    assert set(out) == {"top", "bott", "final", "pred", "rollout", "layers"}
    L, (B, S) = cfg.num_hidden_layers, b["ids"].shape
    lay = out["layers"]
    assert lay.shape == (L, B, S) and out["rollout"].shape == (B, S) and out["rollout"].dtype == torch.float32
    assert torch.equal(out["rollout"], lay[0])
    mask = b["ids"] > 0
    _check_against_maps("%s %s" % (name, "f32" if dtype == torch.float32 else "bf16"), lay, attns, rho, mask)
    assert torch.equal(out["top"], top) and torch.equal(out["final"], fin), "top / final are not the eval forward's"
    assert all(torch.equal(v, m._bottoms_dict(out["bott"])[k]) for k, v in bott.items()), "bott is not the eval forward's"
    assert torch.equal(out["pred"], m.decode(out["top"], out["bott"])), "pred is not decode of the scores"
    if cfg.family == "bert":
        assert bool((lay[:, ~mask] == 0).all()), "mass on a masked key"
        assert (lay.double().sum(-1) - 1).abs().max().item() <= 2e-4, "rows do not sum to 1"
    last = rho * torch.eye(S, device=DEV)[0] + (1 - rho) * attns[-1].mean(1)[:, 0]
    assert (out["rollout"] - last).abs().max().item() > 1e-3, "the rollout is the last layer's CLS attention: the product is a no-op"
    # no dropout, whatever model.training says (the golden configurations carry no dropout: give this model some)
    m.cfg.hidden_dropout_prob = m.cfg.attention_probs_dropout_prob = 0.1
    m.dropout = 0.3
    m.train()
    tr = m.attention_rollout(b["ids"], seg_ids=seg, residual=rho)
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], tr[k]), "%s differs under model.train(): dropout was applied" % k


@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_fp8w_rollout_after_a_training_step(name, labels):
    """an fp8w model after one training step (its calibration pass): the rollout agrees with rollout_reference of its own
    return_attns maps - two models in the same state, one asked for the maps and one for the rollout, as the eval forward moves the
    activation amax history on"""
    from nbest_amd.optim import HipBertAdam
    ms = []
    for _ in range(2):
        m, cfg, _, meta, b = _build(name, labels, "fp8w")
        seg = b["seg"] if meta["seg"] else None
        m.train()
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        m.forward_backward(b["ids"], b["labels"], seg_ids=seg)
        opt.step()
        m.eval()
        ms.append(m)
    assert ms[0]._aamax_valid and ms[1]._aamax_valid
    top, bott, fin, attns, _, _ = ms[0](type("O", (), {})(), b["ids"], seg_ids=seg, return_attns=True)
    out = ms[1].attention_rollout(b["ids"], seg_ids=seg, residual=0.5)
    torch.cuda.synchronize()
    assert torch.equal(out["top"], top) and torch.equal(out["final"], fin)
    _check_against_maps("%s fp8w" % name, out["layers"], attns, 0.5, b["ids"] > 0)
    assert torch.equal(out["rollout"], out["layers"][0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_step_after_rollout_is_unchanged(dtype, labels):
    from nbest_amd.optim import HipBertAdam
    res = []
    for with_ro in (False, True):
        m, cfg, _ = _model(labels, dtype=dtype)
        m.train()
        b = _batch(cfg, labels, 4, 48)
        opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
        if with_ro:
            g0, step0 = m.arena.g.clone(), m.step_counter
            m.attention_rollout(b["ids"], seg_ids=b["seg"], residual=0.3)
            assert torch.equal(m.arena.g, g0) and m.step_counter == step0
        out = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"],
                                 add_l2_loss=True)
        opt.step()
        torch.cuda.synchronize()
        res.append((out["loss_parts"].clone(), m.arena.p.clone(), m.arena.m.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), "a training step after attention_rollout() differs"


def test_model_refusals(labels):
    """a gated mask, a compact mask, a residual outside [0, 1] or NaN, an S beyond the position table: each raises, nothing is
    enqueued (stashes, gradients and counters keep their bits), and a plain predict afterwards is what it was"""
    m, cfg, _ = _model(labels, dtype=torch.bfloat16)
    m.eval()
    b = _batch(cfg, labels, 3, 40)
    base = {k: v.clone() for k, v in m.predict(b["ids"], seg_ids=b["seg"]).items()}
    m.attention_rollout(b["ids"], seg_ids=b["seg"])               # the stash exists and holds this pass
    torch.cuda.synchronize()
    before = _state(m)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    for kw in (dict(), dict(compact=True)):
        m.set_head_mask(mask, **kw)
        with pytest.raises(RuntimeError, match="not built"):
            m.attention_rollout(b["ids"], seg_ids=b["seg"])
        m.set_head_mask(None)
    for rho in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="residual"):
            m.attention_rollout(b["ids"], seg_ids=b["seg"], residual=rho)
    with pytest.raises(RuntimeError, match="position table"):
        m.attention_rollout(torch.ones(1, 513, dtype=b["ids"].dtype, device=DEV))
    torch.cuda.synchronize()
    _same_state(before, _state(m))
    after = m.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    for k in base:
        assert torch.equal(base[k], after[k]), "predict %s changed" % k


def test_cli_predict_rollout(tmp_path):
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
    assert cli.main(common) == 0                               # a small random-weight model after one epoch on the 8 lines
    d = cli.exp_dir(cli.parse_arguments(common))
    if not os.path.exists(os.path.join(d, "model.pt")):
        torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
    src = str(root / "valid")
    plain, with_ro, ro = str(tmp_path / "a.pred"), str(tmp_path / "b.pred"), str(tmp_path / "b.rollout.jsonl")
    both, ro2, attn = str(tmp_path / "c.pred"), str(tmp_path / "c.rollout.jsonl"), str(tmp_path / "c.attn.jsonl")
    assert cli.main(common + ["--predict", src, "--predict_output", plain]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", with_ro, "--predict_rollout", ro, "--rollout_residual", "0.25"]) == 0
    assert cli.main(common + ["--predict", src, "--predict_output", both, "--predict_rollout", ro2, "--predict_attention", attn]) == 0
    assert open(plain, "rb").read() == open(with_ro, "rb").read() == open(both, "rb").read(), ".pred differs with --predict_rollout"
    n_in = len(open(src).read().strip("\n").split("\n"))
    recs = [json.loads(l) for l in open(ro).read().strip("\n").split("\n")]
    recs2 = [json.loads(l) for l in open(ro2).read().strip("\n").split("\n")]
    arecs = [json.loads(l) for l in open(attn).read().strip("\n").split("\n")]
    assert [r["line"] for r in recs] == [r["line"] for r in recs2] == [r["line"] for r in arecs] == list(range(1, n_in + 1))
    for r, r2, a in zip(recs, recs2, arecs):
        assert set(r) == {"line", "segments", "tokens", "residual", "mass", "token_rollout"}
        assert r["residual"] == 0.25 and r2["residual"] == 0.5
        assert r["segments"] == r2["segments"] == a["segments"] and r["tokens"] == r2["tokens"] == a["tokens"]
        for x in (r, r2):
            assert len(x["mass"]) == len(x["segments"]) and abs(sum(x["mass"]) - 1.0) < 1e-5
            assert len(x["token_rollout"]) == sum(x["tokens"]) and min(x["token_rollout"]) >= 0
        assert r["token_rollout"] != r2["token_rollout"], "the residual has no effect"
