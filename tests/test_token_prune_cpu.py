"""CPU: token pruning for predict - the ABI of the new entry points, trainer.token_keep_schedule, the --token_keep parser and the
command line's refusals, predict's refusals that need no device, trainer.token_prune_reference against a second statement of the
selection order, the --predict_tokens record, and the input checks of the end-to-end GPU test (test_token_prune_gpu.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import token_prune_ref as R

import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi as hb, trainer

NAN, INF = float("nan"), float("inf")


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_token_prune_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "nbest_hip.h")).read()
    want = {
        "nbest_token_select": ["score", "key_mask", "origin_in", "k", "idx_out", "mask_out", "maskf_out", "origin_out", "B", "S", "stream"],
        "nbest_rows_compact": ["src", "idx", "dst", "B", "S", "k", "H", "dtype", "stream"],
        "nbest_encoder_infer_tokens": ["d", "wts", "prm", "ids", "seg", "pos", "key_mask", "ws", "ws_bytes", "cls_out", "keep_host", "n_keep",
                                       "token_kept", "stream"],
        "nbest_encoder_infer_tokens_ws_bytes": ["d"],
    }
    assert os.path.exists(hb.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(hb.LIB_PATH)
    for name, names in want.items():
        m = re.search(r"(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/nbest_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names, name
        assert name in hb.EXPORTS, "%s is not in hipabi.EXPORTS" % name
        assert hasattr(lib, name), "libnbest_hip.so does not export %s" % name
    assert callable(hb.token_select) and callable(hb.rows_compact) and callable(hb.encoder_infer_tokens)
    mk = open(os.path.join(ROOT, "n-best-asr-transformer_amd", "csrc", "Makefile")).read()
    assert "token_prune.hip" in mk


def test_descriptor_is_unchanged():
    """the schedule is an argument: the descriptor gained no field for it"""
    assert not [n for n, _ in hb.EncoderDesc._fields_ if "token" in n or "keep" in n]


# ---- token_keep_schedule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,first,last", [(12, 128, 16), (12, 64, 64), (4, 96, 6), (24, 256, 32), (3, 5, 1), (12, 512, 1), (12, 3, 2)])
def test_schedule_properties(L, first, last):
    s = trainer.token_keep_schedule(L, first, last)
    assert len(s) == L - 1 and all(isinstance(x, int) for x in s)
    assert s[0] == first and s[-1] == last
    assert all(a >= b for a, b in zip(s, s[1:])), s
    assert all(last <= x <= first for x in s)
    if first == last:
        assert s == [first] * (L - 1)
    else:      # geometric: the ratios of neighbours agree up to the rounding of both (|error| <= 0.5 each)
        r = (last / first) ** (1.0 / (L - 2))
        for i, x in enumerate(s):
            assert abs(x - first * r ** i) <= 0.5 + 1e-9, (i, x, first * r ** i)


def test_schedule_edges():
    assert trainer.token_keep_schedule(1, 128, 16) == []
    assert trainer.token_keep_schedule(2, 128, 16) == [16]
    assert trainer.token_keep_schedule(3, 128, 16) == [128, 16]
    assert trainer.token_keep_schedule(5, 7, 7) == [7, 7, 7, 7]
    for bad in ((0, 8, 4), (4, 4, 8), (4, 8, 0), (4, 0, 0)):
        with pytest.raises(ValueError):
            trainer.token_keep_schedule(*bad)


def test_parse_token_keep():
    assert trainer.parse_token_keep("40,30,30", 4) == [40, 30, 30]
    assert trainer.parse_token_keep("128:16", 12) == trainer.token_keep_schedule(12, 128, 16)
    assert trainer.parse_token_keep("7", 2) == [7]
    assert trainer.parse_token_keep("", 1) == [] and trainer.parse_token_keep("9:3", 1) == []
    assert trainer.parse_token_keep("40,30", None) is None and trainer.parse_token_keep("128:16", None) is None
    for spec, L in (("40,30", 4), ("40,50,60", 4), ("40,0,0", 4), ("a,b", 3), ("16:128", 12), ("1:2:3", 12), ("4:0", 12), ("40,,30", 4),
                    ("-3", 2), ("40,30", 1)):
        with pytest.raises(ValueError):
            trainer.parse_token_keep(spec, L)
    for spec in ("40,50", "0", "x", "16:128", "8:"):       # what is wrong without knowing L
        with pytest.raises(ValueError):
            trainer.parse_token_keep(spec, None)


# ---- command line ------------------------------------------------------------------------------------------------------------------
FILE = os.path.join(GOLDEN, "valid_head.txt")
BASE = ["--dataset", "dstc2", "--dataroot", GOLDEN, "--deviceId", "0", "--experiment", "exp", "--label_space", os.path.join(GOLDEN, "label_space.json")]


def _refused(argv, capsys, word):
    with pytest.raises(SystemExit) as e:
        cli.parse_arguments(BASE + argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_cli_accepts_token_keep(tmp_path):
    out = str(tmp_path / "t.jsonl")
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--token_keep", "128:16"])
    assert opt.token_keep == "128:16" and opt.predict_tokens is None
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--token_keep", "40,30,30", "--predict_tokens", out])
    assert opt.token_keep == "40,30,30" and opt.predict_tokens == out
    opt = cli.parse_arguments(BASE + ["--predict", FILE])
    assert opt.token_keep is None and opt.predict_tokens is None


def test_cli_refusals(capsys, tmp_path):
    mask = tmp_path / "mask.json"
    mask.write_text("[[1]]")
    out = str(tmp_path / "x.jsonl")
    ok = ["--predict", FILE, "--token_keep", "40:10"]
    _refused(["--token_keep", "40:10"], capsys, "--predict FILE")                       # a training run
    _refused(["--testing", "--token_keep", "40:10"], capsys, "--testing")
    _refused(["--head_importance", out, "--token_keep", "40:10"], capsys, "--head_importance")
    _refused(["--predict", FILE, "--predict_tokens", out], capsys, "--token_keep")
    _refused(ok + ["--dtype", "fp8w", "--predict_fp8"], capsys, "--predict_fp8")
    _refused(ok + ["--head_mask", str(mask)], capsys, "--head_mask")
    _refused(ok + ["--head_mask", str(mask), "--compact_heads"], capsys, "--token_keep")
    _refused(ok + ["--predict_attention", out], capsys, "--predict_attention")
    _refused(ok + ["--predict_attribution", out], capsys, "--predict_attribution")
    _refused(ok + ["--predict_rollout", out], capsys, "--predict_rollout")
    for spec in ("10:40", "40,50", "0", "x,y", "1:2:3"):
        _refused(["--predict", FILE, "--token_keep", spec], capsys, "--token_keep")


# ---- predict's refusals that need no device ----------------------------------------------------------------------------------------
def test_predict_refuses_before_touching_the_device():
    """the argument checks come first: they raise on an object that has nothing but a configuration and a mask slot"""
    from nbest_amd.model import NBestSTCModel

    class Cfg:
        num_hidden_layers = 4

    m = object.__new__(NBestSTCModel)
    object.__setattr__(m, "cfg", Cfg())
    object.__setattr__(m, "_head_mask", None)
    ids = torch.ones(2, 8, dtype=torch.long)
    for keep in ([8, 4], [8, 4, 4, 2], []):
        with pytest.raises(ValueError, match="L - 1"):
            NBestSTCModel.predict(m, ids, token_keep=keep)
    with pytest.raises(ValueError, match=">= 1"):
        NBestSTCModel.predict(m, ids, token_keep=[8, 0, 0])
    with pytest.raises(ValueError, match="non-increasing"):
        NBestSTCModel.predict(m, ids, token_keep=[4, 8, 8])
    with pytest.raises(ValueError, match="return_attns"):
        NBestSTCModel.predict(m, ids, token_keep=[8, 4, 4], return_attns=True)
    with pytest.raises(ValueError, match="return_token_kept"):
        NBestSTCModel.predict(m, ids, return_token_kept=True)
    with pytest.raises(RuntimeError, match="fp8"):
        NBestSTCModel.predict(m, ids, token_keep=[8, 4, 4], fp8=True)
    object.__setattr__(m, "_head_mask", torch.ones(4, 12))
    with pytest.raises(RuntimeError, match="head mask"):
        NBestSTCModel.predict(m, ids, token_keep=[8, 4, 4])


# ---- the selection order -------------------------------------------------------------------------------------------------------------
HAND = [
    # (score, mask, k, expected)
    ([.1, .5, .5, .5, .2], [1, 1, 1, 1, 1], 3, [0, 1, 2]),                    # ties: the lower index
    ([.1, .5, .9, .5, .2], [1, 1, 1, 1, 1], 3, [0, 1, 2]),
    ([.1, .2, .9, .5, .5], [1, 1, 1, 1, 1], 3, [0, 2, 3]),
    ([.9, .1, .8, .7, .6], [1, 1, 0, 1, 1], 3, [0, 3, 4]),                    # a masked token in the middle loses to any real one
    ([.9, .1, .8, .7, .6], [1, 1, 0, 1, 1], 4, [0, 1, 3, 4]),
    ([.9, .1, .8, .7, .6], [1, 1, 0, 1, 1], 5, [0, 1, 2, 3, 4]),              # k = S
    ([.0, NAN, .1, NAN, -INF], [1, 1, 1, 1, 1], 3, [0, 2, 4]),                # a number (even -inf) before a NaN
    ([.0, NAN, .1, NAN, -INF], [1, 1, 1, 1, 1], 4, [0, 1, 2, 4]),             # then NaNs in index order
    ([NAN, .3, .1, INF, .2], [1, 1, 1, 1, 1], 2, [0, 3]),                     # position 0 whatever its score
    ([.0, .3, .1, .4, .2], [0, 1, 1, 1, 1], 1, [0]),                          # k = 1: position 0 alone, even masked
    ([.5, .4, .0, .0, .0], [1, 1, 0, 0, 0], 4, [0, 1, 2, 3]),                 # fewer real tokens than k: padding in index order
    ([.5, .4, .3, .9, .0], [1, 1, 0, 0, 0], 4, [0, 1, 2, 3]),                 # ... by score among the masked, were it not 0: 3 before 2
    ([.5, .4, .3, .9, .0], [1, 1, 0, 0, 0], 3, [0, 1, 3]),
    ([.1, -0.0, 0.0, -1.0, -1.0], [1, 1, 1, 1, 1], 2, [0, 1]),                # -0 ties with +0
    ([.1, NAN, .5, .2, .3], [1, 0, 0, 1, 1], 4, [0, 2, 3, 4]),                # masked number before masked NaN
]


@pytest.mark.parametrize("score,mask,k,want", HAND)
def test_reference_on_hand_built_rows(score, mask, k, want):
    sc = np.array([score, score], dtype=np.float64)
    mk = np.array([mask, mask], dtype=np.uint8)
    got = trainer.token_select_reference(sc, mk, k)
    assert got.shape == (2, k) and got.dtype == np.int64
    assert got[0].tolist() == got[1].tolist() == want
    assert R.select_by_sorting(score, mask, k) == want


def test_reference_against_sorting_on_random_rows():
    g = np.random.default_rng(5)
    for S in (1, 2, 5, 33, 130):
        sc = g.choice([0.0, 0.25, 0.5, 1.0, -1.0, NAN, INF, -INF], size=(6, S)).astype(np.float64) + (g.random((6, S)) < 0.5) * g.random((6, S))
        mk = (g.random((6, S)) < 0.7).astype(np.uint8)
        for k in sorted({1, (S + 1) // 2, max(1, S - 1), S}):
            got = trainer.token_select_reference(sc, mk, k)
            for b in range(6):
                assert got[b].tolist() == R.select_by_sorting(sc[b], mk[b], k), (S, k, b)
    with pytest.raises(ValueError):
        trainer.token_select_reference(np.zeros((1, 4)), np.ones((1, 4)), 5)
    with pytest.raises(ValueError):
        trainer.token_select_reference(np.zeros((1, 4)), np.ones((1, 4)), 0)


def test_prune_reference_score():
    """the score is the head mean of the column sums over the unmasked query rows"""
    g = torch.Generator().manual_seed(2)
    B, heads, S = 2, 3, 6
    a = torch.softmax(torch.randn(B, heads, S, S, generator=g, dtype=torch.float64), -1)
    mask = torch.tensor([[1, 1, 1, 0, 1, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.uint8)
    score, idx = trainer.token_prune_reference(a, mask, 3)
    assert score.dtype == np.float64 and score.shape == (B, S) and idx.shape == (B, 3)
    for b in range(B):
        want = sum(a[b, :, i, :] for i in range(S) if mask[b, i]).mean(0)
        assert np.abs(score[b] - want.numpy()).max() <= 1e-15
        assert idx[b].tolist() == R.select_by_sorting(score[b], mask[b].tolist(), 3)
    assert abs(score[1].sum() - S) <= 1e-12                # every unmasked query row sums to 1


def test_token_prune_record():
    spans = [("cls", 0, 1), ("sys", 1, 4), ("h1", 4, 7), ("h2", 7, 9)]
    kept = torch.tensor([[0, 1, 2, 4, 5, 7, 9, 10, -1, -1, -1, -1], [0, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1]], dtype=torch.int32)
    rec = trainer.token_prune_record(3, spans, kept)
    assert rec == {"line": 3, "segments": ["cls", "sys", "h1", "h2"], "tokens": [1, 3, 3, 2], "kept": [[1, 2, 2, 1], [1, 0, 1, 1]]}
    assert json.loads(json.dumps(rec)) == rec


# ---- the inputs of the end-to-end GPU test -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.E2E))
def test_e2e_inputs_separate_the_scores(name, labels):
    """The end-to-end GPU test accepts any kept set that is a top-k of the oracle's fp64 scores up to TOL of the utterance's largest
    score.  That says something only where the scores are apart at the cut - (a) at every eliminating layer and in every utterance
    that drops a real token, the last kept real token scores at least 100 TOL of the largest score above the first dropped one -
    and where the selection is not the trivial one: (b) at every eliminating layer the kept set differs from "the first k positions"
    in at least half of the utterances.  The schedule has at least three eliminating layers, and real tokens are dropped."""
    keep = R.E2E[name]
    om, meta, b = R.oracle_model(name, labels)
    assert len(keep) == meta["L"] - 1 and all(x >= y for x, y in zip(keep, keep[1:]))
    out = R.oracle_pruned(om, b["ids"], b["seg"] if meta["seg"] else None, keep)
    cnt = R.counts(meta["S"], keep)
    elim = [l for l in range(meta["L"] - 1) if cnt[l + 1] < cnt[l]]
    assert len(elim) >= 3 and sorted(out["scores"]) == elim
    B = b["ids"].shape[0]
    dropped_real = 0
    for l in elim:
        score, org, mask = out["scores"][l]
        kept = out["kept"][l]
        assert kept.shape == (B, cnt[l + 1]) and (kept[:, 0] == 0).all()
        differ = 0
        for u in range(B):
            here = set(kept[u].tolist())
            cur = [j for j in range(cnt[l]) if int(org[u, j]) in here]
            differ += cur != list(range(cnt[l + 1]))
            real = [j for j in range(1, cnt[l]) if mask[u, j]]
            ks = [float(score[u, j]) for j in real if j in cur]
            ds = [float(score[u, j]) for j in real if j not in cur]
            if not ds:
                continue
            dropped_real += len(ds)
            top = float(score[u][mask[u]].max())
            gap = (min(ks) - max(ds)) / top
            print("%s layer %d utterance %d: %d -> %d, gap / largest score = %.3e" % (name, l, u, cnt[l], cnt[l + 1], gap))
            assert gap >= 100 * R.TOL, "%s layer %d utterance %d: the scores at the cut are %.3e of the largest apart" % (name, l, u, gap)
        assert 2 * differ >= B, "%s layer %d: the kept set is the first k positions in %d of %d utterances" % (name, l, B - differ, B)
    assert dropped_real > 0
