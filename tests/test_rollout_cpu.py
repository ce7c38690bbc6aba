"""CPU: attention rollout - the restatement trainer.rollout_reference on hand cases, the --predict_rollout record, the ABI of
nbest_attention_rollout_step and the command line's refusals."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT

import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi as hb, trainer


# ---- rollout_reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.0, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("S", [1, 4, 7])
def test_one_uniform_layer(S, rho):
    """L = 1, uniform attention over S unmasked keys: rho e_0 + (1 - rho) / S"""
    a = torch.full((2, 3, S, S), 1.0 / S, dtype=torch.float64)
    got = trainer.rollout_reference((a,), rho)
    assert got.dtype == torch.float64 and got.shape == (1, 2, S)
    want = torch.full((S,), (1.0 - rho) / S, dtype=torch.float64)
    want[0] += rho
    assert (got[0] - want).abs().max().item() <= 1e-15


# two layers, two heads, three tokens; the head means M0 = [[0,1,0],[0,.5,.5],[1,0,0]] and M1 = [[.5,.25,.25],[0,1,0],[0,0,1]] do
# not commute.  rho = 0.5: A~0 = [[.5,.5,0],[0,.75,.25],[.5,0,.5]], A~1 = [[.75,.125,.125],[0,1,0],[0,0,1]]
A0 = torch.tensor([[[0, 1, 0], [0, 1, 0], [1, 0, 0]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]]], dtype=torch.float32)
A1 = torch.tensor([[[.5, .5, 0], [0, 1, 0], [0, 0, 1]], [[.5, 0, .5], [0, 1, 0], [0, 0, 1]]], dtype=torch.float32)


def test_two_layers_by_hand():
    got = trainer.rollout_reference((A0[None], A1[None]), 0.5)
    assert got.shape == (2, 1, 3)
    # layers[1] = e_0 A~1; layers[0] = e_0 A~1 A~0 (the upper layer's row pushed through the lower layer)
    assert got[1, 0].tolist() == [0.75, 0.125, 0.125]
    assert got[0, 0].tolist() == [0.4375, 0.46875, 0.09375]
    rev = trainer.rollout_reference((A1[None], A0[None]), 0.5)
    assert rev[0, 0].tolist() == [0.375, 0.5625, 0.0625]
    assert (rev[0, 0] - got[0, 0]).abs().max().item() > 0.05, "the layer order does not matter to the restatement"


def test_rows_sum_to_one_and_residual_one_is_one_hot():
    g = torch.Generator().manual_seed(3)
    L, B, heads, S = 4, 3, 5, 9
    maps = tuple(torch.softmax(torch.randn(B, heads, S, S, generator=g, dtype=torch.float64) * 2, -1) for _ in range(L))
    for rho in (0.0, 0.25, 0.9):
        got = trainer.rollout_reference(maps, rho)
        assert got.shape == (L, B, S) and (got >= 0).all()
        assert (got.sum(-1) - 1).abs().max().item() <= 1e-12
    # the last entry is the top layer's head-mean CLS attention mixed with rho
    top = 0.25 * torch.eye(S, dtype=torch.float64)[0] + 0.75 * maps[-1].double().mean(1)[:, 0]
    assert (trainer.rollout_reference(maps, 0.25)[L - 1] - top).abs().max().item() <= 1e-15
    one = trainer.rollout_reference(maps, 1.0)
    want = torch.zeros(L, B, S, dtype=torch.float64)
    want[:, :, 0] = 1.0
    assert torch.equal(one, want)


# ---- rollout_record ----------------------------------------------------------------------------------------------------------------
def test_rollout_record():
    spans = [("cls", 0, 1), ("sys", 1, 6), ("h1", 6, 11), ("h2", 11, 17)]
    n, S = 17, 24
    g = torch.Generator().manual_seed(5)
    p = torch.rand(n, generator=g, dtype=torch.float64) ** 3
    p = p / p.sum()
    row = torch.cat([p, torch.zeros(S - n, dtype=torch.float64)]).float()
    rec = trainer.rollout_record(7, spans, row, 0.5)
    assert set(rec) == {"line", "segments", "tokens", "residual", "mass", "token_rollout"}
    assert rec["line"] == 7 and rec["segments"] == ["cls", "sys", "h1", "h2"] and rec["tokens"] == [1, 5, 5, 6] and rec["residual"] == 0.5
    assert len(rec["token_rollout"]) == sum(rec["tokens"]) == n and len(rec["mass"]) == 4
    assert abs(sum(rec["mass"]) - 1.0) < 1e-5
    for k, (_, a, b) in enumerate(spans):
        assert abs(rec["mass"][k] - p[a:b].sum().item()) < 2e-6
    for x, y in zip(rec["token_rollout"], p.tolist()):
        assert abs(x - y) < 2e-6
    for x in rec["mass"] + rec["token_rollout"]:
        assert x == round(x, 6)
    assert json.loads(json.dumps(rec)) == rec
    # unmasked padding keys (XLM-R, quirk Q1) hold a share of the row: it is left out, the utterance's own tokens sum to 1
    row2 = row.clone()
    row2[n:] = 0.02
    row2 = row2 / row2.sum()
    rec2 = trainer.rollout_record(1, spans, row2, 0.25)
    assert abs(sum(rec2["mass"]) - 1.0) < 1e-5 and abs(sum(rec2["token_rollout"]) - 1.0) < 1e-4 and rec2["residual"] == 0.25
    for x, y in zip(rec2["token_rollout"], rec["token_rollout"]):
        assert abs(x - y) < 2e-6


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_step_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "nbest_hip.h")).read()
    m = re.search(r"int\s+nbest_attention_rollout_step\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/nbest_hip.h does not declare nbest_attention_rollout_step"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["qkv", "key_mask", "lse", "r_in", "r_out", "residual", "B", "S", "heads", "d",
                                                         "dtype", "stream"]
    assert "nbest_attention_rollout_step" in hb.EXPORTS
    assert os.path.exists(hb.LIB_PATH), "run __graft_entry__.build() first"
    assert hasattr(ctypes.CDLL(hb.LIB_PATH), "nbest_attention_rollout_step")
    assert callable(hb.attention_rollout_step)


# ---- command line ------------------------------------------------------------------------------------------------------------------
FILE = os.path.join(GOLDEN, "valid_head.txt")
BASE = ["--dataset", "dstc2", "--dataroot", GOLDEN, "--deviceId", "0", "--experiment", "exp", "--label_space", os.path.join(GOLDEN, "label_space.json")]


def _refused(argv, capsys, word):
    with pytest.raises(SystemExit) as e:
        cli.parse_arguments(BASE + argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_cli_accepts_predict_rollout(tmp_path):
    out = str(tmp_path / "r.jsonl")
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--predict_rollout", out])
    assert opt.predict_rollout == out and opt.rollout_residual == 0.5
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--predict_rollout", out, "--rollout_residual", "0.25"])
    assert opt.rollout_residual == 0.25
    for r in ("0", "1"):
        assert cli.parse_arguments(BASE + ["--predict", FILE, "--predict_rollout", out, "--rollout_residual", r]).rollout_residual == float(r)
    opt = cli.parse_arguments(BASE + ["--predict", FILE, "--predict_rollout", out, "--predict_attention", str(tmp_path / "a.jsonl"),
                                      "--predict_attribution", str(tmp_path / "b.jsonl")])
    assert opt.predict_rollout == out and opt.predict_attention and opt.predict_attribution
    assert cli.parse_arguments(BASE + ["--predict", FILE]).predict_rollout is None


def test_cli_parse_errors(capsys, tmp_path):
    mask = tmp_path / "mask.json"
    mask.write_text("[[1]]")
    out = str(tmp_path / "r.jsonl")
    ok = ["--predict", FILE, "--predict_rollout", out]
    _refused(["--predict_rollout", out], capsys, "--predict FILE")
    _refused(ok + ["--dtype", "fp8w", "--predict_fp8"], capsys, "--predict_fp8")
    _refused(ok + ["--head_mask", str(mask)], capsys, "--head_mask")
    _refused(ok + ["--head_mask", str(mask), "--compact_heads"], capsys, "--compact_heads")
    _refused(["--predict", FILE, "--rollout_residual", "0.5"], capsys, "--predict_rollout")
    for r in ("-0.1", "1.5", "nan"):
        _refused(ok + ["--rollout_residual", r], capsys, "--rollout_residual")
