"""CPU: integrated-gradients attribution - the fp64 reference the GPU tests compare against (restated on oracle.model.OracleModel and
checked for completeness), the --predict_attribution flags, trainer.attribution_record, the default baseline and the new exports."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, case_inputs, load_case


# ---- the fp64 reference: IG on the oracle, autograd through the interpolated pre-LayerNorm embedding -----------------------------
def oracle_model(meta, labels, dtype=torch.float64):
    from oracle.encoder import EncoderConfig
    from oracle.model import OracleModel
    cfg, sd, batch = case_inputs(meta, labels)
    ocfg = EncoderConfig(**{k: v for k, v in cfg.to_dict().items() if k in EncoderConfig.__dataclass_fields__})
    m = OracleModel(ocfg, labels.top2bottom, labels.n_bottom, 0.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    return m.to(dtype), ocfg, cfg, sd, batch


def default_baseline(ids, pad):
    base = torch.where(ids.ne(pad), torch.full_like(ids, pad), ids)
    base[:, 0] = ids[:, 0]
    return base


def oracle_final(m, ocfg, E, ids):
    """final scores of the rows E (the pre-LayerNorm embeddings [n, S, H]) with the key mask / positions of ``ids`` [n, S]"""
    enc = m.bert_encoder
    x = enc.embeddings.LayerNorm(E)
    km = ids > 0                                    # quirk Q1, every family
    for lyr in enc.encoder.layer:
        x = lyr(x, km)
    return m.clf(x[:, 0, :])[2]


def oracle_embed_parts(m, ocfg, ids, seg):
    from oracle.encoder import position_ids_for
    emb = m.bert_encoder.embeddings
    if seg is None or ocfg.family == "xlm-roberta":
        seg = torch.zeros_like(ids)
    pos = position_ids_for(ocfg, ids)
    return emb.word_embeddings.weight, emb.token_type_embeddings(seg), emb.position_embeddings(pos)


def oracle_ig(m, ocfg, ids, seg, base, targets, steps, alphas=None):
    """fp64 IG of final[b, c] for every (b, c) of ``targets``: (attr [P, S], score, baseline_score) on the same alpha grid as
    NBestSTCModel.attribute (midpoint rule, alpha_k = (k + 1/2) / m)"""
    W, T, Pp = oracle_embed_parts(m, ocfg, ids, seg)
    a = ((torch.arange(steps, dtype=torch.float64) + 0.5) / steps) if alphas is None else alphas
    a = a.to(W.dtype)
    out, sc, bs = [], [], []
    for b, c in targets:
        wx, wb = W[ids[b]].detach(), W[base[b]].detach()
        E = (((1 - a)[:, None, None] * wb + a[:, None, None] * wx) + T[b].detach()) + Pp[b].detach()
        E.requires_grad_(True)
        f = oracle_final(m, ocfg, E, ids[b].expand(len(a), -1))[:, c]
        g, = torch.autograd.grad(f.sum(), E)
        out.append((g * (wx - wb)).sum(-1).mean(0))
        with torch.no_grad():
            ends = torch.stack([(wb + T[b]) + Pp[b], (wx + T[b]) + Pp[b]])
            fe = oracle_final(m, ocfg, ends, ids[b].expand(2, -1))[:, c]
        bs.append(fe[0])
        sc.append(fe[1])
    return torch.stack(out).detach(), torch.stack(sc).detach(), torch.stack(bs).detach()


def targets_for(final, labels, seed=0):
    """the top-scoring label and a random label of every row"""
    g = np.random.default_rng(seed)
    B = final.shape[0]
    top = final.argmax(dim=1).tolist()
    return [(b, int(top[b])) for b in range(B)] + [(b, int(g.integers(0, labels.n_bottom))) for b in range(B)]


def test_oracle_ig_is_complete(labels):
    """the reference satisfies completeness: sum_t A = F(x) - F(x') up to the Riemann error, 1e-3 |dF| + 1e-6 at m = 256"""
    meta, _ = load_case("bert_L2")
    m, ocfg, cfg, _, batch = oracle_model(meta, labels)
    ids, seg = torch.from_numpy(batch["ids"]), torch.from_numpy(batch["seg"])
    base = default_baseline(ids, cfg.pad_token_id)
    with torch.no_grad():
        W, T, Pp = oracle_embed_parts(m, ocfg, ids, seg)
        fin = oracle_final(m, ocfg, (W[ids] + T) + Pp, ids)
    tg = targets_for(fin, labels)
    A, sc, bs = oracle_ig(m, ocfg, ids, seg, base, tg, 256)
    np.testing.assert_allclose(sc.numpy(), fin[[b for b, _ in tg], [c for _, c in tg]].numpy(), rtol=0, atol=1e-12)
    for i, (b, c) in enumerate(tg):
        dF = float(sc[i] - bs[i])
        gap = abs(float(A[i].sum()) - dF)
        assert gap <= 1e-3 * abs(dF) + 1e-6, "pair (%d, %d): |sum A - dF| = %.3e, dF = %.3e" % (b, c, gap, dF)
        pads = ids[b].eq(cfg.pad_token_id) | ids[b].eq(base[b])
        assert torch.all(A[i][pads] == 0)


# ---- flags, record layout, default baseline, exports --------------------------------------------------------------------------
def test_predict_attribution_flags(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    src = tmp_path / "in.txt"
    src.write_text(open(os.path.join(GOLDEN, "valid_head.txt")).read())
    base = ["--dataset", "dstc2", "--dataroot", str(tmp_path), "--deviceId", "0"]
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--predict_attribution", str(tmp_path / "a.jsonl")])
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--predict", str(src), "--predict_attribution", str(tmp_path / "a.jsonl"), "--attribution_steps", "0"])
    opt = cli.parse_arguments(base + ["--predict", str(src), "--predict_attribution", str(tmp_path / "a.jsonl"), "--attribution_steps", "8"])
    assert opt.predict_attribution == str(tmp_path / "a.jsonl") and opt.attribution_steps == 8
    opt = cli.parse_arguments(base + ["--predict", str(src)])
    assert opt.predict_attribution is None and opt.attribution_steps == 32


def test_attribution_record_layout():
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer
    spans = [("cls", 0, 1), ("sys", 1, 4), ("h1", 4, 9), ("h2", 9, 12)]
    g = torch.Generator().manual_seed(0)
    attr = torch.randn(2, 16, generator=g)                          # tokens beyond the utterance (padding) are left out
    rec = trainer.attribution_record(7, spans, attr, ["inform-food-x", "request-area"], [1.5, -0.25], [0.5, -2.0], 16)
    ca = torch.rand(3, 2, 16, generator=g)
    att = trainer.attention_record(7, spans, ca)
    assert rec["line"] == 7 and rec["segments"] == att["segments"] and rec["tokens"] == att["tokens"] and rec["steps"] == 16
    assert [l["label"] for l in rec["labels"]] == ["inform-food-x", "request-area"]
    for i, l in enumerate(rec["labels"]):
        assert len(l["token_attr"]) == 12
        assert l["token_attr"] == [round(float(x), 6) for x in attr[i, :12].double().tolist()]
        for k, (_, lo, hi) in enumerate(spans):
            assert abs(l["mass"][k] - sum(l["token_attr"][lo:hi])) < 5e-6
    assert trainer.attribution_record(1, spans, attr[:0], [], [], [], 4)["labels"] == []


def test_default_baseline_rule():
    import nbest_amd  # noqa: F401
    from nbest_amd.model import NBestSTCModel
    ids = torch.tensor([[101, 7, 8, 102, 0, 0], [101, 5, 102, 9, 102, 0]])
    m = NBestSTCModel.__new__(NBestSTCModel)

    class _Cfg:
        pad_token_id = 0
    m.__dict__["cfg"] = _Cfg()
    got = NBestSTCModel.default_baseline(m, ids)
    assert got.tolist() == [[101, 0, 0, 0, 0, 0], [101, 0, 0, 0, 0, 0]]
    _Cfg.pad_token_id = 1                                           # XLM-R: <s> = 0 stays, everything else -> <pad> = 1
    ids = torch.tensor([[0, 7, 8, 2, 1, 1]])
    assert NBestSTCModel.default_baseline(m, ids).tolist() == [[0, 1, 1, 1, 1, 1]]
    assert torch.equal(default_baseline(ids, 1), NBestSTCModel.default_baseline(m, ids))


def test_attribution_symbols_exported():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    for name in ("nbest_embed_ln_fwd_interp", "nbest_embed_attrib"):
        assert name in hb.EXPORTS
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nbest_hip.h")).read()
    for name in ("nbest_embed_ln_fwd_interp", "nbest_embed_attrib", "no_param_grad", "base_ids"):
        assert name in hdr
    fields = [f for f, _ in hb.EncoderDesc._fields_]
    assert fields[-4:] == ["base_ids", "alpha", "no_param_grad", "pad5"]
