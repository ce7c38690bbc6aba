"""CPU: the host side of the attention-map outputs - segment spans of an encoded utterance (inputs.utterance_segments), the
--predict_attention record (trainer.attention_record), its flag check, and the inference workspace it must not grow."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN


def _opt(**kw):
    base = dict(pre_trained_model="bert", tod_pre_trained_model=None, without_system_act=False)
    base.update(kw)
    return type("O", (), base)()


def _tokenizers():
    import nbest_amd  # noqa: F401
    from nbest_amd import inputs
    wp = inputs.WordPieceTokenizer(json.load(open(os.path.join(GOLDEN, "text_vocab.json"))))
    sp = inputs.SentencePieceTokenizer(os.path.join(GOLDEN, "sp_tiny.model"))
    return {"bert": wp, "xlm-roberta": sp}


def _data():
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer
    return trainer.read_wcn_data(os.path.join(GOLDEN, "valid_head.txt"))[0]


LAYOUTS = [("bert", None, False), ("bert", None, True), ("bert", "tod-bert", False), ("xlm-roberta", None, False),
           ("xlm-roberta", None, True), ("xlm-roberta", "tod", False)]


@pytest.mark.parametrize("family,tod,no_sys", LAYOUTS)
@pytest.mark.parametrize("n_best,max_seq_len", [(None, None), (3, None), (1, None), (None, 40), (5, 33), (None, 12), (None, 2)])
def test_segments_follow_encode_utterance(family, tod, no_sys, n_best, max_seq_len):
    """spans tile the encoded utterance; one h* span per kept hypothesis; every span but cls ends on a separator token (the
    first separator, a hypothesis separator or the closing / re-closing one), except the ToD system turn, which ends where the
    [USR] marker begins"""
    from nbest_amd import inputs
    tok = _tokenizers()[family]
    opt = _opt(pre_trained_model=family, tod_pre_trained_model=tod, without_system_act=no_sys)
    sep = tok.sep_token
    first_sep = sep + sep if family == "xlm-roberta" else sep
    sep_ids = set(tok.convert_tokens_to_ids([sep, first_sep]))
    usr_ids = tok.convert_tokens_to_ids(tok.tokenize("[USR]"))
    for seq in _data()[:12]:
        ids, _ = inputs.encode_utterance(seq, tok, opt, n_best, max_seq_len)
        spans = inputs.utterance_segments(seq, tok, opt, n_best, max_seq_len)
        assert sum(b - a for _, a, b in spans) == len(ids) and spans[0][1] == 0 and spans[-1][2] == len(ids)
        assert all(spans[k][2] == spans[k + 1][1] and spans[k][2] > spans[k][1] for k in range(len(spans) - 1))
        names = [n for n, _, _ in spans]
        if max_seq_len is None or len(spans) > 2:
            assert names[0] == "cls" and spans[0][1:] == (0, 1)
        want_sys = tod is not None or not no_sys
        if max_seq_len is None:
            assert ("sys" in names) == want_sys
        hyps = [n for n in names if n.startswith("h")]
        assert hyps == ["h%d" % (i + 1) for i in range(len(hyps))]
        if max_seq_len is None:
            n_in = seq[seq.index("[USR]") + 1:].count("[SEP]") + 1
            assert len(hyps) == (min(n_in, n_best) if n_best else n_in)
        else:
            full = inputs.utterance_segments(seq, tok, opt, n_best, None)
            assert len(hyps) <= len([n for n, _, _ in full if n.startswith("h")])
            if len(ids) < full[-1][2]:                          # cut: the re-closing separator is the last token of the last span
                assert ids[-1] == tok.convert_tokens_to_ids([sep])[0]
        for name, a, b in spans[1:]:
            if name == "sys" and tod:
                assert ids[b:b + len(usr_ids)] == usr_ids or b + len(usr_ids) >= len(ids)     # (or the cut fell into the marker)
            else:
                assert ids[b - 1] in sep_ids, (name, a, b, ids[a:b])
        if tod and len(hyps) and (max_seq_len is None):
            h1 = dict((n, (a, b)) for n, a, b in spans)["h1"]
            assert ids[h1[0]:h1[0] + len(usr_ids)] == usr_ids


def test_segments_of_a_known_utterance():
    from nbest_amd import inputs
    tok = _tokenizers()["bert"]
    seq = "[CLS] [SYS] hello there [USR] cheap food [SEP] cheap foot [SEP] chip".split(" ")
    n = lambda w: len(tok.tokenize(w))
    sys_n, h1, h2, h3 = n("hello") + n("there") + 1, n("cheap") + n("food") + 1, n("cheap") + n("foot") + 1, n("chip") + 1
    spans = inputs.utterance_segments(seq, tok, _opt())
    assert [(s, b - a) for s, a, b in spans] == [("cls", 1), ("sys", sys_n), ("h1", h1), ("h2", h2), ("h3", h3)]
    spans = inputs.utterance_segments(seq, tok, _opt(without_system_act=True), n_best=2)
    assert [(s, b - a) for s, a, b in spans] == [("cls", 1), ("h1", h1), ("h2", h2)]


def test_attention_record_masses_sum_to_one():
    """synthetic CLS-row probabilities [L, heads, S] (rows sum to 1 over the utterance's tokens, padding after them): the
    record's masses are per-layer means over heads of the span sums, and each layer's row sums to 1"""
    from nbest_amd import trainer
    g = torch.Generator().manual_seed(5)
    L, heads, n, S = 3, 4, 17, 24
    spans = [("cls", 0, 1), ("sys", 1, 6), ("h1", 6, 11), ("h2", 11, 17)]
    p = torch.rand(L, heads, n, generator=g) ** 4
    p[:, :, 0] = 0.0                                            # e.g. XLM-R's <s> (id 0) is a masked key
    p = p / p.sum(-1, keepdim=True)
    ca = torch.cat([p, torch.zeros(L, heads, S - n)], -1).float()
    rec = trainer.attention_record(7, spans, ca)
    assert rec["line"] == 7 and rec["segments"] == ["cls", "sys", "h1", "h2"] and rec["tokens"] == [1, 5, 5, 6]
    assert len(rec["mass"]) == L and all(len(r) == 4 for r in rec["mass"])
    for l, row in enumerate(rec["mass"]):
        assert abs(sum(row) - 1.0) < 1e-5
        for k, (_, a, b) in enumerate(spans):
            assert abs(row[k] - p[l, :, a:b].double().sum(-1).mean().item()) < 2e-6
    assert json.loads(json.dumps(rec)) == rec
    # unmasked padding keys (XLM-R pads carry id 1 > 0, quirk Q1): their share is left out, the segments still sum to 1
    ca2 = ca.clone()
    ca2[:, :, n:] = 0.01
    ca2 = ca2 / ca2.sum(-1, keepdim=True)
    for row in trainer.attention_record(1, spans, ca2)["mass"]:
        assert abs(sum(row) - 1.0) < 1e-5


def test_predict_attention_needs_predict(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    src = tmp_path / "in.txt"
    src.write_text(open(os.path.join(GOLDEN, "valid_head.txt")).read())
    base = ["--dataset", "dstc2", "--dataroot", str(tmp_path), "--deviceId", "0"]
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--predict_attention", str(tmp_path / "a.jsonl")])
    opt = cli.parse_arguments(base + ["--predict", str(src), "--predict_attention", str(tmp_path / "a.jsonl")])
    assert opt.predict_attention == str(tmp_path / "a.jsonl")
    assert cli.parse_arguments(base + ["--predict", str(src)]).predict_attention is None


def test_infer_workspace_is_unchanged():
    """nbest_encoder_infer_attn runs in nbest_encoder_infer's workspace: its size query is the same function of the shape as
    before the attention output existed (pinned for bert-base / xlm-roberta-large shapes)"""
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, hipabi as hb
    L = hb.lib()
    assert hasattr(L, "nbest_encoder_infer_attn") and hasattr(L, "nbest_attention_probs")

    def ws(cfg, B, S, dt):
        d = hb.EncoderDesc()
        d.dtype, d.B, d.S, d.H, d.L = dt, B, S, cfg.hidden_size, cfg.num_hidden_layers
        d.heads, d.F = cfg.num_attention_heads, cfg.intermediate_size
        return L.nbest_encoder_infer_ws_bytes(C.byref(d))

    al = lambda x: (x + 255) // 256 * 256
    for mk, B, S in ((ncfg.bert_base, 256, 128), (ncfg.xlmr_large, 64, 256), (ncfg.bert_base, 3, 7)):
        cfg = mk()
        for dt, esz in ((hb.BF16, 2), (hb.F32, 4)):
            M, H, F, heads = B * S, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
            want = 6 * al(M * H * esz) + 3 * al(M * 2 * 4) + al(M * 3 * H * esz) + al(M * F * esz) + al(B * heads * S * 4)
            assert ws(cfg, B, S, dt) == want
