"""CPU: the inference entry point's workspace contract, --predict argument handling and the prediction reader."""
import ctypes as C
import os

import pytest

from conftest import GOLDEN


def _desc(cfg, B, S, dtype):
    from nbest_amd import hipabi as hb
    d = hb.EncoderDesc()
    d.dtype = dtype
    d.B, d.S, d.H, d.L, d.heads, d.F = B, S, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size
    d.vocab, d.max_pos, d.n_types = cfg.vocab_size, cfg.max_position_embeddings, cfg.type_vocab_size
    return d


def test_infer_workspace_is_independent_of_depth_and_small():
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg, hipabi as hb
    L = hb.lib()
    for mk, B, S in ((ncfg.bert_base, 256, 128), (ncfg.xlmr_large, 64, 512)):
        for dt in (hb.BF16, hb.F32):
            ws = {n: L.nbest_encoder_infer_ws_bytes(C.byref(_desc(mk(num_hidden_layers=n), B, S, dt))) for n in (2, 12, 24)}
            assert ws[2] == ws[12] == ws[24] > 0, ws
    for mk, B, S, n in ((ncfg.bert_base, 256, 128, 12), (ncfg.xlmr_large, 64, 512, 24)):
        d = _desc(mk(num_hidden_layers=n), B, S, hb.BF16)
        ws, act = L.nbest_encoder_infer_ws_bytes(C.byref(d)), L.nbest_encoder_act_bytes(C.byref(d))
        assert 8 * ws <= act, (mk.__name__, ws, act)


def _argv(tmp_path, extra):
    return ["--dataset", "dstc2", "--dataroot", str(tmp_path), "--deviceId", "0", "--experiment", str(tmp_path / "exp")] + extra


def test_predict_arguments(tmp_path, capsys):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    with pytest.raises(SystemExit):
        cli.parse_arguments(_argv(tmp_path, ["--predict", str(tmp_path / "missing.txt")]))
    assert "--predict %s: no such file" % (tmp_path / "missing.txt") in capsys.readouterr().err
    src = tmp_path / "new_lists.txt"
    src.write_text("hello there\n")
    opt = cli.parse_arguments(_argv(tmp_path, ["--predict", str(src)]))
    assert cli.predict_output_path(opt) == os.path.join(cli.exp_dir(opt), "new_lists.txt.pred")
    opt = cli.parse_arguments(_argv(tmp_path, ["--predict", str(src), "--predict_output", str(tmp_path / "out.txt")]))
    assert cli.predict_output_path(opt) == str(tmp_path / "out.txt")
    opt = cli.parse_arguments(_argv(tmp_path, []))
    assert opt.predict is None and opt.predict_output is None


def test_predict_refuses_torchrun(tmp_path, monkeypatch, capsys):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    src = tmp_path / "x.txt"
    src.write_text("a b\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(_argv(tmp_path, ["--predict", str(src)]))
    assert "one GPU" in capsys.readouterr().err


def test_prediction_reader_accepts_one_or_three_fields(tmp_path):
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer
    full = open(os.path.join(GOLDEN, "valid_200.txt")).read().strip("\n").split("\n")[:20]
    a = tmp_path / "full.txt"
    a.write_text("\n".join(full) + "\n")
    b = tmp_path / "asr_only.txt"
    b.write_text("\n".join(l.split("\t<=>\t")[0] for l in full) + "\n")
    ra, rb = trainer.read_predict_data(str(a)), trainer.read_predict_data(str(b))
    assert ra[0] == rb[0] == trainer.read_wcn_data(str(a))[0]
    assert ra[2] == trainer.read_wcn_data(str(a))[2] and rb[2] == [[]] * len(full)
    assert len(rb[1]) == len(full)
    c = tmp_path / "mixed.txt"
    c.write_text(full[0] + "\n" + full[1].split("\t<=>\t")[0] + "\n")
    rc = trainer.read_predict_data(str(c))
    assert rc[0] == ra[0][:2] and rc[2] == [ra[2][0], []]
    bad = tmp_path / "bad.txt"
    bad.write_text("a\t<=>\tb\n")
    with pytest.raises(ValueError, match="bad.txt:1"):
        trainer.read_predict_data(str(bad))
