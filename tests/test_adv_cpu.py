"""CPU tests of FGM adversarial training on the word embeddings (--adv_epsilon): the fp64 restatement that tests/test_adv_gpu.py holds
forward_backward(adv=) to (self-checked against the first-order Taylor term it maximises), the C ABI surface, the descriptor field,
model._check_adv, the command line and train_step's refusals - device-free."""
import copy
import ctypes
import os
import re

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi, trainer

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]
ADV = ["--adv_epsilon", "1.0"]
SYMBOLS = ("nbest_embed_ln_fwd_adv", "nbest_embed_ln_bwd_adv", "nbest_embed_adv_ws_bytes", "nbest_embed_adv_delta")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def fgm_reference(model, batch, epsilon, top2bottom=None, seg=True, add_l2=False):
    """One FGM step on a copy of the oracle ``model`` in fp64.  ``batch``: dict(ids, seg, tids, tseg, labels) of CPU tensors.  A
    forward hook on ``bert_encoder.embeddings.word_embeddings`` keeps the output of the ASR pass (the first call of a forward; the
    transcript pass, the second, is left alone), whose gradient after the clean backward is g; delta = epsilon g / ||g||, the norm
    per utterance, zero on padding tokens (ids == 0: the key mask of every family) and for an utterance without gradient.  The same
    hook adds delta on the second pass, which has the hard terms only and no transcript.  Returns dict(loss_parts [4] (the clean
    pass: bottom BCE, top BCE, CE, MSE or 0), adv_loss_parts [3], norm [B], delta [B, S, H], g [B, S, H], grads {name: clean +
    adversarial}, clean_grads)."""
    from oracle import stc
    om = copy.deepcopy(model).double()
    om.train()
    for p in om.parameters():
        p.grad = None
    if top2bottom is None:
        top2bottom = om.clf.top2bottom
    b2t = stc.bottom2top_matrix(top2bottom).double()
    ids, y = batch["ids"].long(), batch["labels"].double()
    sg = batch["seg"].long() if (seg and batch.get("seg") is not None) else None
    state = dict(calls=0, delta=None, e=None)

    def hook(mod, inp, out):
        state["calls"] += 1
        if state["calls"] != 1:
            return None
        if state["delta"] is not None:
            return out + state["delta"]
        out.retain_grad()
        state["e"] = out
        return None

    h = om.bert_encoder.embeddings.word_embeddings.register_forward_hook(hook)
    try:
        tids = batch["tids"].long() if add_l2 else None
        top, bottoms, final, asr, tr = om(ids, tids, seg_ids=sg, trans_seg_ids=batch["tseg"].long() if add_l2 else None)
        _, total, parts = stc.total_loss(top, bottoms, final, y, top2bottom, b2t, asr, tr, add_l2)
        total.backward()
        clean = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
        mask = (ids > 0).unsqueeze(-1).double()
        g = state["e"].grad.detach() * mask
        norm = g.flatten(1).norm(dim=1)
        ok = (norm > 0) & torch.isfinite(norm)
        scale = torch.where(ok, epsilon / norm.clamp_min(1e-300), torch.zeros_like(norm))
        delta = g * scale.view(-1, 1, 1)
        state.update(calls=0, delta=delta)
        top2, bottoms2, final2, _, _ = om(ids, None, seg_ids=sg)
        _, total2, parts2 = stc.total_loss(top2, bottoms2, final2, y, top2bottom, b2t)
        total2.backward()
    finally:
        h.remove()
    lp = torch.stack([parts["bottom_bce"], parts["top_bce"], parts["ce"], parts.get("mse", torch.zeros((), dtype=torch.float64))]).detach()
    alp = torch.stack([parts2["bottom_bce"], parts2["top_bce"], parts2["ce"]]).detach()
    grads = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
    return dict(loss_parts=lp, adv_loss_parts=alp, norm=norm, delta=delta, g=g, grads=grads, clean_grads=clean)


@pytest.fixture(scope="module")
def small(labels):
    """a 1-layer bert oracle and a ragged batch of 4 utterances (S 24) with transcripts"""
    from nbest_amd import config as ncfg, synth
    from oracle.encoder import EncoderConfig
    from oracle.model import OracleModel
    cfg = ncfg.bert_base(num_hidden_layers=1, vocab_size=3000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = synth.model_state(cfg, labels, seed=11)
    ocfg = EncoderConfig(**{k: v for k, v in cfg.to_dict().items() if k in EncoderConfig.__dataclass_fields__})
    om = OracleModel(ocfg, labels.top2bottom, labels.n_bottom, 0.0)
    om.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    batch = {k: torch.from_numpy(v) for k, v in synth.nbest_batch(cfg, labels, 4, 24, n_best=3, seed=5, ragged=True, trans_len=8).items()}
    return om, batch


def test_reference_moves_along_the_first_order_term(small, labels):
    """epsilon 1e-3 on a 1-layer model: L(x + delta) - L(x) agrees with the first-order Taylor term sum_b <g_b, delta_b> =
    epsilon sum_b n_b to 5 % (the Taylor term is what is measured against); delta is exactly zero on padding tokens and
    ||delta_b|| = epsilon to 1e-12"""
    om, batch = small
    eps = 1e-3
    for add_l2 in (False, True):
        r = fgm_reference(om, batch, eps, labels.top2bottom, add_l2=add_l2)
        pad = batch["ids"] == 0
        assert bool(pad.any()) and bool((~pad).all(dim=1).logical_not().any())
        assert r["delta"][pad].abs().max().item() == 0.0
        assert bool((r["norm"] > 0).all())
        assert (r["delta"].flatten(1).norm(dim=1) - eps).abs().max().item() <= 1e-12 * eps
        if not add_l2:                                                  # (with the MSE, g is the gradient of hard + MSE: another function)
            taylor = eps * r["norm"].sum().item()
            rise = (r["adv_loss_parts"].sum() - r["loss_parts"][:3].sum()).item()
            assert taylor > 0 and abs(rise - taylor) <= 0.05 * taylor, (rise, taylor)
        else:
            assert r["loss_parts"][3].item() > 0
        # the returned gradients are the sum of the two passes'
        n = "bert_encoder.embeddings.word_embeddings.weight"
        assert not torch.equal(r["grads"][n], r["clean_grads"][n])


def test_reference_epsilon_zero_doubles_the_clean_gradient(small, labels):
    om, batch = small
    r = fgm_reference(om, batch, 0.0, labels.top2bottom)
    assert r["delta"].abs().max().item() == 0.0
    assert torch.equal(r["adv_loss_parts"], r["loss_parts"][:3])
    for n, g in r["clean_grads"].items():
        assert torch.allclose(r["grads"][n], 2 * g, rtol=1e-12, atol=0.0), n


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hipabi_binds_the_entry_points():
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    L = ctypes.CDLL(hipabi.LIB_PATH)
    for name in SYMBOLS:
        assert name in hipabi.EXPORTS, name
        assert re.search(r"\b(int|size_t) %s\(" % name, hdr), "include/nbest_hip.h does not declare %s" % name
        assert hasattr(L, name), name
    fwd = " ".join(re.search(r"int nbest_embed_ln_fwd\(([^;]*)\);", hdr).group(1).split()).split(",")
    adv = " ".join(re.search(r"int nbest_embed_ln_fwd_adv\(([^;]*)\);", hdr).group(1).split()).split(",")
    assert len(adv) == len(fwd) + 1 and any("const float* delta" in a for a in adv)
    bwd = " ".join(re.search(r"int nbest_embed_ln_bwd\(([^;]*)\);", hdr).group(1).split()).split(",")
    badv = " ".join(re.search(r"int nbest_embed_ln_bwd_adv\(([^;]*)\);", hdr).group(1).split()).split(",")
    assert len(badv) == len(bwd) + 1 and any("const float* delta" in a for a in badv)
    lib = hipabi.lib()
    assert len(lib.nbest_embed_ln_fwd_adv.argtypes) == len(lib.nbest_embed_ln_fwd.argtypes) + 1
    assert len(lib.nbest_embed_ln_bwd_adv.argtypes) == len(lib.nbest_embed_ln_bwd.argtypes) + 1
    assert lib.nbest_embed_adv_ws_bytes(5, 37) >= 5 * 37 * 4
    assert hasattr(hipabi, "embed_adv_delta")


def test_descriptor_field_sits_between_no_input_grad_and_wgrad_skip_host():
    names = [f[0] for f in hipabi.EncoderDesc._fields_]
    i = names.index("emb_delta")
    assert names[i - 1] == "no_input_grad" and names[i + 1] == "wgrad_skip_host"
    assert hipabi.EncoderDesc.emb_delta.offset % 8 == 0 and hipabi.EncoderDesc.emb_delta.size == 8
    assert hipabi.EncoderDesc().emb_delta is None
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    body = hdr[hdr.index("typedef struct nbest_encoder_desc {"):hdr.index("} nbest_encoder_desc;")]
    fields = re.findall(r"^\s*(?:const\s+)?[A-Za-z_0-9]+\**\s+\**([a-z_0-9]+);", body, flags=re.M)
    j = fields.index("emb_delta")
    assert fields[j - 1] == "no_input_grad" and fields[j + 1] == "wgrad_skip_host"
    assert re.search(r"const float\* emb_delta;", body)


def test_entry_points_check_their_arguments_on_the_host():
    """null pointers, a negative or non-finite epsilon, a small workspace: an error code and a message before anything touches a device"""
    L = hipabi.lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)

    def delta(epsilon=1.0, ws_bytes=1 << 20, dout=fake, B=2, S=4):
        return L.nbest_embed_adv_delta(fake, fake, fake, fake, fake, fake, fake, fake, dout, fake, fake, B, S, 768, 1e-12, hipabi.F32, 0.0, 0, 0,
                                       epsilon, fake, ws_bytes, null)
    for kw in (dict(epsilon=-1.0), dict(epsilon=float("nan")), dict(epsilon=float("inf")), dict(ws_bytes=8), dict(dout=null), dict(B=0)):
        assert delta(**kw) < 0, kw
        assert "embed_adv_delta" in hipabi.last_error(), kw
    assert L.nbest_embed_ln_fwd_adv(fake, fake, fake, fake, fake, fake, fake, fake, null, fake, fake, 8, 768, 1e-12, hipabi.F32, 0.0, 0, 0, null) < 0
    assert "embed_ln_fwd_adv" in hipabi.last_error()
    assert L.nbest_embed_ln_bwd_adv(*([fake] * 9), null, *([fake] * 6), 2, 4, 768, 2, hipabi.F32, 0, -1, 0, 0, 0.0, 0, 0, fake, 1 << 30, null) < 0
    assert "embed_ln_bwd_adv" in hipabi.last_error()


# ---- model -------------------------------------------------------------------------------------------------------------------------
def test_check_adv():
    from nbest_amd.model import _check_adv
    assert _check_adv(dict(epsilon=1)) == dict(epsilon=1.0) and _check_adv(dict(epsilon=0.0)) == dict(epsilon=0.0)
    distill = dict(top=None, bott=None, final=None, alpha=0.5)
    for bad, kw in ((dict(epsilon=-0.5), {}), (dict(epsilon=float("nan")), {}), (dict(epsilon=float("inf")), {}), (dict(epsilon="x"), {}),
                    (dict(), {}), (dict(epsilon=1.0, steps=3), {}), (1.0, {}), (dict(epsilon=1.0), dict(need_grad=False)),
                    (dict(epsilon=1.0), dict(distill=distill)), (dict(epsilon=1.0), dict(rdrop=dict(alpha=1.0)))):
        with pytest.raises(ValueError, match="adv"):
            _check_adv(bad, **kw)


def test_the_autograd_bridge_has_no_such_argument():
    import inspect
    from nbest_amd.model import NBestSTCModel
    assert "adv" in inspect.signature(NBestSTCModel.forward_backward).parameters
    assert "adv" not in inspect.signature(NBestSTCModel.forward).parameters


def test_train_step_refuses_before_touching_anything(monkeypatch):
    batch = dict(ids=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="adv_epsilon"):
        trainer.train_step(None, None, batch, teacher=object(), adv_epsilon=1.0)
    with pytest.raises(ValueError, match="adv_epsilon"):
        trainer.train_step(None, None, batch, rdrop_alpha=1.0, adv_epsilon=1.0)
    monkeypatch.setattr(trainer, "dist_info", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="adv_epsilon"):
        trainer.train_step(None, None, batch, adv_epsilon=1.0)
    assert trainer.adv_args(None, object(), 1.0, 2) is None and trainer.adv_args(2, None, None, 1) == dict(epsilon=2.0)


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_default_and_combinations():
    assert cli.parse_arguments(BASE).adv_epsilon is None
    assert cli.parse_arguments(BASE + ADV).adv_epsilon == 1.0
    for optim in (["--optim_choice", "bertadam"], ["--optim_choice", "adam"], ["--optim_choice", "adamw", "--restated_adamw"]):
        opt = cli.parse_arguments(BASE + ADV + optim + ["--ema_decay", "0.9", "--resume", "--add_l2_loss", "--freeze_layers", "0"])
        assert opt.adv_epsilon == 1.0 and opt.ema_decay == 0.9


def test_cli_exp_dir_moves_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert plain.endswith("__cls_stc") and "fgm" not in plain
    assert cli.exp_dir(cli.parse_arguments(BASE + ADV)) == plain + "__fgm_1.0"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--adv_epsilon", "0.5", "--ema_decay", "0.9"])) == plain + "__ema_0.9__fgm_0.5"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--rdrop_alpha", "1.0"])) == plain + "__rdrop_1.0"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--ema_decay", "0.9"])) == plain + "__ema_0.9"


def test_cli_refusals(tmp_path, monkeypatch, capsys):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    for bad, word in ((ADV + ["--testing"], "--testing"), (ADV + ["--predict", str(src)], "--predict"),
                      (ADV + ["--head_importance", str(tmp_path / "imp.json")], "--head_importance"),
                      (ADV + ["--distill_from", "t.pt"], "--distill_from"),
                      (ADV + ["--rdrop_alpha", "1.0", "--dropout", "0.3"], "--rdrop_alpha"),
                      (ADV + ["--dtype", "fp8w"], "fp8w"), (ADV + ["--freeze_embeddings"], "--freeze_embeddings"),
                      (ADV + ["--freeze_layers", "1"], "--freeze_layers"),
                      (["--adv_epsilon", "0"], "--adv_epsilon"), (["--adv_epsilon", "-1"], "--adv_epsilon"),
                      (["--adv_epsilon", "nan"], "--adv_epsilon"), (["--adv_epsilon", "inf"], "--adv_epsilon")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        assert word in capsys.readouterr().err, bad
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + ADV)
    assert "data parallelism is not built" in capsys.readouterr().err
    assert cli.parse_arguments(BASE).adv_epsilon is None                # ... and fine without the flag
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.parse_arguments(BASE + ADV).adv_epsilon == 1.0
