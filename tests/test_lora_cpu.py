"""CPU: LoRA on merged weights - the projection identity against autograd, target parsing, the block table, the adapter file,
exp_dir naming, the command-line refusals and the new ABI symbols.  The kernels and the training path: test_lora_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

import nbest_amd  # noqa: F401
from nbest_amd import arena as ar, cli, config as ncfg, hipabi as hb, lora, synth
from nbest_amd.model import NBestSTCModel, freeze_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]
LORA = ["--lora_rank", "8"]


# ---- the two identities the design rests on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,r,scale", [(24, 16, 1, 2.0), (40, 28, 5, 0.37), (64, 64, 8, 2.0)])
def test_projection_of_the_dense_gradient_is_autograd(rows, cols, r, scale):
    g = torch.Generator().manual_seed(rows + r)
    W0 = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    A = torch.randn(r, cols, generator=g, dtype=torch.float64).requires_grad_()
    B = torch.randn(rows, r, generator=g, dtype=torch.float64).requires_grad_()
    x = torch.randn(7, cols, generator=g, dtype=torch.float64)
    t = torch.randn(7, rows, generator=g, dtype=torch.float64)
    # the factored form, as peft computes it ...
    loss = ((x @ W0.t() + scale * (x @ A.t()) @ B.t() - t) ** 2).sum()
    loss.backward()
    # ... against: the dense gradient of the MERGED matrix, projected
    W = lora.lora_reference_merge(W0, A.detach(), B.detach(), scale).requires_grad_()
    ((x @ W.t() - t) ** 2).sum().backward()
    dA, dB = lora.lora_reference_grad(W.grad, A.detach(), B.detach(), scale)
    assert torch.allclose(dA, A.grad, rtol=1e-12, atol=1e-12) and torch.allclose(dB, B.grad, rtol=1e-12, atol=1e-12)
    assert torch.equal(lora.lora_reference_merge(W0, A.detach(), torch.zeros_like(B), scale), W0)


# ---- targets, configuration -------------------------------------------------------------------------------------------------------------
def test_target_parsing():
    assert lora.parse_targets("query,value") == ("query", "value")
    assert lora.parse_targets("value, query") == ("query", "value")                     # table order, whatever the user's
    assert lora.parse_targets(["ffn_down", "key"]) == ("key", "ffn_down")
    assert lora.parse_targets(",".join(lora.TARGET_NAMES)) == ("query", "key", "value", "attn_out", "ffn_up", "ffn_down")
    for bad in ("", "q", "query,query", "query,dense", []):
        with pytest.raises(ValueError, match="lora"):
            lora.parse_targets(bad)
    assert lora.check_config(8, 16, 12) == (8, 16.0, tuple(range(12)))
    assert lora.check_config(64, 0.5, 4, [3, 1, 1]) == (64, 0.5, (1, 3))
    for rank, alpha, layers in ((0, 1, None), (65, 1, None), (2.5, 1, None), (8, 0, None), (8, float("nan"), None), (8, 1, [4]), (8, 1, [])):
        with pytest.raises(ValueError, match="lora"):
            lora.check_config(rank, alpha, 4, layers)


# ---- the block table of a bert-base arena -----------------------------------------------------------------------------------------------
def test_block_table_of_bert_base(labels):
    cfg = ncfg.bert_base()
    a = ar.ParamArena(cfg, labels, "cpu", compute_dtype=torch.float32)           # zero pages: nothing is touched
    H, F, L, r = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, 8
    st = lora.LoraState(a, r, 16, lora.TARGET_NAMES, device="cpu")
    assert len(st.blocks) == 6 * L and st.table.n == 6 * L
    for l in range(L):
        q, k, v, o, up, down = st.blocks[6 * l:6 * l + 6]
        wqkv = a.layer_offsets[l].wqkv
        # query / key / value: rows 0 / H / 2H of the fused [3H, H] matrix, stride H
        assert (q.p_off, k.p_off, v.p_off) == (wqkv, wqkv + H * H, wqkv + 2 * H * H)
        assert all((b.rows, b.cols) == (H, H) for b in (q, k, v, o))
        assert o.p_off == a.layer_offsets[l].wo and up.p_off == a.layer_offsets[l].w1 and down.p_off == a.layer_offsets[l].w2
        assert (up.rows, up.cols) == (F, H) and (down.rows, down.cols) == (H, F)
    tiles = 0
    for i, b in enumerate(st.blocks):
        d = st.table.host[i]
        assert (d.p_off, d.rows, d.cols, d.stride, d.rank) == (b.p_off, b.rows, b.cols, b.cols, r) and d.scale == 2.0
        assert d.a_off % 64 == 0 and d.b_off % 64 == 0 and d.base_off % 64 == 0
        assert d.b_off >= d.a_off + r * b.cols and d.tile_start == tiles
        tiles += -(-b.rows // 64) * -(-b.cols // 256)
        if i + 1 < len(st.blocks):
            assert st.blocks[i + 1].a_off >= d.b_off + b.rows * r and st.blocks[i + 1].base_off >= d.base_off + b.rows * b.cols
    assert st.table.n_tiles == tiles and st.table.ws_bytes == hb.lib().nbest_lora_grad_ws_bytes(st.table.host, st.table.n) > 0
    assert st.n_trainable == L * r * (4 * 2 * H + 2 * (H + F))
    qv = lora.LoraState(a, r, 16, ("query", "value"), layers=[3, 11], device="cpu")
    assert [(b.layer, b.target) for b in qv.blocks] == [(3, "query"), (3, "value"), (11, "query"), (11, "value")]
    assert qv.adapted == {"bert_encoder.encoder.layer.%d.attention.self.%s.weight" % (l, t) for l in (3, 11) for t in ("query", "value")}
    assert set(qv.params) == {n + s for n in qv.adapted for s in (".lora_A", ".lora_B")}
    # the optimizer's table over the adapter arena
    _, n_t, n_b = qv.build_descs(1e-3)
    chunk = hb.lib().nbest_bertadam_chunk()
    assert n_t == 8 and n_b == sum(-(-(sh[0] * sh[1]) // chunk) for _, _, sh in qv.slots)


# ---- a small model on the CPU: enable / freeze plan / adapter file ----------------------------------------------------------------------
def _cpu_model(labels, seed=5, L=2):
    cfg = ncfg.bert_base(num_hidden_layers=L, vocab_size=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = NBestSTCModel(cfg, labels, device="cpu", compute_dtype=torch.float32)
    m.arena.load_state(synth.model_state(cfg, labels, seed=seed))
    return m


def test_enable_freezes_the_base_and_plans_the_backward(labels):
    m = _cpu_model(labels, L=3)
    before = m.arena.p.clone()
    full = freeze_plan(m)
    assert m.lora is None and full.first_trainable == 0 and full.skip is None
    st = m.enable_lora(4, 8, targets=("query", "value"), layers=[1, 2], seed=3)
    assert m.lora is st and torch.equal(m.arena.p, before)                               # B = 0: nothing to merge
    assert all(p.requires_grad == n.startswith("clf.") for n, p in m.named_parameters())
    plan = freeze_plan(m)
    assert plan.trainable == {n for n, _ in m.named_parameters() if n.startswith("clf.")}  # what the optimizer reads: no base tensor
    assert plan.first_trainable == 1 and plan.no_input_grad == 1 and not plan.with_embeddings
    assert list(plan.skip) == [1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1]                         # only the QKV weight gradients run
    for b in st.blocks:
        A, B = st.params[b.name + ".lora_A"], st.params[b.name + ".lora_B"]
        assert A.abs().max() <= 1.0 / b.cols ** 0.5 and A.abs().max() > 0.5 / b.cols ** 0.5 and not B.any()
        assert A.grad.data_ptr() == st.view(st.g, b.name + ".lora_A").data_ptr()
        assert torch.equal(st.base_view(b), m.arena.view(m.arena.p, b.name))
    with pytest.raises(RuntimeError, match="has LoRA enabled"):
        m.enable_lora(4, 8)
    with pytest.raises(RuntimeError, match="with LoRA enabled"):
        m.load_reference_state({})
    m.disable_lora()
    assert m.lora is None and freeze_plan(m).first_trainable == 0 and freeze_plan(m).skip is None
    assert all(p.requires_grad == ("pooler" not in n) for n, p in m.named_parameters())
    m.set_head_mask(torch.ones(3, 12))
    with pytest.raises(RuntimeError, match="head mask"):
        m.enable_lora(4, 8)


def test_adapter_file_round_trip_and_digest(labels, tmp_path):
    m = _cpu_model(labels)
    st = m.enable_lora(5, 10, targets="query,ffn_down", seed=1)
    for n, p in st.params.items():
        if n.endswith("lora_B"):
            p.data.normal_(generator=torch.Generator().manual_seed(len(n)))
    sd = m.lora_state_dict()
    heads = {n for n, _ in m.named_parameters() if n.startswith("clf.")}
    meta = {"format", "rank", "alpha", "targets", "layers", "base_digest"}
    assert set(sd) == meta | set(st.params) | heads                                       # factors, heads, metadata - nothing else
    assert (sd["format"], sd["rank"], sd["alpha"], sd["targets"], sd["layers"]) == (lora.FORMAT, 5, 10.0, ["query", "ffn_down"], [0, 1])
    assert re.fullmatch(r"[0-9a-f]{40}", sd["base_digest"])
    import hashlib
    h = hashlib.sha1()
    for b in st.blocks:
        h.update(m.arena.view(m.arena.p, b.name).numpy().astype("<f4").tobytes())       # B was 0 when the base was taken: p is the base
    assert sd["base_digest"] == h.hexdigest()
    torch.save(sd, tmp_path / "lora.pt")
    back = torch.load(tmp_path / "lora.pt", weights_only=True)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) if torch.is_tensor(sd[k]) else back[k] == sd[k] for k in sd)
    # another base: refused before anything is installed, naming both digests; the model stays as it was (LoRA off)
    other = _cpu_model(labels, seed=6)
    p0 = other.arena.p.clone()
    with pytest.raises(ValueError) as e:
        other.load_lora(back)
    od = lora.LoraState(other.arena, 5, 10, "query,ffn_down")
    od.capture_base(other.arena)
    assert sd["base_digest"] in str(e.value) and od.base_digest() in str(e.value) and od.base_digest() != sd["base_digest"]
    assert other.lora is None and torch.equal(other.arena.p, p0)
    assert all(p.requires_grad == ("pooler" not in n) for n, p in other.named_parameters())
    same = _cpu_model(labels)
    for bad, word in ((dict(back, format="x"), "not an adapter file"), ({k: v for k, v in back.items() if not k.endswith("lora_B")}, "lacks"),
                      (dict(back, rank=4), "shape mismatch"), (dict(back, targets=["query", "nope"]), "unknown target")):
        with pytest.raises(ValueError, match=word):
            same.load_lora(bad)
        assert same.lora is None


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_defaults_and_exp_dir():
    opt = cli.parse_arguments(BASE)
    assert opt.lora_rank is None and opt.lora_adapter is None
    plain = cli.exp_dir(opt)
    assert "lora" not in plain
    opt = cli.parse_arguments(BASE + LORA)
    assert (opt.lora_rank, opt.lora_alpha, opt.lora_targets, opt.lora_lr) == (8, 16.0, "query,value", opt.lr)
    assert cli.exp_dir(opt) == plain + "__lora_r8_a16_query+value"
    opt = cli.parse_arguments(BASE + ["--lora_rank", "4", "--lora_alpha", "6.5", "--lora_targets", "ffn_up,query", "--lora_lr", "1e-3"])
    assert (opt.lora_alpha, opt.lora_targets, opt.lora_lr) == (6.5, "query,ffn_up", 1e-3)
    assert cli.exp_dir(opt) == plain + "__lora_r4_a6.5_query+ffn_up"
    # the independent options stay allowed
    opt = cli.parse_arguments(BASE + LORA + ["--rdrop_alpha", "1.0", "--dropout", "0.3", "--contrastive_weight", "0.1", "--add_l2_loss", "--resume"])
    assert cli.exp_dir(opt).endswith("__rdrop_1.0__cl_0.1_0.1__lora_r8_a16_query+value")
    assert cli.parse_arguments(BASE + LORA + ["--distill_from", "t.pt"]).lora_rank == 8


def test_cli_refusals(tmp_path, monkeypatch, capsys):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    hm = tmp_path / "mask.json"
    hm.write_text("[[1.0, 0.0]]\n")
    for bad, word in ((LORA + ["--testing"], "--testing"), (LORA + ["--predict", str(src)], "--predict"),
                      (LORA + ["--head_importance", str(tmp_path / "imp.json")], "--head_importance"),
                      (LORA + ["--dtype", "fp8w"], "fp8w"), (LORA + ["--optim_choice", "adam"], "--optim_choice adam"),
                      (LORA + ["--optim_choice", "adamw", "--restated_adamw"], "--optim_choice adamw"),
                      (LORA + ["--shard_optimizer", "on"], "--shard_optimizer"), (LORA + ["--ema_decay", "0.9"], "--ema_decay"),
                      (LORA + ["--freeze_embeddings"], "--freeze_embeddings"), (LORA + ["--freeze_layers", "1"], "--freeze_layers"),
                      (LORA + ["--train_head_mask", str(hm)], "--train_head_mask"), (LORA + ["--adv_epsilon", "1.0"], "--adv_epsilon"),
                      (["--lora_rank", "0"], "rank"), (["--lora_rank", "65"], "rank"), (LORA + ["--lora_alpha", "0"], "alpha"),
                      (LORA + ["--lora_targets", "query,dense"], "unknown target"), (LORA + ["--lora_lr", "0"], "--lora_lr"),
                      (["--lora_alpha", "4"], "--lora_rank"), (["--lora_targets", "query"], "--lora_rank"), (["--lora_lr", "1e-3"], "--lora_rank"),
                      (["--lora_adapter", str(src)], "--lora_adapter"),
                      (["--testing", "--lora_adapter", str(tmp_path / "missing.pt")], "no such file"),
                      (["--testing", "--lora_adapter", str(src), "--dtype", "fp8w"], "fp8w")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        err = capsys.readouterr().err
        assert word in err, (bad, err)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + LORA)
    assert "data parallelism is not built" in capsys.readouterr().err
    assert cli.parse_arguments(BASE).lora_rank is None                    # ... and fine without the flag
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.parse_arguments(BASE + ["--testing", "--lora_adapter", str(src)]).lora_adapter == str(src)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared():
    new = ["nbest_lora_plan", "nbest_lora_grad_ws_bytes", "nbest_lora_merge", "nbest_lora_grad"]
    L = ctypes.CDLL(hb.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nbest_hip.h")).read()
    for s in new:
        assert s in hb.EXPORTS and hasattr(L, s) and re.search(r"\b%s\(" % s, header), s
    assert "typedef struct nbest_lora_desc" in header and "#define NBEST_LORA_MAX_RANK 64" in header
    assert ctypes.sizeof(hb.LoraDesc) == 64 and hb.LORA_MAX_RANK == 64


def test_host_checks_need_no_device():
    """everything nbest_lora_merge / nbest_lora_grad refuse is refused on the host table, before a launch (no GPU here at all)"""
    ok = dict(p_off=0, base_off=0, a_off=0, b_off=512, rows=64, cols=64, rank=8, scale=2.0)
    t = hb.LoraTable([ok])
    assert t.n_tiles == 1 and t.ws_bytes == 4 * (8 * 64 + 64 * 8)
    fake = ctypes.c_void_p(1 << 20)
    lib = hb.lib()
    for change, code in ((dict(rank=0), -1), (dict(rank=65), -1), (dict(cols=62), -2), (dict(stride=128), -2), (dict(p_off=2), -4),
                         (dict(a_off=-64), -1)):
        bad = hb.LoraTable([dict(ok, **change)], plan=False)
        assert lib.nbest_lora_merge(fake, None, fake, fake, bad.host, fake, 1, None) == code, change
        assert lib.nbest_lora_grad(fake, fake, fake, bad.host, fake, 1, fake, 1 << 20, None) == code, change
        assert "lora_" in hb.last_error()
    assert lib.nbest_lora_merge(None, None, fake, fake, t.host, fake, 1, None) == -1 and "null pointer" in hb.last_error()
    assert lib.nbest_lora_grad(fake, fake, None, t.host, fake, 1, fake, 1 << 20, None) == -1
    assert lib.nbest_lora_grad(fake, fake, fake, t.host, fake, 1, fake, t.ws_bytes - 4, None) == -6 and "workspace" in hb.last_error()
    assert lib.nbest_lora_grad(fake, fake, fake, t.host, fake, 0, fake, 1 << 20, None) == -1
    t.host[0].tile_start = 3                                              # not the plan's: a kernel would index past the grid
    assert lib.nbest_lora_merge(fake, None, fake, fake, t.host, fake, 1, None) == -1 and "nbest_lora_plan" in hb.last_error()
