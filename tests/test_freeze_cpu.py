"""Frozen parameters (requires_grad False) on the host: the stash and workspace sizes of nbest_encoder_desc.first_trainable,
the freeze plan a model derives from its flags, the CLI flags and their refusals, and a world-2 gloo run of the gradient
exchange restricted to the trainable ranges."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _al(x):
    return (x + 255) & ~255


def _desc(hb, L, B=2, S=64, H=128, F=256, dtype=None, first_trainable=0):
    d = hb.EncoderDesc()
    d.dtype = hb.F32 if dtype is None else dtype
    d.B, d.S, d.H, d.L, d.heads, d.F = B, S, H, L, H // 64, F
    d.vocab, d.max_pos, d.n_types = 300, 512, 2
    d.pos_pad_id = -1
    d.first_trainable = first_trainable
    return d


def _lib():
    import nbest_amd  # noqa: F401
    from nbest_amd import hipabi as hb
    if not os.path.exists(hb.LIB_PATH):
        pytest.skip("libnbest_hip.so is not built")
    return hb, hb.lib()


def test_zeroed_descriptor_keeps_todays_stash_size():
    """fp32: X[0..L] + emb_stats + L layer blocks, as the layout comment of encoder.hip states"""
    hb, lib = _lib()
    B, S, H, F, L = 2, 64, 128, 256, 4
    M = B * S
    MH, MF, M3H = _al(M * H * 4), _al(M * F * 4), _al(M * 3 * H * 4)
    st, lse = _al(M * 8), _al(B * (H // 64) * S * 4)
    layer = M3H + MH + lse + MH + st + MH + MF + MF + MH + st
    want = (L + 1) * MH + st + L * layer
    d = _desc(hb, L, B, S, H, F)
    assert (d.first_trainable, d.no_input_grad, d.wgrad_skip_host) == (0, 0, None)
    assert lib.nbest_encoder_act_bytes(C.byref(d)) == want


@pytest.mark.parametrize("dtype_name", ["F32", "BF16"])
def test_act_bytes_shrink_by_the_frozen_layers(dtype_name):
    hb, lib = _lib()
    dt = getattr(hb, dtype_name)
    B, S, L = 2, 64, 6
    M = B * S
    esz = 2 if dtype_name == "BF16" else 4
    MH, st = _al(M * 128 * esz), _al(M * 8)
    full = lib.nbest_encoder_act_bytes(C.byref(_desc(hb, L, B, S, dtype=dt)))
    layer = (full - (L + 1) * MH - st) // L
    ws0 = lib.nbest_encoder_ws_bytes(C.byref(_desc(hb, L, B, S, dtype=dt)))
    for K in range(1, L + 1):
        got = lib.nbest_encoder_act_bytes(C.byref(_desc(hb, L, B, S, dtype=dt, first_trainable=K)))
        # X[K..L] and layers K..L-1; no embedding statistics (the embeddings are frozen too)
        assert got == (L + 1 - K) * MH + (L - K) * layer, K
        assert got == full - K * (MH + layer) - st
        # the frozen layers' forward runs on scratch in ws: a few [M][H] buffers more, independent of K
        ws = lib.nbest_encoder_ws_bytes(C.byref(_desc(hb, L, B, S, dtype=dt, first_trainable=K)))
        assert ws0 < ws <= ws0 + 2 * MH + 4 * st + _al(B * 2 * S * 4)


def _cpu_model(L=4):
    import nbest_amd  # noqa: F401
    from nbest_amd import config as ncfg
    from nbest_amd.model import NBestSTCModel
    labels = ncfg.LabelSpace.from_json(os.path.join(ROOT, "tests", "golden", "label_space.json"))
    cfg = ncfg.bert_base(num_hidden_layers=L, vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256)
    return NBestSTCModel(cfg, labels, device="cpu", compute_dtype=torch.float32)


def test_freeze_plan_from_requires_grad():
    from nbest_amd.model import freeze_plan
    m = _cpu_model(4)
    p = freeze_plan(m)
    assert (p.first_trainable, p.no_input_grad, p.with_embeddings, p.skip) == (0, 0, True, None)
    assert not any("pooler" in n for n in p.trainable)
    for q in m.bert_encoder.embeddings.parameters():
        q.requires_grad_(False)
    p = freeze_plan(m)
    assert (p.first_trainable, p.no_input_grad, p.with_embeddings, p.skip) == (0, 1, False, None)
    for n, q in m.named_parameters():
        if n.startswith(("bert_encoder.encoder.layer.0.", "bert_encoder.encoder.layer.1.")):
            q.requires_grad_(False)
    p = freeze_plan(m)
    assert (p.first_trainable, p.no_input_grad, p.with_embeddings) == (2, 1, False)
    assert list(p.skip) == [1] * 8 + [0] * 8
    # a frozen middle matrix: the QKV gradient is skipped only when all of Q, K and V are frozen
    lay3 = "bert_encoder.encoder.layer.3."
    m.get_parameter(lay3 + "output.dense.weight").requires_grad_(False)
    m.get_parameter(lay3 + "attention.self.key.weight").requires_grad_(False)
    p = freeze_plan(m)
    assert list(p.skip)[12:] == [0, 0, 0, 1]
    for n in ("query", "value"):
        m.get_parameter(lay3 + "attention.self.%s.weight" % n).requires_grad_(False)
    assert list(freeze_plan(m).skip)[12:] == [1, 0, 0, 1]
    for q in m.parameters():
        q.requires_grad_(False)
    p = freeze_plan(m)
    assert p.first_trainable == 4 and not p.trainable


def test_cli_freeze_flags_and_refusals():
    from nbest_amd import cli
    base = ["--dataset", "d", "--dataroot", "r", "--deviceId", "0"]
    o = cli.parse_arguments(base)
    assert (o.freeze_embeddings, o.freeze_layers) == (False, 0)
    name = cli.exp_dir(o)
    assert "fz_" not in name                                     # existing experiment names do not change
    o2 = cli.parse_arguments(base + ["--freeze_embeddings", "--freeze_layers", "2"])
    assert cli.exp_dir(o2) == name + "__fz_emb_2"
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--freeze_layers", "-1"])
    m = _cpu_model(4)
    with pytest.raises(SystemExit):
        cli.freeze_parameters(m, False, 5)
    frozen = cli.freeze_parameters(m, True, 4)
    assert all(not p.requires_grad for n, p in m.named_parameters() if n in frozen)
    assert all(p.requires_grad for n, p in m.named_parameters() if n not in frozen and "pooler" not in n)
    assert any(n.startswith("clf.") for n, _ in m.named_parameters() if n not in frozen)
    assert len([n for n in frozen if n.startswith("bert_encoder.embeddings.")]) == 5


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import nbest_amd  # noqa: F401
    from nbest_amd import trainer
    from nbest_amd.model import freeze_plan
    m = _cpu_model(4)
    a = m.arena
    for n, p in m.named_parameters():
        if n.startswith(("bert_encoder.embeddings.", "bert_encoder.encoder.layer.0.", "bert_encoder.encoder.layer.1.")):
            p.requires_grad_(False)
    m.get_parameter("bert_encoder.encoder.layer.3.output.dense.weight").requires_grad_(False)     # a frozen middle matrix
    plan = freeze_plan(m)
    torch.manual_seed(rank)
    a.g.copy_(torch.randn(a.total))
    local = a.g.clone()
    sent = []                                            # arena ranges handed to all_reduce
    real = dist.all_reduce

    def spy(t, *args, **kw):
        lo = (t.data_ptr() - a.g.data_ptr()) // 4
        sent.append((lo, lo + t.numel()))
        return real(t, *args, **kw)
    dist.all_reduce = spy
    red = trainer.GradReducer(a, n_chunks=2, sparse_word_grad=True)
    red.set_trainable(plan.trainable)
    red.set_step_tokens(torch.tensor([[5, 6, 7]]))      # frozen word table: no count exchange, no row exchange
    ok = red._tok is None
    for lo, hi in sorted(red.chunks, reverse=True):
        red.layers_ready(lo, hi)
    red.wait()
    dist.all_reduce = real
    gathered = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    want = sum(gathered)
    for s in a.slots:
        seg = slice(s.offset, s.offset + s.numel)
        if s.name in plan.trainable:
            ok = ok and torch.allclose(a.g[seg], want[seg], atol=1e-6)
        else:                                            # frozen (or pooler): never sent, untouched
            ok = ok and torch.equal(a.g[seg], local[seg])
            ok = ok and not any(lo < s.offset + s.numel and s.offset < hi for lo, hi in sent)
    both = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(both, torch.where(torch.isin(torch.arange(a.total), torch.cat(
        [torch.arange(s.offset, s.offset + s.numel) for s in a.slots if s.name in plan.trainable])), a.g, torch.zeros_like(a.g)))
    ok = ok and torch.equal(both[0], both[1])            # replicas of every trainable gradient bit-identical
    # everything trainable again: the full buckets (heads + 2 layer buckets + embeddings)
    for p in m.parameters():
        p.requires_grad_(True)
    red.set_trainable(freeze_plan(m).trainable)
    ok = ok and red.trainable is None and not red.word_frozen
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_reducer_sends_no_frozen_range_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29631
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(res) == [(0, True), (1, True)]
