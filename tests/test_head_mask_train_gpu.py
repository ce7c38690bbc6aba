"""GPU: training under a head mask (set_head_mask(mask, trainable=True); nbest_encoder_desc.head_gate_stash).  The parameter
gradients against the fp64 oracle under the same gates; bit equality with the model whose attention-output columns carry the gate
(gates 0 / 0.5 / 1 scale exactly in fp32 and bf16) across the weight-gradient modes, frozen parameters, accumulation, the transcript
pass and the smallest shapes; an all-ones mask against no mask; one optimizer step; eval passes; the refusals; the CLI end to end."""
import json
import os
import shutil

import pytest
import torch

from conftest import GOLDEN, load_case
from test_attrib_cpu import oracle_model
from test_head_gate_cpu import case_tensors, mixed_mask
from test_head_gate_gpu import _hip_model
from test_head_mask_train_cpu import oracle_gated_param_grads, train_mask
from test_infer_gpu import _batch, _model, _same_state, _state

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAY = "bert_encoder.encoder.layer.%d."
WO = "attention.output.dense.weight"


# ---- 1. fp32 against the fp64 oracle ------------------------------------------------------------------------------------------------
_REF = {}


def _shared_reference(name, labels):
    """the fp64 oracle's loss and parameter gradients of a golden case under train_mask, computed once (nobody modifies it)"""
    if name not in _REF:
        meta, _ = load_case(name)
        om, ocfg, _, _, batch = oracle_model(meta, labels)
        ids, seg, y = case_tensors(meta, batch)
        mask = train_mask(ocfg.num_hidden_layers, ocfg.num_attention_heads)
        total, grads, _ = oracle_gated_param_grads(om, ocfg, labels, ids, seg, y, mask)
        _REF[name] = (meta, batch, mask, total, grads)
    return _REF[name]


@pytest.mark.parametrize("cls_top", [True, False])
@pytest.mark.parametrize("name", ["bert_L2", "xlmr_L2"])
def test_fp32_gradients_match_the_oracle_under_a_gate(name, cls_top, labels):
    """fp32, dropout 0, gates 0 / 0.3 / 1 / 1.7 in every layer: arena gradients of forward_backward under the trainable mask against
    the oracle's total.backward() through the gate hook, at the bars of tests/test_adv_gpu.py::
    test_whole_model_fp32_matches_the_fgm_reference: noise-to-signal 2e-3 per tensor (the STC heads as one fused matrix, key bias
    skipped), loss 1e-4 relative.  With the top layer on the CLS rows (the default) and full width."""
    meta, batch, mask, total, ref_g = _shared_reference(name, labels)
    for l in range(mask.shape[0]):                             # the gate set of the issue in EVERY layer, the cls_top layer included
        assert sorted(set(mask[l].tolist())) == [0.0, 0.3, 1.0, 1.7], (l, mask[l])
    m, _, _ = _hip_model(meta, labels, torch.float32)
    m.train()
    m.cls_top = cls_top
    m.set_head_mask(mask, trainable=True)
    ids, seg, y = (None if t is None else t.to(DEV) for t in case_tensors(meta, batch))
    out = m.forward_backward(ids, y, seg_ids=seg)
    torch.cuda.synchronize()
    loss = out["loss_parts"].double().cpu()[:3].sum().item()
    print("trainable mask %s fp32 cls_top=%s: loss %.6f vs %.6f" % (name, cls_top, loss, total.item()))
    assert abs(loss - total.item()) <= 1e-4 * abs(total.item())
    named = dict(m.named_parameters())
    fused = lambda n: n.startswith("clf.") and (n.endswith(".weight") or n.endswith(".bias"))
    worst = (0.0, "")
    for kind in (".weight", ".bias"):
        names = [n for n in ref_g if fused(n) and n.endswith(kind)]
        num = sum((named[n].grad.double().cpu() - ref_g[n]).pow(2).sum().item() for n in names) ** 0.5
        den = sum(ref_g[n].pow(2).sum().item() for n in names) ** 0.5
        worst = max(worst, (num / den, "clf fused " + kind))
    for n, g_ref in ref_g.items():
        if n.endswith("attention.self.key.bias") or fused(n) or "pooler" in n:   # (softmax is invariant to a key bias: both sides are noise)
            continue
        ns = ((named[n].grad.double().cpu() - g_ref).norm() / g_ref.norm().clamp_min(1e-30)).item()
        worst = max(worst, (ns, n))
    print("trainable mask %s fp32 cls_top=%s: worst gradient noise-to-signal %.3e (%s), bar 2e-3" % ((name, cls_top) + worst))
    assert worst[0] <= 2e-3, worst
    # the pruned heads: exact zeros, as in the oracle
    for l in range(mask.shape[0]):
        for h in (mask[l] == 0).nonzero().flatten().tolist():
            sl = slice(64 * h, 64 * h + 64)
            assert named[LAY % l + WO].grad[:, sl].abs().max().item() == 0.0
            assert named[LAY % l + "attention.self.query.weight"].grad[sl].abs().max().item() == 0.0


# ---- 2. bit equality with the weight-scaled model -------------------------------------------------------------------------------------
def _tiny_batch(cfg, labels, B, S, seed=3):
    """a batch at a shape the synthetic generator does not make (S < 3): random word ids behind a [CLS], full rows"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    ids[:, 0] = 101
    tids = torch.randint(1000, 2000, (B, 4), generator=g)
    tids[:, 0] = 101
    lab = _batch(cfg, labels, B, 16, seed=seed)["labels"]
    return dict(ids=ids.to(DEV), seg=torch.zeros_like(ids).to(DEV), labels=lab, tids=tids.to(DEV), tseg=torch.zeros_like(tids).to(DEV))


def _pair(labels, dtype, L=2, mode=None, family="bert"):
    """model A (to run under the trainable mixed_mask) and model B: the same weights with the attention-output columns of head h of
    layer l multiplied by the gate, no mask; same seed, train mode"""
    from nbest_amd.model import NBestSTCModel
    a, cfg, sd = _model(labels, family, L=L, dtype=dtype)
    mask = mixed_mask(L, cfg.num_attention_heads)
    sd2 = {k: v.copy() for k, v in sd.items()}
    for l in range(L):
        w = sd2[LAY % l + WO]
        for h in range(cfg.num_attention_heads):
            w[:, 64 * h:64 * h + 64] *= mask[l, h].item()
    b = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=dtype, dropout=0.3, seed=7)
    b.load_reference_state(sd2)
    for m in (a, b):
        m.train()
        if mode is not None:
            m.wgrad_group = mode
    a.set_head_mask(mask, trainable=True)
    return a, b, cfg, mask


def _fb(m, bt, **kw):
    out = m.forward_backward(bt["ids"], bt["labels"], seg_ids=bt["seg"], trans_input_ids=bt["tids"], trans_seg_ids=bt["tseg"], **kw)
    torch.cuda.synchronize()
    return out


def _assert_same_bits(tag, a, b, oa, ob, mask):
    """outputs and every gradient slice of A (masked) and B (scaled columns): torch.equal - Wo's against B's with the head's columns
    times the gate; the exact zeros of the gate-0 heads"""
    for k in ("top", "bott", "final", "loss_parts"):
        assert torch.equal(oa[k], ob[k]), (tag, k)
    na, nb = dict(a.named_parameters()), dict(b.named_parameters())
    col = mask.to(DEV).float().repeat_interleave(64, dim=1)                       # [L, H]
    n_grads = 0
    for n, p in na.items():
        if "pooler" in n:
            continue
        assert (p.grad is None) == (nb[n].grad is None), (tag, n)
        if p.grad is None:
            continue
        n_grads += 1
        want = nb[n].grad
        if n.endswith(WO):
            l = int(n.split(".layer.")[1].split(".")[0])
            want = want * col[l][None, :]
        assert torch.equal(p.grad, want), (tag, n, (p.grad.float() - want.float()).abs().max().item())
        if ".encoder.layer." in n:
            l = int(n.split(".layer.")[1].split(".")[0])
            for h in (mask[l] == 0).nonzero().flatten().tolist():
                sl = slice(64 * h, 64 * h + 64)
                if n.endswith(WO):
                    assert p.grad[:, sl].abs().max().item() == 0.0, (tag, n, h)
                elif ".attention.self." in n:                                    # Q / K / V weight rows and bias entries of the head
                    assert p.grad[sl].abs().max().item() == 0.0, (tag, n, h)
    assert n_grads > 0
    return n_grads


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bits_of_the_weight_scaled_model(dtype, labels):
    """B 4, S 48 ragged, dropout on, one forward_backward; then add_l2_loss (the transcript pass under the same mask) and a second
    call with accumulate=True on top"""
    a, b, cfg, mask = _pair(labels, dtype)
    bt = _batch(cfg, labels, 4, 48)
    n = _assert_same_bits("plain", a, b, _fb(a, bt), _fb(b, bt), mask)
    assert n >= 2 * 16 + 5
    _assert_same_bits("add_l2_loss", a, b, _fb(a, bt, add_l2_loss=True), _fb(b, bt, add_l2_loss=True), mask)
    _assert_same_bits("accumulate", a, b, _fb(a, bt, accumulate=True), _fb(b, bt, accumulate=True), mask)
    # the mask did something: the un-masked model A gives other scores
    a.set_head_mask(None)
    a.step_counter = b.step_counter
    assert not torch.equal(_fb(a, bt, need_grad=False)["final"], _fb(b, bt, need_grad=False)["final"])


@pytest.mark.parametrize("mode", ["never", "always", "window"])
def test_bits_under_every_weight_gradient_mode(mode, labels):
    """bf16, L = 3 (one layer without a partner), wgrad_group NEVER / ALWAYS / WINDOW: the deferred launches read the gated context
    from the stash long after the layer's scratch is reused"""
    from nbest_amd import hipabi as hb
    code = dict(never=hb.WGRAD_GROUP_NEVER, always=hb.WGRAD_GROUP_ALWAYS, window=hb.WGRAD_GROUP_WINDOW)[mode]
    a, b, cfg, mask = _pair(labels, torch.bfloat16, L=3, mode=code)
    bt = _batch(cfg, labels, 4, 48)
    assert hb.encoder_wgrad_plan(a._desc(4, 48, 0).desc, 0, 3)["mode"] == code
    for cls_top in (True, False):
        a.cls_top = b.cls_top = cls_top
        _assert_same_bits("wgrad_group %s cls_top %s" % (mode, cls_top), a, b, _fb(a, bt), _fb(b, bt), mask)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("frozen", ["emb+layer0", "all_layers"])
def test_bits_with_frozen_parameters(frozen, dtype, labels):
    """freeze_layers = 1 with the embeddings frozen (requires_grad_(False)): layer 0 runs on scratch and gates in place; an
    all-frozen encoder: every layer does, the top one on the CLS rows"""
    a, b, cfg, mask = _pair(labels, dtype)
    n_layers = 1 if frozen == "emb+layer0" else cfg.num_hidden_layers
    pre = ("bert_encoder.embeddings.",) + tuple(LAY % l for l in range(n_layers))
    for m in (a, b):
        for n, p in m.named_parameters():
            if n.startswith(pre):
                p.requires_grad_(False)
    bt = _batch(cfg, labels, 4, 48)
    n = _assert_same_bits(frozen, a, b, _fb(a, bt), _fb(b, bt), mask)
    assert a._training_plan().first_trainable == n_layers and n > 0
    assert all(p.grad is None for n, p in a.named_parameters() if n.startswith(pre))


@pytest.mark.parametrize("B,S", [(2, 16), (5, 33), (3, 2), (2, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bits_at_small_and_odd_shapes(dtype, B, S, labels):
    """B 2 S 16, B 5 S 33, B 3 S 2 (the smallest shape of the CLS-row top layer) and B 2 S 1 (full-width top layer)"""
    a, b, cfg, mask = _pair(labels, dtype)
    bt = _batch(cfg, labels, B, S) if S >= 3 else _tiny_batch(cfg, labels, B, S)
    assert a._cls_top_ok(True, S, None) == (S >= 2)
    _assert_same_bits("B %d S %d" % (B, S), a, b, _fb(a, bt), _fb(b, bt), mask)


# ---- 3. an all-ones trainable mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_ones_trainable_mask_equals_no_mask(dtype, labels):
    a, cfg, _ = _model(labels, dtype=dtype)
    b, _, _ = _model(labels, dtype=dtype)
    a.train()
    b.train()
    a.set_head_mask(torch.ones(cfg.num_hidden_layers, cfg.num_attention_heads), trainable=True)
    bt = _batch(cfg, labels, 4, 48)
    for kw in ({}, {"add_l2_loss": True}):
        oa, ob = _fb(a, bt, **kw), _fb(b, bt, **kw)
        for k in ("top", "bott", "final", "loss_parts", "asr_cls"):
            assert torch.equal(oa[k], ob[k]), k
        assert torch.equal(a.arena.g.view(torch.int32), b.arena.g.view(torch.int32))


# ---- 4. one optimizer step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_optimizer_step_under_the_mask(dtype, labels):
    """two train_steps (BertAdam) under the mask: the Q / K / V rows of a pruned head move by weight decay alone - they take the bits of
    the same rows of a model stepped on an all-zero gradient; the rows of a kept head do not.  Then the mask is removed and a plain
    train_step (with the transcript pass) runs, on this model and on one that never had a mask and was given the stepped weights,
    optimizer moments and counters: outputs, gradients, master and compute weights, moments, the gradient buffer and the counters are
    the same bits afterwards, and the stashes are sized without the gated contexts again - the mask leaves nothing behind"""
    from nbest_amd import trainer
    from nbest_amd.model import NBestSTCModel
    from nbest_amd.optim import HipBertAdam
    a, cfg, sd = _model(labels, dtype=dtype)
    z, _, _ = _model(labels, dtype=dtype)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    bt = _batch(cfg, labels, 4, 48)
    a.train()
    a.set_head_mask(mask, trainable=True)
    kw = dict(lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    oa, oz = HipBertAdam(a, **kw), HipBertAdam(z, **kw)
    z.arena.g.zero_()
    for _ in range(2):                                       # (the warm-up makes the first step's learning rate 0)
        trainer.train_step(a, oa, bt)
        oz.step()
    torch.cuda.synchronize()
    na, nz, n0 = dict(a.named_parameters()), dict(z.named_parameters()), sd
    for l in range(cfg.num_hidden_layers):
        pruned, kept = (mask[l] == 0).nonzero().flatten().tolist(), (mask[l] == 1).nonzero().flatten().tolist()
        for part in ("query", "key", "value"):
            for kind in ("weight", "bias"):
                n = LAY % l + "attention.self.%s.%s" % (part, kind)
                for h in pruned:
                    sl = slice(64 * h, 64 * h + 64)
                    assert torch.equal(na[n].data[sl], nz[n].data[sl]), (n, h)
                if part != "key" or kind == "weight":
                    sl = slice(64 * kept[0], 64 * kept[0] + 64)
                    assert not torch.equal(na[n].data[sl], nz[n].data[sl]), (n, "a kept head did not train")
        n = LAY % l + "attention.self.query.weight"
        sl = slice(64 * pruned[0], 64 * pruned[0] + 64)
        assert not torch.equal(na[n].data[sl].cpu(), torch.from_numpy(n0[n])[sl]), "BertAdam decays the rows of a pruned head"
    # no residue: the mask removed, a plain step equals that of a model that never had one
    a.set_head_mask(None)
    c = NBestSTCModel(cfg, labels, device=DEV, compute_dtype=dtype, dropout=0.3, seed=7)
    c.load_reference_state({k: v.detach().cpu() for k, v in a.state_dict().items()})
    c.train()
    c.step_counter = a.step_counter
    oc = HipBertAdam(c, **kw)
    oc.load_state_dict(oa.state_dict())
    o1, o2 = trainer.train_step(a, oa, bt, add_l2_loss=True), trainer.train_step(c, oc, bt, add_l2_loss=True)
    torch.cuda.synchronize()
    for k in ("top", "bott", "final", "loss_parts", "asr_cls", "trans_cls"):
        assert torch.equal(o1[k], o2[k]), k
    sa, sc = _state(a, oa), _state(c, oc)
    assert sa.keys() == sc.keys()
    for k in sa:
        if isinstance(sa[k], torch.Tensor):                                          # p, g, weights, m, v (and the fp8 histories, if any)
            assert torch.equal(sa[k].view(torch.int32) if sa[k].dtype == torch.float32 else sa[k], sc[k].view(torch.int32) if sc[k].dtype == torch.float32 else sc[k]), k
    assert sa["step"] == sc["step"] and sa["valid"] == sc["valid"] and oa.step_count == oc.step_count
    # the stashes: laid out and sized as without a mask again (their bytes are not compared: the CLS-row top layer leaves regions of
    # its block unwritten, which hold whatever the buffer held before - on A the masked passes' data, on C nothing)
    for slot, S in ((0, 48), (1, bt["tids"].shape[1])):
        assert a._desc(4, S, slot).desc.head_gate_stash == 0 and a._desc(4, S, slot).act_bytes == c._desc(4, S, slot).act_bytes
        assert sa["stash_gen"][slot] > 0 and sa["stash"][slot][1] >= a._desc(4, S, slot).act_bytes
    n = 4 * 48 * cfg.hidden_size
    assert torch.equal(sa["dh"][1][:n], sc["dh"][1][:n])


# ---- 5. eval passes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eval_under_a_trainable_mask_has_the_bits_of_the_plain_mask(dtype, labels):
    m, cfg, _ = _model(labels, dtype=dtype)
    m.eval()
    bt = _batch(cfg, labels, 4, 48)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    res = []
    for trainable in (False, True):
        m.set_head_mask(mask, trainable=trainable)
        assert m.head_mask_trainable is trainable
        ev = m.forward_backward(bt["ids"], bt["labels"], seg_ids=bt["seg"], need_grad=False)
        pr = m.predict(bt["ids"], seg_ids=bt["seg"])
        fw = m(None, bt["ids"], seg_ids=bt["seg"])
        torch.cuda.synchronize()
        res.append([ev[k].clone() for k in ("top", "bott", "final", "loss_parts", "asr_cls")] + [pr[k].clone() for k in ("top", "bott", "final", "cls")]
                   + [fw[0].clone(), fw[2].clone()])
    for x, y in zip(*res):
        assert torch.equal(x, y)
    m.set_head_mask(None)
    assert not torch.equal(m.predict(bt["ids"], seg_ids=bt["seg"])["final"], res[1][7])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(labels, monkeypatch):
    """the bridge forward, adv= and a world size above 1 in train_step under a trainable mask, and an fp8w model: each raises and
    leaves arena.g, the stashes and step_counter as they were"""
    from nbest_amd import trainer
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, dtype=torch.bfloat16)
    m.train()
    bt = _batch(cfg, labels, 4, 48)
    mask = mixed_mask(cfg.num_hidden_layers, cfg.num_attention_heads)
    m.set_head_mask(mask, trainable=True)
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, warmup=0.1, t_total=40)
    _fb(m, bt, add_l2_loss=True)
    before = _state(m)
    with pytest.raises(RuntimeError, match="head mask"):
        m(None, bt["ids"], seg_ids=bt["seg"])
    with pytest.raises(RuntimeError, match="head mask"):
        m.forward_backward(bt["ids"], bt["labels"], seg_ids=bt["seg"], adv=dict(epsilon=1.0))
    monkeypatch.setattr(trainer, "dist_info", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="head mask"):
        trainer.train_step(m, opt, bt)
    monkeypatch.undo()
    torch.cuda.synchronize()
    _same_state(before, _state(m))
    with pytest.raises(ValueError):
        m.set_head_mask(None, trainable=True)
    assert m.head_mask_trainable
    m8, _, _ = _model(labels, dtype=torch.bfloat16, fp8=True)
    m8.train()
    _fb(m8, bt)
    m8.set_head_mask(mask, trainable=True)
    before = _state(m8)
    with pytest.raises(RuntimeError, match="fp8w"):
        m8.forward_backward(bt["ids"], bt["labels"], seg_ids=bt["seg"])
    torch.cuda.synchronize()
    _same_state(before, _state(m8))


# ---- 7. the CLI end to end ----------------------------------------------------------------------------------------------------------------
def _f1_of(line):
    return line.split("(p/r/f): ")[1].split("\t")[0], line.split("Loss: ")[1].split("\t")[0], line.rsplit("Acc: ", 1)[1].strip()


def test_cli_train_head_mask(tmp_path):
    """train 1 epoch, score the heads, prune, fine-tune 1 epoch under --train_head_mask from --init_checkpoint: log.train names the
    mask, and --testing --head_mask on the fine-tuned model.pt reproduces the last valid line of the training log; --resume under
    another mask is refused"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli, trainer
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_200.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")

    def args(exp):
        return ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
                "--bert_dropout", "0.1", "--lr", "1e-3", "--bert_lr", "1e-4", "--batchSize", "16", "--max_epoch", "1", "--experiment", exp,
                "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"), "--dtype", "f32",
                "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "3", "--resume"]

    def model_pt(d):
        if not os.path.exists(os.path.join(d, "model.pt")):                  # no epoch beat F1 0: the weights of the last one
            torch.save(torch.load(os.path.join(d, "last.pt"), weights_only=True)["model"], os.path.join(d, "model.pt"))
        return os.path.join(d, "model.pt")

    base = args(str(tmp_path / "exp"))
    assert cli.main(base) == 0
    d0 = cli.exp_dir(cli.parse_arguments(base))
    init = model_pt(d0)
    imp = str(tmp_path / "imp.json")
    assert cli.main(base + ["--head_importance", imp, "--prune_heads", "6"]) == 0
    pruned = json.load(open(imp))["pruned_mask"]
    assert sum(1 for r in pruned for x in r if x == 0.0) == 6
    mask_path = str(tmp_path / "pruned.json")
    json.dump(pruned, open(mask_path, "w"))
    # the fine-tune, in an experiment root of its own
    fine = args(str(tmp_path / "fine"))
    assert cli.main(fine + ["--train_head_mask", mask_path, "--init_checkpoint", init]) == 0
    d_plain = cli.exp_dir(cli.parse_arguments(fine))
    d_hm = cli.exp_dir(cli.parse_arguments(fine + ["--train_head_mask", mask_path]))
    assert d_hm == d_plain + "__hm_" + trainer.head_mask_digest(pruned) and os.path.isdir(d_hm) and not os.path.exists(d_plain)
    log = open(os.path.join(d_hm, "log.train")).read()
    assert "Head mask: %s" % mask_path in log and trainer.head_mask_digest(pruned) in log
    ck = torch.load(os.path.join(d_hm, "last.pt"), weights_only=True)
    assert ck["head_mask"] == pruned
    sd = torch.load(model_pt(d_hm), weights_only=True)
    assert not any("mask" in k for k in sd) and sd[LAY % 0 + WO].shape == (768, 768)
    valid_lines = [l for l in log.split("\n") if l.startswith("[Valid]")]
    os.makedirs(d_plain)
    shutil.copy(os.path.join(d_hm, "model.pt"), os.path.join(d_plain, "model.pt"))
    assert cli.main(fine + ["--testing", "--head_mask", mask_path]) == 0
    tested = [l for l in open(os.path.join(d_plain, "log.test")).read().split("\n") if l.startswith("[Valid]")]
    print("training log: %s\n--testing:    %s" % (valid_lines[-1], tested[-1]))
    assert _f1_of(tested[-1]) == _f1_of(valid_lines[-1])
    # a mask of the wrong shape exits before its directory is made
    bad_path = str(tmp_path / "bad.json")
    json.dump([[1.0] * 12] * 3, open(bad_path, "w"))
    with pytest.raises(SystemExit, match="train_head_mask"):
        cli.main(fine + ["--train_head_mask", bad_path])
    assert not os.path.exists(cli.exp_dir(cli.parse_arguments(fine + ["--train_head_mask", bad_path])))
    # --resume under another mask (its directory seeded with this run's checkpoint), and without one
    other = [r[:] for r in pruned]
    l, h = next((l, h) for l in range(2) for h in range(12) if other[l][h] == 1.0)
    other[l][h] = 0.5
    other_path = str(tmp_path / "other.json")
    json.dump(other, open(other_path, "w"))
    d_other = cli.exp_dir(cli.parse_arguments(fine + ["--train_head_mask", other_path]))
    os.makedirs(d_other)
    shutil.copy(os.path.join(d_hm, "last.pt"), os.path.join(d_other, "last.pt"))
    with pytest.raises(SystemExit, match="head mask"):
        cli.main(fine + ["--train_head_mask", other_path])
    shutil.copy(os.path.join(d_hm, "last.pt"), os.path.join(d_plain, "last.pt"))
    with pytest.raises(SystemExit, match="head mask"):
        cli.main(fine)
