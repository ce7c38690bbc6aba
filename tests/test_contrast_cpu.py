"""CPU: the in-batch contrastive term between the ASR and the transcript CLS rows (nbest_cls_contrast, forward_backward(contrast=),
train_step(contrast_weight=), --contrastive_weight).  The restatement of include/nbest_hip.h's K8c formulas in torch (fp64 in the
tests; ``contrast_reference``, which tests/test_contrast_gpu.py imports) against torch autograd on the same expression, its
identities, the unsaturated draw both files use with the conditions that make the GPU file's bars meaningful, transcript_keys, the
C ABI, the host-side argument checks and the command line."""
import ctypes
import math
import os
import re

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import nbest_amd  # noqa: F401
from nbest_amd import cli, hipabi, trainer

BASE = ["--dataset", "dstc2", "--dataroot", "x", "--deviceId", "0"]
CL = ["--contrastive_weight", "1.0"]
SYMBOLS = ("nbest_cls_contrast", "nbest_cls_contrast_ws_bytes")
# the GPU file's bars (tests/test_rdrop_gpu.py's for these quantities): the loss relative, a gradient against its largest element
BAR_LOSS, BAR_GRAD = 1e-5, 1e-4


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _keep(B, key, device=None):
    eye = torch.eye(B, dtype=torch.bool, device=device)
    return torch.ones(B, B, dtype=torch.bool, device=device) if key is None else (eye | (key.unsqueeze(1) != key.unsqueeze(0)))


def contrast_reference(a, t, key, weight, temperature):
    """the formulas of K8c in the dtype of ``a`` / ``t`` ([B, H]; pass fp64 for the reference), the gradients ANALYTIC:
    dict(L (unweighted, a sum over the batch), hits, da, dt (of weight * L))"""
    B = a.shape[0]
    na, nt = a.norm(dim=1, keepdim=True).clamp_min(1e-12), t.norm(dim=1, keepdim=True).clamp_min(1e-12)
    u, v = a / na, t / nt
    Z = (u @ v.T) / temperature
    keep = _keep(B, key)
    Zm = Z.masked_fill(~keep, -math.inf)
    lr, lc = torch.logsumexp(Zm, dim=1), torch.logsumexp(Zm, dim=0)
    d = torch.diagonal(Z)
    L = 0.5 * ((lr - d) + (lc - d)).sum()
    hits = int((Zm.argmax(dim=1) == torch.arange(B)).sum())         # argmax: the first maximum
    G = (weight / (2.0 * temperature)) * (keep.to(Z.dtype) * (torch.exp(Z - lr.unsqueeze(1)) + torch.exp(Z - lc.unsqueeze(0)))
                                          - 2.0 * torch.eye(B, dtype=Z.dtype))
    du, dv = G @ v, G.T @ u
    da = (du - (du * u).sum(dim=1, keepdim=True) * u) / na
    dt = (dv - (dv * v).sum(dim=1, keepdim=True) * v) / nt
    return dict(L=L, hits=hits, da=da, dt=dt)


def contrast_loss(a, t, key, temperature):
    """the same loss as an expression for torch autograd (F.normalize, masked logsumexp)"""
    u, v = torch.nn.functional.normalize(a, dim=1), torch.nn.functional.normalize(t, dim=1)
    Z = (u @ v.T) / temperature
    Zm = Z.masked_fill(~_keep(a.shape[0], key), -math.inf)
    d = torch.diagonal(Z)
    return 0.5 * ((torch.logsumexp(Zm, dim=1) - d) + (torch.logsumexp(Zm, dim=0) - d)).sum()


def draw_keys(B):
    """all distinct but: rows 0 and 2 share a key (B >= 3), rows 10 .. 19 share one (B >= 64)"""
    key = torch.arange(B, dtype=torch.int64)
    if B >= 3:
        key[2] = key[0]
    if B >= 64:
        key[10:20] = key[10]
    return key


_DRAWS = {}


def unsaturated_draw(B, H, T, seed=0):
    """(a, t, key): bf16-rounded fp32 rows whose positives are correlated just enough that the softmaxes neither saturate nor are
    flat: t = c a + noise with c = T (ln max(B - 1, 1) + 0.5), so the own logit leads the B - 1 others by about half a nat.
    Cached on (B, H, T, seed): both test files share one draw; nobody writes to it."""
    k = (B, H, T, seed)
    if k not in _DRAWS:
        g = torch.Generator().manual_seed(1000 * seed + 7 * B + H)
        a = torch.randn(B, H, generator=g)
        c = T * (math.log(max(B - 1, 1)) + 0.5)
        t = c * a + torch.randn(B, H, generator=g)
        _DRAWS[k] = (a.bfloat16().float(), t.bfloat16().float(), draw_keys(B))
    return _DRAWS[k]


@pytest.mark.parametrize("B", [1, 2, 5, 65])
def test_analytic_gradient_is_autograd_of_the_same_expression(B):
    g = torch.Generator().manual_seed(B)
    a, t = torch.randn(B, 24, generator=g, dtype=torch.float64), torch.randn(B, 24, generator=g, dtype=torch.float64)
    t = t + 0.3 * a
    key = draw_keys(B)
    if B == 2:
        key = torch.tensor([4, 4])                     # duplicate keys at every B > 1
    if B == 5:
        key[4] = key[3]
    for k in (key, None):
        for T, W in ((0.1, 1.3), (0.05, 0.7)):
            ref = contrast_reference(a, t, k, W, T)
            aa, tt = a.clone().requires_grad_(True), t.clone().requires_grad_(True)
            L = contrast_loss(aa, tt, k, T)
            (W * L).backward()
            assert abs(ref["L"].item() - L.item()) <= 1e-10 * max(1.0, abs(L.item()))
            assert (ref["da"] - aa.grad).abs().max().item() <= 1e-10 and (ref["dt"] - tt.grad).abs().max().item() <= 1e-10


def test_identities():
    B, H, T, W = 7, 16, 0.1, 1.3
    g = torch.Generator().manual_seed(3)
    a, t = torch.randn(B, H, generator=g, dtype=torch.float64), torch.randn(B, H, generator=g, dtype=torch.float64)
    none, distinct = contrast_reference(a, t, None, W, T), contrast_reference(a, t, torch.arange(B) * 3 + 1, W, T)
    assert none["L"].item() == distinct["L"].item() and none["hits"] == distinct["hits"]
    assert torch.equal(none["da"], distinct["da"]) and torch.equal(none["dt"], distinct["dt"])
    assert none["L"].item() > 0 and none["da"].abs().max().item() > 0
    same = contrast_reference(a, t, torch.full((B,), 5, dtype=torch.int64), W, T)
    assert same["L"].item() == 0.0 and same["hits"] == B and not same["da"].any() and not same["dt"].any()
    one = contrast_reference(a[:1], t[:1], None, W, T)
    assert one["L"].item() == 0.0 and one["hits"] == 1 and not one["da"].any() and not one["dt"].any()
    key = torch.tensor([0, 1, 0, 3, 4, 4, 6])
    ab, ba = contrast_reference(a, t, key, W, T), contrast_reference(t, a, key, W, T)
    assert abs(ab["L"].item() - ba["L"].item()) <= 1e-12 * ab["L"].item()
    assert torch.allclose(ab["da"], ba["dt"], rtol=0, atol=1e-12) and torch.allclose(ab["dt"], ba["da"], rtol=0, atol=1e-12)
    # a key takes a pair out of BOTH denominators: the loss differs from the unkeyed one
    assert ab["L"].item() != none["L"].item()


@pytest.mark.parametrize("T", [0.05, 0.1])
@pytest.mark.parametrize("H", [64, 768, 1024])
@pytest.mark.parametrize("B", [2, 3, 5, 64, 65, 257, 512])
def test_the_draw_is_unsaturated_and_fp32_resolves_it(B, H, T):
    """what makes the GPU file's parity bars meaningful on this draw: (1) the mean own-probability exp(Z_ii - lr_i) lies in
    [0.05, 0.95] - no softmax is saturated (gradients not tiny) or flat; (2) an fp32 torch evaluation of the restatement is within a
    tenth of the GPU bars of the fp64 one, so an fp32 kernel with sane summation has a factor of ten to spare"""
    a, t, key = unsaturated_draw(B, H, T)
    assert torch.equal(a, a.bfloat16().float()) and torch.equal(t, t.bfloat16().float())
    W = 1.3
    ref = contrast_reference(a.double(), t.double(), key, W, T)
    u, v = torch.nn.functional.normalize(a.double(), dim=1), torch.nn.functional.normalize(t.double(), dim=1)
    Zm = ((u @ v.T) / T).masked_fill(~_keep(B, key), -math.inf)
    own = torch.exp(torch.diagonal(Zm) - torch.logsumexp(Zm, dim=1)).mean().item()
    assert 0.05 <= own <= 0.95, own
    f32 = contrast_reference(a, t, key, W, T)
    e_l = abs(f32["L"].item() - ref["L"].item()) / ref["L"].item()
    e_g = max(((f32[k].double() - ref[k]).abs().max() / ref[k].abs().max()).item() for k in ("da", "dt"))
    print("draw B=%d H=%d T=%g: own-probability %.3f, fp32 vs fp64: L %.2e (bar / 10 = %.0e), gradient %.2e (bar / 10 = %.0e)"
          % (B, H, T, own, e_l, BAR_LOSS / 10, e_g, BAR_GRAD / 10))
    assert e_l <= BAR_LOSS / 10 and e_g <= BAR_GRAD / 10 and f32["hits"] == ref["hits"]


def test_the_draw_is_shared_and_keyed():
    a, t, key = unsaturated_draw(65, 64, 0.1)
    assert unsaturated_draw(65, 64, 0.1)[0] is a and not torch.equal(unsaturated_draw(65, 64, 0.1, seed=1)[0], a)
    assert key[2] == key[0] == 0 and (key[10:20] == 10).all() and key[20] == 20 and key.dtype == torch.int64
    assert torch.equal(draw_keys(2), torch.arange(2))


# ---- trainer.transcript_keys --------------------------------------------------------------------------------------------------------
def test_transcript_keys():
    tids = torch.tensor([[5, 9, 2, 0], [5, 9, 3, 0], [5, 9, 2, 0], [7, 0, 0, 0], [5, 9, 3, 0], [5, 9, 2, 1]])
    k = trainer.transcript_keys(tids)
    assert k.dtype == torch.int64 and tuple(k.shape) == (6,) and k.tolist() == [0, 1, 0, 3, 1, 5]
    assert trainer.transcript_keys(tids[:1]).tolist() == [0]
    assert trainer.transcript_keys(torch.cat([tids, tids])).tolist() == [0, 1, 0, 3, 1, 5] * 2        # the R-Drop batch: doubled keys
    assert trainer.rdrop_batch(dict(ids=tids, tids=tids, tkey=k))["tkey"].tolist() == k.tolist() * 2


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hipabi_binds_the_entry_points():
    hdr = open(os.path.join(conftest.ROOT, "include", "nbest_hip.h")).read()
    L = ctypes.CDLL(hipabi.LIB_PATH)
    for name in SYMBOLS:
        assert name in hipabi.EXPORTS, name
        assert re.search(r"\b(int|size_t) %s\(" % name, hdr), "include/nbest_hip.h does not declare %s" % name
        assert hasattr(L, name), name
    args = " ".join(re.search(r"int nbest_cls_contrast\(([^;]*)\);", hdr).group(1).split()).split(",")
    lib = hipabi.lib()
    assert len(args) == len(lib.nbest_cls_contrast.argtypes) == 17 and "const int64_t* key" in args[4]
    assert "K8c" in hdr and hasattr(hipabi, "cls_contrast")
    B, H = 5, 37
    assert lib.nbest_cls_contrast_ws_bytes(B, H) >= (2 * B * H + B * B) * 4


def test_the_entry_point_checks_its_arguments_on_the_host():
    """each refusal is made before the first launch: an error code and a message with no device in sight"""
    L = hipabi.lib()
    fake, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)
    ARG, DTYPE, WORKSPACE = -1, -3, -6

    def call(ha=fake, ht=fake, out=fake, ws=fake, B=4, H=64, weight=1.0, temperature=0.1, dtype=hipabi.F32, short=0):
        n = L.nbest_cls_contrast_ws_bytes(max(B, 1), max(H, 1)) - short
        return L.nbest_cls_contrast(ha, 64, ht, 64, null, weight, temperature, out, fake, fake, 0, B, H, dtype, ws, n, null)
    for kw, code in ((dict(ha=null), ARG), (dict(ht=null), ARG), (dict(out=null), ARG), (dict(ws=null), ARG), (dict(B=0), ARG),
                     (dict(H=0), ARG), (dict(B=4097), ARG), (dict(temperature=0.0), ARG), (dict(temperature=-1.0), ARG),
                     (dict(temperature=float("nan")), ARG), (dict(temperature=float("inf")), ARG), (dict(weight=-0.5), ARG),
                     (dict(weight=float("nan")), ARG), (dict(weight=float("inf")), ARG), (dict(short=1), WORKSPACE),
                     (dict(dtype=7), DTYPE)):
        assert call(**kw) == code, kw
        assert "cls_contrast" in hipabi.last_error(), kw


# ---- model -------------------------------------------------------------------------------------------------------------------------
def test_check_contrast():
    from nbest_amd.model import _check_contrast
    tids = torch.zeros(4, 3, dtype=torch.long)
    ok = _check_contrast(dict(weight=1, temperature=0.1), 4, tids)
    assert ok == dict(weight=1.0, temperature=0.1, keys=None)
    assert _check_contrast(dict(weight=0.0, temperature=2, keys=None), 4, tids)["weight"] == 0.0
    keys = torch.arange(4)
    assert _check_contrast(dict(weight=1.0, temperature=0.1, keys=keys), 4, tids)["keys"] is keys
    good = dict(weight=1.0, temperature=0.1)
    for bad, kw in ((dict(weight=-0.5, temperature=0.1), {}), (dict(weight=float("nan"), temperature=0.1), {}),
                    (dict(weight=float("inf"), temperature=0.1), {}), (dict(weight="x", temperature=0.1), {}),
                    (dict(weight=1.0, temperature=0.0), {}), (dict(weight=1.0, temperature=-1.0), {}),
                    (dict(weight=1.0, temperature=float("nan")), {}), (dict(weight=1.0, temperature=float("inf")), {}),
                    (dict(weight=1.0), {}), (dict(temperature=0.1), {}), (dict(good, margin=1.0), {}), (1.0, {}),
                    (dict(good, keys=torch.arange(3)), {}), (dict(good, keys=torch.arange(4, dtype=torch.int32)), {}),
                    (dict(good, keys=[0, 1, 2, 3]), {}), (good, dict(trans_input_ids=None)), (good, dict(adv=dict(epsilon=1.0)))):
        kw = dict(dict(trans_input_ids=tids), **kw)
        with pytest.raises(ValueError, match="contrast"):
            _check_contrast(bad, 4, **kw)


def test_the_autograd_bridge_has_no_such_argument():
    import inspect
    from nbest_amd.model import NBestSTCModel
    assert "contrast" in inspect.signature(NBestSTCModel.forward_backward).parameters
    assert "contrast" not in inspect.signature(NBestSTCModel.forward).parameters


def test_train_step_refuses_before_touching_anything(monkeypatch):
    batch = dict(ids=torch.zeros(2, 3, dtype=torch.long), tids=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="contrast_weight"):
        trainer.train_step(None, None, batch, contrast_weight=1.0, adv_epsilon=1.0)
    with pytest.raises(ValueError, match="contrast_weight"):
        trainer.train_step(None, None, dict(ids=batch["ids"]), contrast_weight=1.0)
    monkeypatch.setattr(trainer, "dist_info", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="contrast_weight"):
        trainer.train_step(None, None, batch, contrast_weight=1.0)
    assert trainer.contrast_args(None, 0.1, batch, 1.0, 2) is None
    monkeypatch.setattr(trainer, "dist_info", lambda: (0, 1))
    got = trainer.contrast_args(2, 0.05, dict(batch, tkey=torch.tensor([0, 0])), None, 1)
    assert got["weight"] == 2.0 and got["temperature"] == 0.05 and got["keys"].tolist() == [0, 0]
    assert trainer.contrast_args(2, 0.05, dict(tids=torch.tensor([[1, 2], [1, 3]])), None, 1)["keys"].tolist() == [0, 1]


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_default_and_combinations():
    plain = cli.parse_arguments(BASE)
    assert plain.contrastive_weight is None and plain.contrastive_temperature is None
    opt = cli.parse_arguments(BASE + CL)
    assert opt.contrastive_weight == 1.0 and opt.contrastive_temperature == 0.1
    assert cli.parse_arguments(BASE + CL + ["--contrastive_temperature", "0.05"]).contrastive_temperature == 0.05
    for optim in (["--optim_choice", "bertadam"], ["--optim_choice", "adam"], ["--optim_choice", "adamw", "--restated_adamw"]):
        opt = cli.parse_arguments(BASE + CL + optim + ["--ema_decay", "0.9", "--resume", "--add_l2_loss", "--freeze_layers", "1",
                                                       "--freeze_embeddings", "--rdrop_alpha", "0.5", "--dropout", "0.3"])
        assert opt.contrastive_weight == 1.0 and opt.ema_decay == 0.9 and opt.rdrop_alpha == 0.5 and opt.add_l2_loss
    assert cli.parse_arguments(BASE + CL + ["--distill_from", "t.pt"]).distill_from == "t.pt"
    assert cli.parse_arguments(BASE + CL + ["--n_layers", "12"]).n_accum_steps == 4          # gradient accumulation


def test_cli_exp_dir_moves_only_with_the_flag():
    plain = cli.exp_dir(cli.parse_arguments(BASE))
    assert plain.endswith("__cls_stc") and "cl_" not in plain.split("__cls_stc")[0].replace("cls_", "")
    assert cli.exp_dir(cli.parse_arguments(BASE + CL)) == plain + "__cl_1.0_0.1"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--contrastive_weight", "0.5", "--contrastive_temperature", "0.05"])) == plain + "__cl_0.5_0.05"
    assert cli.exp_dir(cli.parse_arguments(BASE + CL + ["--rdrop_alpha", "1.0", "--dropout", "0.3", "--ema_decay", "0.9"])) == \
        cli.exp_dir(cli.parse_arguments(BASE + ["--rdrop_alpha", "1.0", "--dropout", "0.3", "--ema_decay", "0.9"])) + "__cl_1.0_0.1"
    assert cli.exp_dir(cli.parse_arguments(BASE + ["--rdrop_alpha", "1.0", "--dropout", "0.3"])) == \
        cli.exp_dir(cli.parse_arguments(BASE + ["--dropout", "0.3"])) + "__rdrop_1.0"


def test_cli_refusals(tmp_path, monkeypatch, capsys):
    src = tmp_path / "in.txt"
    src.write_text("hello\n")
    mask = tmp_path / "mask.json"
    mask.write_text("[[1.0, 0.0]]")
    for bad, word in ((CL + ["--testing"], "--testing"), (CL + ["--predict", str(src)], "--predict"),
                      (CL + ["--head_importance", str(tmp_path / "imp.json")], "--head_importance"),
                      (CL + ["--adv_epsilon", "1.0"], "--adv_epsilon"), (CL + ["--dtype", "fp8w"], "fp8w"),
                      (CL + ["--train_head_mask", str(mask)], "--train_head_mask"),
                      (["--contrastive_weight", "0"], "--contrastive_weight"), (["--contrastive_weight", "-1"], "--contrastive_weight"),
                      (["--contrastive_weight", "nan"], "--contrastive_weight"), (["--contrastive_weight", "inf"], "--contrastive_weight"),
                      (CL + ["--contrastive_temperature", "0"], "--contrastive_temperature"),
                      (CL + ["--contrastive_temperature", "-0.1"], "--contrastive_temperature"),
                      (CL + ["--contrastive_temperature", "nan"], "--contrastive_temperature"),
                      (CL + ["--contrastive_temperature", "inf"], "--contrastive_temperature"),
                      (["--contrastive_temperature", "0.1"], "--contrastive_weight")):
        with pytest.raises(SystemExit):
            cli.parse_arguments(BASE + bad)
        assert word in capsys.readouterr().err, bad
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_arguments(BASE + CL)
    assert "negatives across ranks are not built" in capsys.readouterr().err
    assert cli.parse_arguments(BASE).contrastive_weight is None                # ... and fine without the flag
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.parse_arguments(BASE + CL).contrastive_weight == 1.0
