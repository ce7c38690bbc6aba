"""GPU: sharpness-aware minimization (--sam_rho).  The K9s kernels (nbest_sam_norms, nbest_sam_perturb, nbest_sam_restore) on the
hand-built table of tests/optim_ref.py in guard-filled buffers, against the fp64 restatement of tests/sam_ref.py and their bit-exact
contracts; a SAM train_step on whole models decomposed, bit for bit, against twin models that run its stages one by one; what the
second pass's loss means (the oracle at the weights read back from the device); the refusals; the command line.  Every bound is the
issue's or tests/sam_ref.py's, never what the kernels give."""
import math
import os
import re
import shutil

import pytest
import torch

import optim_ref as R
import sam_ref as S
from conftest import GOLDEN, load_case, case_inputs

pytestmark = pytest.mark.gpu

WS_GUARD, BK_GUARD, LOW_GUARD = -4321.0, 777.25, 7.0
RULES = ("bertadam", "adam", "adamw")


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------
class KEnv:
    """the table on the device and the shared (never written) weights and gradient"""

    def __init__(self):
        from test_optim_kernels_gpu import Env
        e = Env()
        self.hb, self.L, self.tab, self.descs, self.n_t, self.n_b = e.hb, e.L, e.tab, e.descs, e.n_t, e.n_b
        self.cov, self.act = e.cov, e.act
        self.p0, self.g0 = S.state(self.tab)
        self.low0 = torch.where(self.cov, self.p0.to(torch.bfloat16), torch.tensor(LOW_GUARD, dtype=torch.bfloat16))

    def bufs(self, lowp=True, g=None):
        return dict(p=self.p0.clone().cuda(), g=(self.g0 if g is None else g).clone().cuda(),
                    backup=torch.full((self.tab.total,), BK_GUARD, device="cuda"), low=self.low0.clone().cuda() if lowp else None,
                    partial=torch.full((self.n_b + 8,), WS_GUARD, device="cuda"), clip=torch.full((2 + 8,), WS_GUARD, device="cuda"))

    def norms(self, b, eta):
        hb, L, P = self.hb, self.L, self.hb.ptr
        if eta is None:
            hb.check(L.nbest_bertadam_norms(P(b["g"]), P(self.descs), self.n_t, self.n_b, 0, self.n_b, P(b["partial"]), hb.stream_ptr()), "norms")
        else:
            hb.check(L.nbest_sam_norms(P(b["p"]), P(b["g"]), P(self.descs), self.n_t, self.n_b, eta, P(b["partial"]), hb.stream_ptr()), "sam_norms")
        hb.check(L.nbest_adam_clip_coef(P(b["partial"]), self.n_b, 0.0, P(b["clip"]), hb.stream_ptr()), "adam_clip_coef")

    def perturb(self, b, rho, eta):
        hb, P = self.hb, self.hb.ptr
        return self.L.nbest_sam_perturb(P(b["p"]), P(b["g"]), P(b["backup"]), P(b["low"]), P(self.descs), self.n_t, self.n_b,
                                        P(b["clip"][1:2]), rho, -1.0 if eta is None else eta, hb.stream_ptr())

    def restore(self, b):
        hb, P = self.hb, self.hb.ptr
        return self.L.nbest_sam_restore(P(b["p"]), P(b["backup"]), P(b["low"]), P(self.descs), self.n_t, self.n_b, hb.stream_ptr())

    def run(self, rho, eta, lowp, g=None):
        b = self.bufs(lowp, g)
        self.norms(b, eta)
        self.hb.check(self.perturb(b, rho, eta), "sam_perturb")
        torch.cuda.synchronize()
        return b, {k: (None if v is None else v.cpu()) for k, v in b.items()}


@pytest.fixture(scope="module")
def kenv():
    return KEnv()


MODES = [(S.RHO, None), (S.ASAM_RHO, S.ETA)]
MODE_IDS = ["plain", "adaptive"]


@pytest.mark.parametrize("lowp", [True, False], ids=["lowp", "nolowp"])
@pytest.mark.parametrize("rho,eta", MODES, ids=MODE_IDS)
def test_perturb_matches_fp64_per_element(kenv, rho, eta, lowp):
    """the block sums and the norm against fp64 (plain: optim_ref's chain bound; adaptive: sam_ref.ASAM_PARTIAL_K); every element of
    the new p against sam_reference fed the norm the device left, within K 2^-24 (|e_ref| + |p'_ref|), K = 1 plain (the fma's one
    rounding) / 4 adaptive (three more roundings on e); the radius | ||p' - p|| - rho | <= 2^-24 ||p'|| + 8 2^-24 rho (adaptive: of
    (p' - p) / t - the issue sets the same bound there, which is tighter than the triangle inequality's 2^-24 ||p' / t||); bit-exact: guards, gaps and the inactive tensor in p, backup and p_lowp, g, backup = old p, p_lowp = RNE bf16 of
    the value written, the guards behind the partials and the norm, a second run, and perturb + restore = nothing happened"""
    tab, act, cov = kenv.tab, kenv.act, kenv.cov
    b, a = kenv.run(rho, eta, lowp)
    _, a2 = kenv.run(rho, eta, lowp)
    for k in ("p", "backup", "partial", "clip") + (("low",) if lowp else ()):
        assert _same(a[k], a2[k]), "two runs differ in %s" % k
    # norms
    partial, norm = a["partial"][:kenv.n_b].double(), a["clip"][1].item()
    assert (a["partial"][kenv.n_b:] == WS_GUARD).all() and (a["clip"][2:] == WS_GUARD).all() and a["clip"][0].item() == 1.0
    ref_partial = R.ref_norms(tab, kenv.g0, 0.0)[0] if eta is None else S.adaptive_partials(tab, kenv.p0, kenv.g0, eta)
    worst = 0.0
    for t in tab.tensors:
        bound = R.partial_bound(t) if eta is None else S.ASAM_PARTIAL_K * S.EPS
        for blk in range(t.block_start, t.block_start + (t.numel + R.CHUNK - 1) // R.CHUNK):
            want = ref_partial[blk].item()
            if want == 0.0:
                assert partial[blk].item() == 0.0, (t.numel, blk)
                continue
            r = abs(partial[blk].item() - want) / want
            worst = max(worst, r / S.EPS)
            assert r <= bound, (t.numel, blk, r / S.EPS, bound / S.EPS)
    want_norm = math.sqrt(ref_partial.sum().item())
    nbound = R.coef_bound(None) if eta is None else 0.5 * S.ASAM_PARTIAL_K * S.EPS + 4 * S.EPS
    rn = abs(norm - want_norm) / want_norm
    print("sam %s: block sums worst %.2f x 2^-24, norm %.6f vs fp64 %.6f (%.2f x 2^-24, bound %.1f)"
          % ("plain" if eta is None else "adaptive", worst, norm, want_norm, rn / S.EPS, nbound / S.EPS))
    assert rn <= nbound
    # per element
    ref = S.sam_reference(tab, kenv.p0, kenv.g0, rho, eta, norm=norm)
    assert ref.s > 0.0
    K = 1 if eta is None else 4
    err = (a["p"].double() - ref.p).abs()[act]
    scale = (ref.e.abs() + ref.p.abs())[act]
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double()) / S.EPS
    print("sam %s: per-element worst %.3f x 2^-24 (|e| + |p'|), K = %d; moved elements %d of %d"
          % ("plain" if eta is None else "adaptive", ratio.max().item(), K, int((a["p"] != kenv.p0)[act].sum()), int(act.sum())))
    assert ratio.max().item() <= K
    assert int((a["p"] != kenv.p0)[act].sum()) > 0.5 * int(act.sum())
    # radius
    d = (a["p"].double() - kenv.p0.double())[act]
    if eta is not None:
        d = d / (kenv.p0.double().abs() + R.f32(eta))[act]
    radius = d.norm().item()
    rbound = S.EPS * a["p"].double()[act].norm().item() + 8 * S.EPS * rho
    print("sam %s: radius %.9f vs rho %s (off by %.3e, bound %.3e)" % ("plain" if eta is None else "adaptive", radius, rho, abs(radius - rho), rbound))
    assert abs(radius - rho) <= rbound
    # bit-exact contracts
    assert _same(a["g"], kenv.g0), "g was written"
    assert _same(a["p"][~act], kenv.p0[~act]) and (a["backup"][~act] == BK_GUARD).all()
    assert _same(a["backup"][act], kenv.p0[act])
    if lowp:
        assert _same(a["low"][~act], kenv.low0[~act]) and _same(a["low"][act], a["p"][act].to(torch.bfloat16))
        assert not _same(a["low"][act], kenv.low0[act])
    # restore
    kenv.hb.check(kenv.restore(b), "sam_restore")
    torch.cuda.synchronize()
    assert _same(b["p"].cpu(), kenv.p0) and (b["backup"].cpu()[~act] == BK_GUARD).all()
    assert not lowp or _same(b["low"].cpu(), kenv.low0)


@pytest.mark.parametrize("rho,eta", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", ["rho0", "zero_grad", "inf_grad"])
def test_nothing_moves_without_a_finite_positive_scale(kenv, case, rho, eta):
    """rho = 0, an all-zero gradient (norm 0) or one infinite gradient element (norm inf): p keeps every bit, no NaN appears, backup
    and p_lowp are written all the same (backup = p, p_lowp = bf16(p) on the active tensors, from a p_lowp that held other values)"""
    tab, act = kenv.tab, kenv.act
    g = kenv.g0.clone()
    if case == "zero_grad":
        g[kenv.cov] = 0.0
    if case == "inf_grad":
        g[tab.tensors[-1].offset + 12345] = math.inf
    b = kenv.bufs(True, g)
    b["low"][act.cuda()] = -3.0
    kenv.norms(b, eta)
    kenv.hb.check(kenv.perturb(b, 0.0 if case == "rho0" else rho, eta), "sam_perturb")
    torch.cuda.synchronize()
    a = {k: v.cpu() for k, v in b.items()}
    norm = a["clip"][1].item()
    assert (norm == 0.0) if case == "zero_grad" else (math.isinf(norm) if case == "inf_grad" else norm > 0)
    assert _same(a["p"], kenv.p0) and not bool(torch.isnan(a["p"]).any())
    assert _same(a["backup"][act], kenv.p0[act]) and (a["backup"][~act] == BK_GUARD).all()
    assert _same(a["low"][act], kenv.p0[act].to(torch.bfloat16)) and _same(a["low"][~act], kenv.low0[~act])
    assert _same(a["g"], g)


def test_argument_refusals_leave_the_buffers_untouched(kenv):
    """every refusal of include/nbest_hip.h returns NBEST_ERR_ARG (-1) and enqueues nothing: p, backup, p_lowp and the partials keep
    their bits"""
    hb, L, P = kenv.hb, kenv.L, kenv.hb.ptr
    b = kenv.bufs(True)
    kenv.norms(b, None)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in b.items()}
    null, st, d, n_t, n_b, inf, nan = P(None), hb.stream_ptr(), P(kenv.descs), kenv.n_t, kenv.n_b, math.inf, math.nan
    p, g, bk, low, part, norm = P(b["p"]), P(b["g"]), P(b["backup"]), P(b["low"]), P(b["partial"]), P(b["clip"][1:2])
    calls = [L.nbest_sam_perturb(*a) for a in (
        (null, g, bk, low, d, n_t, n_b, norm, 0.05, -1.0, st), (p, null, bk, low, d, n_t, n_b, norm, 0.05, -1.0, st),
        (p, g, null, low, d, n_t, n_b, norm, 0.05, -1.0, st), (p, g, bk, low, null, n_t, n_b, norm, 0.05, -1.0, st),
        (p, g, bk, low, d, n_t, n_b, null, 0.05, -1.0, st), (p, g, bk, low, d, 0, n_b, norm, 0.05, -1.0, st),
        (p, g, bk, low, d, n_t, 0, norm, 0.05, -1.0, st), (p, g, bk, low, d, n_t, -3, norm, 0.05, -1.0, st),
        (p, g, bk, low, d, n_t, n_b, norm, -0.05, -1.0, st), (p, g, bk, low, d, n_t, n_b, norm, inf, -1.0, st),
        (p, g, bk, low, d, n_t, n_b, norm, nan, -1.0, st), (p, g, bk, low, d, n_t, n_b, norm, 0.05, 0.0, st),
        (p, g, bk, low, d, n_t, n_b, norm, 0.05, inf, st), (p, g, bk, low, d, n_t, n_b, norm, 0.05, nan, st))]
    calls += [L.nbest_sam_norms(*a) for a in (
        (null, g, d, n_t, n_b, 0.01, part, st), (p, null, d, n_t, n_b, 0.01, part, st), (p, g, null, n_t, n_b, 0.01, part, st),
        (p, g, d, n_t, n_b, 0.01, null, st), (p, g, d, 0, n_b, 0.01, part, st), (p, g, d, n_t, 0, 0.01, part, st),
        (p, g, d, n_t, n_b, 0.0, part, st), (p, g, d, n_t, n_b, -1.0, part, st), (p, g, d, n_t, n_b, inf, part, st),
        (p, g, d, n_t, n_b, nan, part, st))]
    calls += [L.nbest_sam_restore(*a) for a in (
        (null, bk, low, d, n_t, n_b, st), (p, null, low, d, n_t, n_b, st), (p, bk, low, null, n_t, n_b, st), (p, bk, low, d, 0, n_b, st),
        (p, bk, low, d, n_t, 0, st))]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls), calls
    for k, v in b.items():
        assert _same(v, before[k]), k


# ---- whole model -----------------------------------------------------------------------------------------------------------------------
def _build_dropout(labels, dtype, dropout=0.1):
    """bert_L2 through test_model_gpu._build, then dropout switched on (heads, hidden states, attention probabilities)"""
    from test_model_gpu import _build
    meta, _ = load_case("bert_L2")
    m, b = _build(meta, labels, dtype)
    if dropout:
        m.dropout = dropout
        m.cfg.hidden_dropout_prob = m.cfg.attention_probs_dropout_prob = dropout
    return m, b, meta


def _optimizer(m, rule, **kw):
    from nbest_amd.optim import HipAdam, HipBertAdam
    if rule == "bertadam":
        return HipBertAdam(m, lr=1e-3, bert_lr=1e-4, warmup=0.1, t_total=40, **kw)
    return HipAdam(m, kind=rule, lr=1e-3, bert_lr=1e-4, l2=0.01 if rule == "adam" else 0.0, warmup=0.1, t_total=40, max_grad_norm=5.0, **kw)


def _images(a):
    """the weight images a forward / backward reads besides p: the bf16 copy, its transposed and packed forms"""
    return {k: getattr(a, k).clone() for k in ("w16", "w16t", "wpk", "wpkt") if getattr(a, k, None) is not None}


def _spy(opt):
    """record, around the optimizer's own methods, what a SAM train_step leaves between its stages"""
    rec, a = {}, opt.arena
    perturb, step = opt.sam_perturb, opt.step

    def sam_perturb(*args, **kw):
        rec["g1"] = a.g.clone()
        perturb(*args, **kw)
        rec["p_e"], rec["img_e"], rec["norm"] = a.p.clone(), _images(a), opt.sam_norm.clone()

    def do_step():
        rec["g2"] = a.g.clone()
        step()

    opt.sam_perturb, opt.step = sam_perturb, do_step
    return rec


def _fb(m, b, meta, **kw):
    return m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"] if meta["seg"] else None, trans_input_ids=b["tids"],
                              trans_seg_ids=b["tseg"], add_l2_loss=meta["add_l2"], **kw)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sam_step_decomposes_bit_for_bit(dtype, rule, labels):
    """bert_L2, dropout 0.1 on, rho 0.05: (a) arena.g after pass 1 is a plain forward_backward's; (b) the perturbed p and bf16 copy are
    the standalone kernels' on copies, the transposed / packed images a fresh refresh_compute_copy()'s on a twin holding p'; (c)
    arena.g after pass 2 is a plain forward_backward's on that twin (same seed, same step_counter: same dropout bits); (d) p, m, v
    and the images after the step are those of a twin at w whose arena.g is set to (c)'s and which steps plainly; both counters
    moved by 1, nothing is pending, the backup stays allocated.  No tolerance anywhere"""
    from nbest_amd import hipabi as hb
    from nbest_amd.trainer import train_step
    m, b, meta = _build_dropout(labels, dtype)
    opt = _optimizer(m, rule)
    assert opt.sam_backup is None and opt.sam_norm is None and not opt.sam_pending
    rec = _spy(opt)
    p0 = m.arena.p.clone()
    out = train_step(m, opt, b, add_l2_loss=meta["add_l2"], add_segment_ids=meta["seg"], sam_rho=0.05)
    torch.cuda.synchronize()
    assert m.step_counter == 1 and opt.step_count == 1 and not opt.sam_pending and opt.sam_backup is not None
    # (a)
    t1, _, _ = _build_dropout(labels, dtype)
    o1 = _fb(t1, b, meta)
    assert _same(t1.arena.g, rec["g1"]), "(a) pass 1's gradient is not the plain step's"
    for k in ("top", "bott", "final", "loss_parts"):
        assert _same(out[k], o1[k]), "(a) the returned %s is not the first pass's" % k
    # (b) standalone kernels on copies of w and of pass 1's gradient
    topt = _optimizer(t1, rule)
    a1, L, P, st = t1.arena, hb.lib(), hb.ptr, hb.stream_ptr()
    pc, low, bk = a1.p.clone(), None if a1.w16 is None else a1.w16.clone(), torch.zeros_like(a1.p)
    n0 = topt.parts[0][2]
    partial, clip = torch.zeros(n0 + topt.parts[1][2], device="cuda"), torch.zeros(2, device="cuda")
    for (descs, n_t, n_b, _), base in zip(topt.parts, (0, n0)):
        hb.check(L.nbest_bertadam_norms(P(rec["g1"]), P(descs), n_t, n_b, 0, n_b, P(partial[base:]), st), "norms")
    hb.check(L.nbest_adam_clip_coef(P(partial), partial.numel(), 0.0, P(clip), st), "clip")
    for descs, n_t, n_b, _ in topt.parts:
        hb.check(L.nbest_sam_perturb(P(pc), P(rec["g1"]), P(bk), P(low), P(descs), n_t, n_b, P(clip[1:2]), 0.05, -1.0, st), "perturb")
    assert _same(clip[1:2], rec["norm"]) and _same(out["sam_norm"], rec["norm"]) and rec["norm"].item() > 0
    assert _same(pc, rec["p_e"]) and not _same(pc, p0), "(b) the perturbed p is not the standalone kernel's"
    assert low is None or _same(low, rec["img_e"]["w16"])
    t2, _, _ = _build_dropout(labels, dtype)
    t2.arena.p.copy_(rec["p_e"])
    t2.arena.refresh_compute_copy()
    img2 = _images(t2.arena)
    assert sorted(img2) == sorted(rec["img_e"]) and (dtype == torch.float32 or len(img2) >= 2)
    for k, v in img2.items():
        assert _same(v, rec["img_e"][k]), "(b) image %s is not a fresh refresh's" % k
    # (c)
    o2 = _fb(t2, b, meta)
    assert _same(t2.arena.g, rec["g2"]) and not _same(rec["g2"], rec["g1"]), "(c) pass 2's gradient is not the plain step's at w + e"
    assert _same(out["sam_loss_parts"], o2["loss_parts"])
    # (d)
    a1.g.copy_(rec["g2"])
    topt.step()
    torch.cuda.synchronize()
    a = m.arena
    for k in ("p", "m", "v"):
        assert _same(getattr(a, k), getattr(a1, k)), "(d) %s after the step" % k
    for k, v in _images(a1).items():
        assert _same(v, getattr(a, k)), "(d) image %s after the step" % k
    print("decomposition %s: |p - p0| max %.3e after the step" % (rule, (a.p - p0).abs().max().item()))
    # (the first step of a warm-up schedule has learning rate 0: under bertadam / adamw p stays where it was, the moments move)
    assert not _same(a.m, torch.zeros_like(a.m)) and (rule != "adam" or (a.p - p0).abs().max().item() > 0)
    # the backup holds w on every trainable tensor (the pooler is never trainable: never written)
    for s in a.slots:
        if "pooler" not in s.name:
            assert _same(a.view(opt.sam_backup, s.name), a.view(p0, s.name)), s.name


OPTIONS = ["plain", "add_l2_loss", "rdrop_alpha", "teacher", "contrast_weight", "ema_decay", "frozen"]


@pytest.fixture(scope="module")
def teacher(labels):
    from test_model_gpu import _build
    meta, _ = load_case("bert_L2")
    meta = dict(meta, seed=meta["seed"] + 1)
    t, _ = _build(meta, labels, torch.bfloat16)
    t.eval()
    return t


def _frozen_names(m):
    return [n for n, _ in m.named_parameters() if n.startswith("bert_encoder.embeddings.") or n.startswith("bert_encoder.encoder.layer.0.")]


def _option_run(labels, option, teacher, sam_rho, dtype=torch.bfloat16, spy=False):
    from nbest_amd.trainer import train_step
    m, b, meta = _build_dropout(labels, dtype)
    if option == "frozen":
        for n, p in m.named_parameters():
            if n in set(_frozen_names(m)):
                p.requires_grad_(False)
    opt = _optimizer(m, "bertadam", **(dict(ema_decay=0.9) if option == "ema_decay" else {}))
    kw = dict(add_segment_ids=meta["seg"], add_l2_loss=option == "add_l2_loss")
    if option == "rdrop_alpha":
        kw["rdrop_alpha"] = 1.0
    if option == "teacher":
        kw.update(teacher=teacher, distill_alpha=0.5)
    if option == "contrast_weight":
        kw.update(contrast_weight=0.1, contrast_temperature=0.1)
    rec = _spy(opt) if spy else None
    out = train_step(m, opt, b, **kw, **({} if sam_rho is None else dict(sam_rho=sam_rho)))
    torch.cuda.synchronize()
    assert m.step_counter == 1 and opt.step_count == 1 and not opt.sam_pending
    return m, opt, out, rec


@pytest.mark.parametrize("option", OPTIONS)
def test_rho_zero_is_the_plain_step_and_sam_is_reproducible(option, labels, teacher):
    """(e) / (f): bf16, dropout 0.1, under each allowed option: with sam_rho = 0 through the API the whole step gives the plain
    train_step's p, m and v (and weight average), bit for bit; two runs at rho 0.05 give the same bits and differ from the plain
    step; with the embeddings and layer 0 frozen their p is untouched after the perturbation and after the step, and they are
    not in the norm"""
    plain, popt, pout, _ = _option_run(labels, option, teacher, None)
    zero, zopt, zout, _ = _option_run(labels, option, teacher, 0.0)
    assert popt.sam_backup is None and zopt.sam_backup is not None and "sam_norm" not in pout
    for k in ("p", "m", "v") + (("ema",) if option == "ema_decay" else ()):
        assert _same(getattr(zero.arena, k), getattr(plain.arena, k)), "rho 0: %s differs from the plain step's" % k
    for k in ("top", "loss_parts"):
        assert _same(zout[k], pout[k]), k
    assert _same(zout["sam_loss_parts"], zout["loss_parts"]) and zout["sam_norm"].item() > 0
    from nbest_amd.optim import warmup_linear
    r1, o1, out1, rec = _option_run(labels, option, teacher, 0.05, spy=True)
    r2, _, out2, _ = _option_run(labels, option, teacher, 0.05)
    for k in ("p", "m", "v") + (("ema",) if option == "ema_decay" else ()):
        assert _same(getattr(r1.arena, k), getattr(r2.arena, k)), "rho 0.05: two runs differ in %s" % k
    assert _same(out1["sam_loss_parts"], out2["sam_loss_parts"]) and _same(out1["sam_norm"], out2["sam_norm"])
    print("option %s: |p_sam - p_plain| max %.3e, |m_sam - m_plain| max %.3e, lr_mult of the step %.3f"
          % (option, (r1.arena.p - plain.arena.p).abs().max().item(), (r1.arena.m - plain.arena.m).abs().max().item(),
             warmup_linear(0, o1.t_total, o1.warmup)))
    # (the first BertAdam step of a warm-up schedule has learning rate 0: p stays, the moments carry the gradient)
    assert not _same(r1.arena.m, plain.arena.m) and not _same(out1["sam_loss_parts"], out1["loss_parts"])
    assert _same(out1["loss_parts"], pout["loss_parts"])                     # the first pass is the plain step's
    if option == "frozen":
        fresh, _, _ = _build_dropout(labels, torch.bfloat16)
        a, f = r1.arena, fresh.arena
        for n in _frozen_names(r1):
            assert _same(a.view(rec["p_e"], n), f.view(f.p, n)), "frozen %s moved under the perturbation" % n
            assert _same(a.view(a.p, n), f.view(f.p, n)) and _same(a.view(a.w16, n), f.view(f.w16, n)), n
            assert (a.view(o1.sam_backup, n) == 0).all(), "frozen %s was read into the backup" % n
        moved = [s.name for s in a.slots if not _same(a.view(rec["p_e"], s.name), f.view(f.p, s.name))]
        assert moved and not set(moved) & set(_frozen_names(r1))
        g = rec["g1"].double()
        live = torch.zeros(a.total, dtype=torch.bool, device="cuda")
        for s in a.slots:
            if s.name not in set(_frozen_names(r1)) and "pooler" not in s.name:
                live[s.offset:s.offset + s.numel] = True
        want = g[live].norm().item()
        assert abs(rec["norm"].item() - want) <= R.coef_bound(None) * want      # optim_ref's bound of the fixed-order total norm


# ---- meaning -----------------------------------------------------------------------------------------------------------------------------
def test_second_pass_loss_is_the_oracle_at_the_perturbed_weights(labels):
    """fp32, dropout 0, bert_L2, rho 0.05: sam_loss_parts against the oracle model's loss evaluated at the weights read back from the
    device after sam_perturb, within 1e-4 relative (the bar of test_model_gpu's losses), total and hard terms; and the sharpness
    sum(sam_loss_parts[:3]) - sum(loss_parts[:3]) is positive.  (The oracle alone, on the CPU, gives +104.59 on 210.28 for this case
    and rho: its own gradient, its own perturbation.)"""
    from nbest_amd.trainer import train_step
    from oracle import stc
    from test_model_gpu import _oracle_for
    m, b, meta = _build_dropout(labels, torch.float32, dropout=0.0)
    opt = _optimizer(m, "bertadam")
    perturb, seen = opt.sam_perturb, {}

    def sam_perturb(*args, **kw):
        perturb(*args, **kw)
        seen["sd"] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    opt.sam_perturb = sam_perturb
    out = train_step(m, opt, b, add_l2_loss=meta["add_l2"], add_segment_ids=meta["seg"], sam_rho=0.05)
    torch.cuda.synchronize()
    cfg, sd, batch = case_inputs(meta, labels)
    om = _oracle_for(cfg, sd, labels)
    t = {k: torch.from_numpy(v) for k, v in batch.items()}

    def oracle_loss():
        with torch.no_grad():
            top, bottoms, final, asr, tr = om(t["ids"], t["tids"], seg_ids=t["seg"], trans_seg_ids=t["tseg"])
            _, total, parts = stc.total_loss(top, bottoms, final, t["labels"], labels.top2bottom, stc.bottom2top_matrix(labels.top2bottom),
                                             asr, tr, meta["add_l2"])
        return total.item(), (parts["bottom_bce"] + parts["top_bce"] + parts["ce"]).item()

    total_w, hard_w = oracle_loss()
    om.load_state_dict(seen["sd"])
    total_e, hard_e = oracle_loss()
    lp, sp = out["loss_parts"].double().cpu(), out["sam_loss_parts"].double().cpu()
    print("sam meaning: at w device %.5f oracle %.5f; at w + e device %.5f oracle %.5f; sharpness device %.5f oracle (device weights) %.5f"
          % (lp.sum(), total_w, sp.sum(), total_e, (sp[:3].sum() - lp[:3].sum()), hard_e - hard_w))
    assert abs(lp.sum().item() - total_w) <= 1e-4 * abs(total_w)
    assert abs(sp.sum().item() - total_e) <= 1e-4 * abs(total_e)
    assert abs(sp[:3].sum().item() - hard_e) <= 1e-4 * abs(hard_e)
    assert sp[:3].sum().item() - lp[:3].sum().item() > 0 and hard_e - hard_w > 0


# ---- the rest ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_arenas_and_counters_unchanged(labels):
    """optimizer.sam_perturb (pending, sharded, LoRA, inside ema_weights(), a bad rho / eta) and train_step (adv_epsilon, a trainable
    head mask, an fp8w model, LoRA, a pending perturbation): the arenas keep their bits, step_counter and step_count stay"""
    from nbest_amd.trainer import train_step
    from test_model_gpu import _build
    m, b, meta = _build_dropout(labels, torch.bfloat16)
    opt = _optimizer(m, "bertadam", ema_decay=0.9)
    _fb(m, b, meta)
    torch.cuda.synchronize()
    a = m.arena
    snap = lambda: {k: getattr(a, k).clone() for k in ("p", "g", "m", "v", "w16", "w16t")}
    before, counters = snap(), (m.step_counter, opt.step_count)

    def unchanged():
        torch.cuda.synchronize()
        now = snap()
        return all(_same(now[k], before[k]) for k in before) and (m.step_counter, opt.step_count) == counters and not opt.sam_pending

    for kw in (dict(rho=-1.0), dict(rho=math.inf), dict(rho=math.nan), dict(rho=0.05, adaptive=True, eta=0.0),
               dict(rho=0.05, adaptive=True, eta=math.nan)):
        with pytest.raises(ValueError, match="sam_perturb"):
            opt.sam_perturb(**kw)
    with pytest.raises(RuntimeError, match="no perturbation"):
        opt.sam_restore()
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.sam_perturb(0.05)
    opt.sharded = True
    with pytest.raises(RuntimeError, match="sharded"):
        opt.sam_perturb(0.05)
    with pytest.raises(RuntimeError, match="sharded"):
        train_step(m, opt, b, sam_rho=0.05)
    opt.sharded = False
    with pytest.raises(ValueError, match="adv_epsilon"):
        train_step(m, opt, b, sam_rho=0.05, adv_epsilon=1.0)
    m.set_head_mask(torch.ones(m.cfg.num_hidden_layers, m.cfg.num_attention_heads), trainable=True)
    with pytest.raises(RuntimeError, match="head mask"):
        train_step(m, opt, b, sam_rho=0.05)
    m.set_head_mask(None)
    assert unchanged() and opt.sam_backup is None
    # pending: a second perturbation is refused, sam_restore() gives every bit back
    opt.sam_perturb(0.05)
    assert opt.sam_pending and not _same(a.p, before["p"])
    mid = a.p.clone()
    with pytest.raises(RuntimeError, match="pending"):
        opt.sam_perturb(0.05)
    with pytest.raises(RuntimeError, match="pending"):
        train_step(m, opt, b, sam_rho=0.05)
    with pytest.raises(RuntimeError, match="pending"):      # the average must not be swapped in under w + e
        with opt.ema_weights():
            pass
    torch.cuda.synchronize()
    assert _same(a.p, mid) and opt.sam_pending
    opt.sam_restore()
    assert unchanged()
    # LoRA (its own optimizer: no weight average) and fp8w
    lm, _, _ = _build_dropout(labels, torch.bfloat16)
    lopt = _optimizer(lm, "bertadam")
    lm.enable_lora(rank=4, alpha=8.0)
    _fb(lm, b, meta)
    torch.cuda.synchronize()
    lp, lg = lm.arena.p.clone(), lm.arena.g.clone()
    with pytest.raises(RuntimeError, match="LoRA"):
        lopt.sam_perturb(0.05)
    with pytest.raises(RuntimeError, match="LoRA"):
        train_step(lm, lopt, b, sam_rho=0.05)
    torch.cuda.synchronize()
    assert _same(lm.arena.p, lp) and _same(lm.arena.g, lg) and lm.step_counter == 1 and lopt.step_count == 0 and lopt.sam_backup is None
    f8, _ = _build(meta, labels, "fp8w")
    fopt = _optimizer(f8, "bertadam")
    fp = f8.arena.p.clone()
    with pytest.raises(RuntimeError, match="fp8w"):
        train_step(f8, fopt, b, sam_rho=0.05)
    assert _same(f8.arena.p, fp) and f8.step_counter == 0 and fopt.step_count == 0 and fopt.sam_backup is None


@pytest.mark.parametrize("rule", RULES)
def test_plain_step_after_a_sam_step(rule, labels):
    """bf16, dropout 0.1: a SAM step (adaptive, to run that path through a model), then a plain step; a twin that never ran one and
    is handed the state after the SAM step (p, m, v, both counters) gives the same bits from the same plain step.  Without sam_rho
    the backup is never allocated"""
    from nbest_amd.trainer import train_step
    m, b, meta = _build_dropout(labels, torch.bfloat16)
    opt = _optimizer(m, rule)
    kw = dict(add_l2_loss=meta["add_l2"], add_segment_ids=meta["seg"])
    out = train_step(m, opt, b, sam_rho=0.5, sam_adaptive=True, sam_eta=0.01, **kw)
    assert out["sam_norm"].item() > 0 and not _same(out["sam_loss_parts"], out["loss_parts"])
    t, _, _ = _build_dropout(labels, torch.bfloat16)
    topt = _optimizer(t, rule)
    for k in ("p", "m", "v"):
        getattr(t.arena, k).copy_(getattr(m.arena, k))
    t.arena.refresh_compute_copy()
    t.step_counter, topt.step_count = m.step_counter, opt.step_count
    if topt.__dict__.get("scheduler") is not None:
        topt.scheduler.last_epoch = opt.scheduler.last_epoch
    for k, v in _images(t.arena).items():
        assert _same(v, getattr(m.arena, k)), "image %s after the SAM step is not a fresh refresh's" % k
    o1, o2 = train_step(m, opt, b, **kw), train_step(t, topt, b, **kw)
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "g", "w16"):
        assert _same(getattr(m.arena, k), getattr(t.arena, k)), k
    assert _same(o1["loss_parts"], o2["loss_parts"]) and "sam_norm" not in o1
    assert m.step_counter == t.step_counter == 2 and opt.step_count == topt.step_count == 2
    assert topt.sam_backup is None and opt.sam_backup is not None


def test_cli_sam_rho(tmp_path):
    """one epoch on valid_head.txt (the tiny set-up of test_cli_rdrop_alpha) with --sam_rho 0.05: the __sam_0.05 directory, the flag
    named once in log.train, a [SAM] line with a finite sharpness and gradient norm, last.pt with the keys of a plain run (which
    has neither line); --testing is refused with the flag"""
    import nbest_amd  # noqa: F401
    from nbest_amd import cli
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    plain = ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
             "--bert_dropout", "0.1", "--optim_choice", "bertadam", "--lr", "1e-2", "--bert_lr", "1e-4", "--warmup_proportion", "0.1",
             "--batchSize", "2", "--max_epoch", "1", "--experiment", str(tmp_path / "exp"), "--pre_trained_model", "bert",
             "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
             "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "1", "--n_best", "5", "--resume"]
    keys = {}
    for name, extra, tail in (("plain", [], ""), ("sam", ["--sam_rho", "0.05"], "__sam_0.05")):
        args = plain + extra
        assert cli.main(args) == 0
        d = cli.exp_dir(cli.parse_arguments(args))
        assert d == cli.exp_dir(cli.parse_arguments(plain)) + tail and os.path.isdir(d)
        keys[name] = sorted(torch.load(os.path.join(d, "last.pt"), weights_only=True).keys())
        log = open(os.path.join(d, "log.train")).read().split("\n")
        train = [l for l in log if l.startswith("[Train]\tEpoch: 00")]
        assert len(train) == 1
        loss = float(re.search(r"Loss: ([0-9.]+)", train[0]).group(1))
        assert 0.0 < loss < 1e4
        lines = [l for l in log if l.startswith("[SAM]")]
        named = [l for l in log if l.startswith("SAM: rho")]
        if name == "plain":
            assert not lines and not named
            continue
        assert len(named) == 1 and named[0].startswith("SAM: rho 0.05;")
        assert len(lines) == 1
        sharp, gnorm = re.match(r"\[SAM\]\tEpoch: 00\tSharpness: (-?[0-9.]+)\tGradNorm: ([0-9.]+)$", lines[0]).groups()
        assert math.isfinite(float(sharp)) and math.isfinite(float(gnorm)) and float(gnorm) > 0
        print("cli %s: %s | %s" % (name, train[0], lines[0]))
        with pytest.raises(SystemExit):
            cli.main(args + ["--testing"])
    assert keys["sam"] == keys["plain"]
