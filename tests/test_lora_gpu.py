"""GPU: LoRA on merged weights - nbest_lora_merge / nbest_lora_grad through the ABI on hand-built tables (per element against
fp64, derived bounds), the model / optimizer path (enable_lora, HipBertAdam's adapter arena, the adapter file) and the CLI.

Bounds, u = 2^-24 (fp32 round to nearest), whatever the order of the additions and with or without fma:
  merge  |d| <= (2 r + 2) u (|W0| + |s| sum_k |B_ik A_kj|)     r products, r additions, one scaling, one final addition
  dA     |d| <= (rows + 4) u |s| sum_i |B_ik g_ij|             rows products, rows - 1 additions, one scaling (+ slack of 4)
  dB     |d| <= (cols + 4) u |s| sum_j |g_ij A_kj|"""
import os
import shutil

import pytest
import torch

from conftest import GOLDEN
from test_infer_gpu import _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
GUARD = 256                 # elements of sentinel around every buffer
SENT = 12345.0

# (matrix rows, cols, first block row, block rows): the last one is the middle third of a 192 x 64 matrix (the fused-QKV case)
SHAPES = [(64, 64, 0, 64), (320, 192, 0, 320), (64, 256, 0, 64), (256, 64, 0, 256), (192, 64, 64, 64)]


def _up(n, a=64):
    return (n + a - 1) // a * a


class _Case:
    """buffers of one call: p / g hold the whole matrices between guards, base the packed blocks, ab the factors; every gap and
    guard holds SENT (p, p_lowp, g_ab, ws tail) so a stray write shows"""

    def __init__(self, ranks, scales, seed, b_zero=False):
        from nbest_amd import hipabi as hb
        gen = torch.Generator().manual_seed(seed)
        blocks, poff, boff, aoff = [], GUARD, GUARD, GUARD
        self.mats = []
        for (mr, mc, r0, br), rank, scale in zip(SHAPES, ranks, scales):
            blocks.append(dict(p_off=poff + r0 * mc, base_off=boff, a_off=aoff, b_off=_up(aoff + rank * mc) + 64, rows=br, cols=mc, rank=rank,
                               scale=scale))
            self.mats.append((poff, mr, mc))
            poff = _up(poff + mr * mc) + GUARD
            boff = _up(boff + br * mc) + GUARD
            aoff = _up(blocks[-1]["b_off"] + br * rank) + GUARD
        self.blocks = blocks
        self.p0 = torch.full((poff,), SENT)
        for o, mr, mc in self.mats:                                   # the matrices start as random values: non-block rows must survive
            self.p0[o:o + mr * mc] = torch.randn(mr * mc, generator=gen)
        self.g = torch.full((poff,), SENT)
        for o, mr, mc in self.mats:
            self.g[o:o + mr * mc] = torch.randn(mr * mc, generator=gen) * 0.1
        self.base = torch.full((boff,), SENT)
        self.ab = torch.full((aoff,), SENT)
        for b in blocks:
            n = b["rows"] * b["cols"]
            self.base[b["base_off"]:b["base_off"] + n] = torch.randn(n, generator=gen) * 0.05
            self.ab[b["a_off"]:b["a_off"] + b["rank"] * b["cols"]] = (torch.rand(b["rank"] * b["cols"], generator=gen) * 2 - 1) / b["cols"] ** 0.5
            self.ab[b["b_off"]:b["b_off"] + b["rows"] * b["rank"]] = 0.0 if b_zero else torch.randn(b["rows"] * b["rank"], generator=gen) * 0.3
        self.table = hb.LoraTable(blocks, DEV)
        self.d = {k: getattr(self, k).to(DEV) for k in ("p0", "g", "base", "ab")}

    def host(self, b):
        """(W0, A, B, g block) of a block in fp64 on the host"""
        n, r = b["rows"] * b["cols"], b["rank"]
        W0 = self.base[b["base_off"]:b["base_off"] + n].view(b["rows"], b["cols"]).double()
        A = self.ab[b["a_off"]:b["a_off"] + r * b["cols"]].view(r, b["cols"]).double()
        B = self.ab[b["b_off"]:b["b_off"] + b["rows"] * r].view(b["rows"], r).double()
        g = self.g[b["p_off"]:b["p_off"] + n].view(b["rows"], b["cols"]).double()
        return W0, A, B, g

    def block_mask(self, total):
        m = torch.zeros(total, dtype=torch.bool)
        for b in self.blocks:
            m[b["p_off"]:b["p_off"] + b["rows"] * b["cols"]] = True
        return m

    def factor_mask(self):
        m = torch.zeros(self.ab.numel(), dtype=torch.bool)
        for b in self.blocks:
            m[b["a_off"]:b["a_off"] + b["rank"] * b["cols"]] = True
            m[b["b_off"]:b["b_off"] + b["rows"] * b["rank"]] = True
        return m


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


CONFIGS = [((1,) * 5, (2.0,) * 5), ((5,) * 5, (0.37,) * 5), ((8,) * 5, (2.0,) * 5), ((64,) * 5, (0.37,) * 5), ((1, 5, 8, 64, 8), (2.0, 0.37, 2.0, 0.37, 2.0))]


# ---- merge ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks,scales", CONFIGS)
def test_merge_per_element(ranks, scales):
    from nbest_amd import hipabi as hb, lora
    c = _Case(ranks, scales, seed=sum(ranks))
    p = c.d["p0"].clone()
    plow = torch.full((p.numel(),), SENT, dtype=torch.bfloat16, device=DEV)
    hb.lora_merge(p, plow, c.d["base"], c.d["ab"], c.table)
    p2 = c.d["p0"].clone()
    hb.lora_merge(p2, None, c.d["base"], c.d["ab"], c.table)          # without the bf16 copy: the same fp32
    torch.cuda.synchronize()
    ph, pl = p.cpu(), plow.cpu()
    mask = c.block_mask(p.numel())
    assert torch.equal(_bits(ph[~mask]), _bits(c.p0[~mask])), "an element outside the blocks was written"
    assert torch.equal(_bits(pl[~mask]), _bits(torch.full((int((~mask).sum()),), SENT, dtype=torch.bfloat16)))
    assert torch.equal(_bits(pl[mask]), _bits(ph[mask].to(torch.bfloat16))), "bf16 copy is not the RNE of p"
    assert torch.equal(_bits(p2.cpu()), _bits(ph))
    for b in c.blocks:
        W0, A, B, _ = c.host(b)
        got = ph[b["p_off"]:b["p_off"] + b["rows"] * b["cols"]].view(b["rows"], b["cols"]).double()
        ref = lora.lora_reference_merge(W0, A, B, b["scale"])
        bound = (2 * b["rank"] + 2) * U * (W0.abs() + abs(b["scale"]) * (B.abs() @ A.abs()))
        worst = ((got - ref).abs() / bound).max().item()
        print("merge %dx%d r=%d s=%g: worst |d| / bound %.3f" % (b["rows"], b["cols"], b["rank"], b["scale"], worst))
        assert worst <= 1.0, (b, worst)


def test_merge_with_zero_B_gives_the_base_bits():
    from nbest_amd import hipabi as hb
    c = _Case((1, 5, 8, 64, 8), (2.0, 0.37, 2.0, 0.37, 2.0), seed=11, b_zero=True)
    base = c.d["base"].clone()
    for b in c.blocks:                                                # signed zeros and a denormal must come through as they are
        base[b["base_off"]:b["base_off"] + 3] = torch.tensor([-0.0, 0.0, 1e-42], device=DEV)
    p = c.d["p0"].clone()
    hb.lora_merge(p, None, base, c.d["ab"], c.table)
    torch.cuda.synchronize()
    for b in c.blocks:
        n = b["rows"] * b["cols"]
        assert torch.equal(_bits(p[b["p_off"]:b["p_off"] + n]), _bits(base[b["base_off"]:b["base_off"] + n])), b


# ---- projection -------------------------------------------------------------------------------------------------------------------------
def _grad(c, g, ws_fill):
    from nbest_amd import hipabi as hb
    gab = torch.full((c.ab.numel(),), SENT, device=DEV)
    nws = c.table.ws_bytes // 4
    ws = torch.full((nws + GUARD,), SENT, device=DEV)
    ws[:nws] = ws_fill
    hb.lora_grad(g, c.d["ab"], gab, c.table, ws[:nws].view(torch.uint8))
    torch.cuda.synchronize()
    assert torch.equal(_bits(ws[nws:]), _bits(torch.full((GUARD,), SENT, device=DEV))), "wrote past the workspace"
    return gab.cpu()


@pytest.mark.parametrize("ranks,scales", CONFIGS)
def test_grad_per_element(ranks, scales):
    from nbest_amd import lora
    c = _Case(ranks, scales, seed=100 + sum(ranks))
    g0 = c.d["g"].clone()
    gab = _grad(c, c.d["g"], 0.0)
    again = _grad(c, c.d["g"], float("nan"))                          # every partial the reduce reads is written first
    assert torch.equal(_bits(gab), _bits(again)), "two runs differ (one on a NaN-filled workspace)"
    assert torch.equal(_bits(c.d["g"]), _bits(g0)), "g was written"
    fm = c.factor_mask()
    assert torch.equal(_bits(gab[~fm]), _bits(torch.full((int((~fm).sum()),), SENT))), "wrote outside dA / dB"
    for b in c.blocks:
        _, A, B, g = c.host(b)
        r, s = b["rank"], b["scale"]
        dA = gab[b["a_off"]:b["a_off"] + r * b["cols"]].view(r, b["cols"]).double()
        dB = gab[b["b_off"]:b["b_off"] + b["rows"] * r].view(b["rows"], r).double()
        rA, rB = lora.lora_reference_grad(g, A, B, s)
        bA = (b["rows"] + 4) * U * abs(s) * (B.abs().t() @ g.abs())
        bB = (b["cols"] + 4) * U * abs(s) * (g.abs() @ A.abs().t())
        wA, wB = ((dA - rA).abs() / bA).max().item(), ((dB - rB).abs() / bB).max().item()
        print("grad %dx%d r=%d s=%g: worst |d| / bound dA %.4f dB %.4f" % (b["rows"], b["cols"], r, s, wA, wB))
        assert wA <= 1.0 and wB <= 1.0, (b, wA, wB)


def test_grad_of_a_one_hot_gradient():
    c = _Case((1, 5, 8, 64, 8), (2.0, 0.37, 2.0, 0.37, 2.0), seed=21)
    g = torch.zeros_like(c.d["g"])
    hot = []
    for n, b in enumerate(c.blocks):
        i, j = (7 * n + 3) % b["rows"], (11 * n + 5) % b["cols"]
        g[b["p_off"] + i * b["cols"] + j] = 1.5 + n
        hot.append((i, j, 1.5 + n))
    for o, mr, mc in c.mats:                                          # rows of the matrix outside the block must not leak in
        m = torch.ones(mr * mc, dtype=torch.bool)
        for b in c.blocks:
            if o <= b["p_off"] < o + mr * mc:
                m[b["p_off"] - o:b["p_off"] - o + b["rows"] * b["cols"]] = False
        g[o:o + mr * mc][m.to(DEV)] = 99.0
    gab = _grad(c, g, float("nan"))
    for b, (i, j, v) in zip(c.blocks, hot):
        _, A, B, _ = c.host(b)
        r, s = b["rank"], b["scale"]
        dA = gab[b["a_off"]:b["a_off"] + r * b["cols"]].view(r, b["cols"]).double()
        dB = gab[b["b_off"]:b["b_off"] + b["rows"] * r].view(b["rows"], r).double()
        wantA, wantB = s * B[i, :] * v, s * v * A[:, j]
        assert ((dA[:, j] - wantA).abs() <= 3 * U * wantA.abs()).all() and ((dB[i, :] - wantB).abs() <= 3 * U * wantB.abs()).all()
        dA[:, j] = 0.0
        dB[i, :] = 0.0
        assert not dA.any() and not dB.any(), "a one-hot gradient reached another row of dA / column of dB"


def test_argument_checks_launch_nothing():
    from nbest_amd import hipabi as hb
    c = _Case((8,) * 5, (2.0,) * 5, seed=31)
    p, gab = c.d["p0"].clone(), torch.full((c.ab.numel(),), SENT, device=DEV)
    ws = torch.full((c.table.ws_bytes // 4,), SENT, device=DEV)
    lib, st = hb.lib(), hb.stream_ptr()

    def merge(t, p_=p, base=c.d["base"], ab=c.d["ab"], dev=None):
        return lib.nbest_lora_merge(hb.ptr(p_), None, hb.ptr(base), hb.ptr(ab), t.host, hb.ptr(t.dev if dev is None else dev), t.n, st)

    def grad(t, ws_bytes=None, g=c.d["g"], gab_=gab):
        return lib.nbest_lora_grad(hb.ptr(g), hb.ptr(c.d["ab"]), hb.ptr(gab_), t.host, hb.ptr(t.dev), t.n, hb.ptr(ws),
                                   ws.numel() * 4 if ws_bytes is None else ws_bytes, st)

    for change, code in ((dict(rank=0), -1), (dict(rank=65), -1), (dict(cols=190), -2), (dict(stride=256), -2), (dict(p_off=c.blocks[1]["p_off"] + 2), -4)):
        bad = hb.LoraTable([c.blocks[0], dict(c.blocks[1], **change)] + c.blocks[2:], DEV, plan=False)
        good = hb.LoraTable(c.blocks, DEV)
        for i in range(bad.n):                                        # only the changed field differs from the planned table
            bad.host[i].tile_start, bad.host[i].ws_off = good.host[i].tile_start, good.host[i].ws_off
        assert merge(bad) == code and grad(bad) == code, change
    assert merge(c.table, p_=None) == -1 and merge(c.table, base=None) == -1 and merge(c.table, ab=None) == -1
    assert lib.nbest_lora_merge(hb.ptr(p), None, hb.ptr(c.d["base"]), hb.ptr(c.d["ab"]), c.table.host, None, c.table.n, st) == -1
    assert lib.nbest_lora_merge(hb.ptr(p), None, hb.ptr(c.d["base"]), hb.ptr(c.d["ab"]), None, hb.ptr(c.table.dev), c.table.n, st) == -1
    assert grad(c.table, g=None) == -1 and grad(c.table, gab_=None) == -1
    assert grad(c.table, ws_bytes=c.table.ws_bytes - 4) == -6 and "workspace" in hb.last_error()
    assert merge(c.table, p_=p[1:]) == -4                                # a buffer that is not 16-byte aligned
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(c.d["p0"])) and bool((gab == SENT).all()) and bool((ws == SENT).all())
    assert merge(c.table) == 0 and grad(c.table) == 0                 # ... and the same buffers are accepted as they are
    torch.cuda.synchronize()


# ---- model level ------------------------------------------------------------------------------------------------------------------------
def _fb(m, b):
    return m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], trans_input_ids=b["tids"], trans_seg_ids=b["tseg"], add_l2_loss=True)


def _merge_ok(st, arena, tag):
    from nbest_amd import lora
    for blk in st.blocks:
        A, B = st.view(st.p, blk.name + ".lora_A").cpu(), st.view(st.p, blk.name + ".lora_B").cpu()
        W0 = st.base_view(blk).cpu().double()
        ref = lora.lora_reference_merge(W0, A, B, st.scale)
        bound = (2 * st.rank + 2) * U * (W0.abs() + abs(st.scale) * (B.double().abs() @ A.double().abs()))
        got = arena.view(arena.p, blk.name)
        assert ((got.cpu().double() - ref).abs() <= bound).all(), (tag, blk.name)
        if arena.w16 is not None:
            assert torch.equal(_bits(arena.view(arena.w16, blk.name)), _bits(got.to(torch.bfloat16))), (tag, blk.name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L,layers,targets", [(2, None, ("query", "value")), (4, (2, 3), ("key", "attn_out", "ffn_down"))])
def test_training_path(L, layers, targets, dtype, labels):
    from nbest_amd import lora
    from nbest_amd.optim import HipBertAdam
    full, cfg, _ = _model(labels, L=L, dtype=dtype)
    m, _, _ = _model(labels, L=L, dtype=dtype)
    b = _batch(cfg, labels, 4, 48)
    full.train()
    m.train()
    pr0 = full.predict(b["ids"], seg_ids=b["seg"])
    o0 = _fb(full, b)
    st = m.enable_lora(8, 16, targets=targets, layers=layers, seed=2)
    p_start, base0 = m.arena.p.clone(), st.base.clone()
    # 1. the model is the model it was: scores of a training pass and of predict, to the bit; the dense gradient of every adapted
    #    matrix is the full model's (the freeze tests' guarantee); no base tensor has a .grad
    pr1 = m.predict(b["ids"], seg_ids=b["seg"])
    o1 = _fb(m, b)
    torch.cuda.synchronize()
    for k in ("top", "bott", "final"):
        assert torch.equal(_bits(o0[k]), _bits(o1[k])) and torch.equal(_bits(pr0[k]), _bits(pr1[k])), k
    assert torch.equal(_bits(o0["loss_parts"]), _bits(o1["loss_parts"]))
    for blk in st.blocks:
        assert torch.equal(_bits(m.arena.view(m.arena.g, blk.name)), _bits(full.arena.view(full.arena.g, blk.name))), blk.name
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not n.startswith("clf.")), n
    # 2. optimizer steps: the adapter gradients are the projection of arena.g (while B = 0, dA is exactly zero)
    opt = HipBertAdam(m, lr=5e-4, bert_lr=3e-5, lora_lr=2e-3)         # no schedule: a warm-up's first step has learning rate 0
    for step in range(3):
        if step:
            _fb(m, b)
        fac = st.p.clone()
        opt.step()
        torch.cuda.synchronize()
        for blk in st.blocks:
            A = fac[blk.a_off:blk.a_off + st.rank * blk.cols].view(st.rank, blk.cols).cpu().double()
            B = fac[blk.b_off:blk.b_off + blk.rows * st.rank].view(blk.rows, st.rank).cpu().double()
            g = m.arena.view(m.arena.g, blk.name).cpu().double()
            dA, dB = st.view(st.g, blk.name + ".lora_A").cpu().double(), st.view(st.g, blk.name + ".lora_B").cpu().double()
            rA, rB = lora.lora_reference_grad(g, A, B, st.scale)
            assert ((dA - rA).abs() <= (blk.rows + 4) * U * abs(st.scale) * (B.abs().t() @ g.abs())).all(), (step, blk.name)
            assert ((dB - rB).abs() <= (blk.cols + 4) * U * abs(st.scale) * (g.abs() @ A.abs().t())).all(), (step, blk.name)
            if step == 0:
                assert not dA.any() and dB.any(), blk.name
            else:
                assert dA.any(), blk.name
        _merge_ok(st, m.arena, "step %d" % step)
    # 3. after three steps: base and everything that is neither adapted nor a head is untouched; the blocks moved
    assert torch.equal(_bits(st.base), _bits(base0)) and opt.step_count == 3
    a = m.arena
    for s in a.slots:
        same = torch.equal(_bits(a.view(a.p, s.name)), _bits(p_start[s.offset:s.offset + s.numel].view(s.shape)))
        assert same == (s.name not in st.adapted and not s.name.startswith("clf.")), s.name
    # 4. the adapter file on a fresh model that holds the base reproduces the model; restore_base gives every bit back
    want = m.predict(b["ids"], seg_ids=b["seg"])
    sd = m.lora_state_dict()
    fresh, _, _ = _model(labels, L=L, dtype=dtype)
    fresh.load_lora(sd)
    got = fresh.predict(b["ids"], seg_ids=b["seg"])
    torch.cuda.synchronize()
    for k in ("top", "bott", "final"):
        assert torch.equal(_bits(want[k]), _bits(got[k])), k
    assert torch.equal(_bits(fresh.arena.p), _bits(a.p)) and fresh.lora is not None
    osd = opt.state_dict()
    assert set(osd["lora"]) == set(st.params) and all(v["next_m"].any() for v in osd["lora"].values())
    opt2 = HipBertAdam(fresh, lr=5e-4, bert_lr=3e-5, lora_lr=2e-3)
    opt2.load_state_dict(osd)
    assert torch.equal(_bits(fresh.lora.m), _bits(st.m)) and torch.equal(_bits(fresh.lora.v), _bits(st.v)) and opt2.step_count == 3
    m.disable_lora(restore_base=True)
    torch.cuda.synchronize()
    for s in a.slots:
        if not s.name.startswith("clf."):
            assert torch.equal(_bits(a.view(a.p, s.name)), _bits(p_start[s.offset:s.offset + s.numel].view(s.shape))), s.name
            if a.w16 is not None:
                assert torch.equal(_bits(a.view(a.w16, s.name)), _bits(a.view(a.p, s.name).to(torch.bfloat16))), s.name
    assert m.lora is None and all(p.requires_grad == ("pooler" not in n) for n, p in m.named_parameters())


def test_loss_goes_down_and_accumulation_is_linear(labels):
    from nbest_amd.optim import HipBertAdam
    m, cfg, _ = _model(labels, L=2, dtype=torch.bfloat16)
    b = _batch(cfg, labels, 4, 48)
    st = m.enable_lora(8, 16, targets=("query", "value", "ffn_up"))
    # the heads barely move (lr 1e-6): what brings the loss down is the factors.  BertAdam has no bias correction, so without a
    # warm-up its first steps are about 3 lr per element: 1e-4 keeps ten of them on one batch monotone
    opt = HipBertAdam(m, lr=1e-6, bert_lr=3e-5, lora_lr=1e-4)
    m.eval()
    first = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)["loss_parts"].sum().item()
    m.train()
    for _ in range(10):
        m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
        opt.step()
    m.eval()
    last = m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], need_grad=False)["loss_parts"].sum().item()
    print("loss on the fixed batch: %.4f -> %.4f after 10 LoRA steps" % (first, last))
    assert last < 0.7 * first
    factors = st.p.clone()
    assert factors[st.blocks[0].b_off:st.blocks[0].b_off + 64].any()              # B has left zero
    # gradient accumulation: the projection of g1 + g2 is the sum of the projections (same factors), to fp32 rounding
    m.train()
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"])
    st.project_grad(m.arena)
    one = st.g.clone()
    m.forward_backward(b["ids"], b["labels"], seg_ids=b["seg"], accumulate=True)
    st.project_grad(m.arena)
    two = st.g.clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(st.p), _bits(factors)) and one.any()
    ratio = (two.norm() / one.norm()).item()
    print("||proj(g1 + g2)|| / ||proj(g1)|| = %.3f" % ratio)
    assert 1.2 < ratio < 2.8                                           # two micro-batches under other dropout bits: about twice one


def test_refusals(labels):
    from nbest_amd.optim import HipAdam, HipBertAdam
    m, cfg, _ = _model(labels, L=2, dtype=torch.bfloat16)
    m.enable_lora(4, 8)
    with pytest.raises(RuntimeError, match="HipAdam on a model with LoRA enabled is not built"):
        HipAdam(m, kind="adamw", lr=1e-3)
    with pytest.raises(RuntimeError, match="ema_decay on a model with LoRA enabled is not built"):
        HipBertAdam(m, lr=1e-3, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="has LoRA enabled"):
        m.enable_lora(4, 8)
    m.disable_lora()
    adam = HipAdam(m, kind="adamw", lr=1e-3)
    m.enable_lora(4, 8)                                               # enabled after the optimizer was built: its step refuses
    with pytest.raises(RuntimeError, match="HipAdam on a model with LoRA enabled is not built"):
        adam.step_main()
    m.disable_lora()
    m.set_head_mask(torch.ones(2, 12))
    with pytest.raises(RuntimeError, match="under a head mask is not built"):
        m.enable_lora(4, 8)
    f8, _, _ = _model(labels, L=2, dtype=torch.bfloat16, fp8=True)
    with pytest.raises(RuntimeError, match="fp8w model is not built"):
        f8.enable_lora(4, 8)


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def _args(root, exp, extra, epochs="1"):
    return ["--dataset", "dstc2", "--dataroot", str(root), "--deviceId", "0", "--random_seed", "999", "--dropout", "0.3",
            "--bert_dropout", "0.1", "--lr", "5e-4", "--bert_lr", "3e-5", "--batchSize", "16", "--max_epoch", epochs, "--experiment", exp,
            "--add_segment_ids", "--label_space", os.path.join(GOLDEN, "label_space.json"),
            "--vocab", os.path.join(GOLDEN, "text_vocab.json"), "--encoder_layers", "2", "--n_best", "3", "--resume"] + extra


def test_cli_train_adapter_file_predict_and_resume(tmp_path, capsys):
    import nbest_amd  # noqa: F401
    from nbest_amd import cli, lora
    root = tmp_path / "data"
    root.mkdir()
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "train")
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), root / "valid")
    exp = str(tmp_path / "exp")
    flags = ["--lora_rank", "4", "--lora_targets", "value,query,ffn_down", "--lora_lr", "2e-3"]
    assert cli.main(_args(root, exp, flags)) == 0
    plain = cli.exp_dir(cli.parse_arguments(_args(root, exp, [])))
    d = cli.exp_dir(cli.parse_arguments(_args(root, exp, flags)))
    assert d == plain + "__lora_r4_a8_query+value+ffn_down" and os.path.isdir(d)
    log = open(os.path.join(d, "log.train")).read()
    n_fac = 2 * 4 * (2 * (768 + 768) + (768 + 3072))
    assert "LoRA: rank 4, alpha 8, targets query,value,ffn_down, lr 0.002" in log and "(%d in the factors of 6 blocks" % n_fac in log
    ck = torch.load(os.path.join(d, "last.pt"), weights_only=True)
    assert ck["lora"]["config"] == dict(rank=4, alpha=8.0, targets=["query", "value", "ffn_down"], layers=[0, 1])
    assert set(ck["optimizer"]["lora"]) == set(ck["lora"]["factors"]) and ck["optimizer"]["step"] == 2
    # model.pt / lora.pt are written on a new best valid F1 only; one tiny epoch may not get there: then they come from last.pt
    if os.path.exists(os.path.join(d, "model.pt")):
        assert os.path.exists(os.path.join(d, "lora.pt"))
    else:
        assert not os.path.exists(os.path.join(d, "lora.pt"))
        torch.save(ck["model"], os.path.join(d, "model.pt"))
        torch.save(lora.adapter_from_checkpoint(ck), os.path.join(d, "lora.pt"))
    ad = torch.load(os.path.join(d, "lora.pt"), weights_only=True)
    merged = torch.load(os.path.join(d, "model.pt"), weights_only=True)
    heads = {k for k in merged if k.startswith("clf.")}
    assert set(ad) == {"format", "rank", "alpha", "targets", "layers", "base_digest"} | set(ck["lora"]["factors"]) | heads
    assert os.path.getsize(os.path.join(d, "lora.pt")) < os.path.getsize(os.path.join(d, "model.pt")) // 20
    # --predict on the merged model.pt == --predict --lora_adapter on the base, byte for byte.  The scoring flags read
    # <exp_dir>/model.pt of the name without the lora_ part: one experiment root holds the merged file there, another the base
    src = tmp_path / "in.txt"
    shutil.copy(os.path.join(GOLDEN, "valid_head.txt"), src)
    base = dict(merged)
    base.update(ck["lora"]["base"])
    outs = []
    for name, sd, extra in (("merged", merged, []), ("base", base, ["--lora_adapter", os.path.join(d, "lora.pt")])):
        e2 = str(tmp_path / name)
        d2 = cli.exp_dir(cli.parse_arguments(_args(root, e2, [])))
        os.makedirs(d2)
        torch.save(sd, os.path.join(d2, "model.pt"))
        out = str(tmp_path / (name + ".pred"))
        assert cli.main(_args(root, e2, ["--predict", str(src), "--predict_output", out] + extra)) == 0
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 0
    # an already merged model.pt is not a base: the digest check says so, naming both
    e2 = str(tmp_path / "merged")
    with pytest.raises(SystemExit) as e:
        cli.main(_args(root, e2, ["--predict", str(src), "--lora_adapter", os.path.join(d, "lora.pt")]))
    assert ad["base_digest"] in str(e.value) and "base_digest" in str(e.value)
    # --resume continues (one more epoch), and refuses another configuration
    more = _args(root, exp, flags, epochs="2")
    d3 = cli.exp_dir(cli.parse_arguments(more))
    os.makedirs(d3)
    shutil.copy(os.path.join(d, "last.pt"), os.path.join(d3, "last.pt"))
    assert cli.main(more) == 0
    log = open(os.path.join(d3, "log.train")).read()
    assert "Resumed after epoch 00 (optimizer step 2)" in log and log.count("[Train]\tEpoch: ") == 1
    ck3 = torch.load(os.path.join(d3, "last.pt"), weights_only=True)
    assert ck3["epoch"] == 1 and ck3["optimizer"]["step"] == 4
    assert all(torch.equal(ck3["lora"]["base"][k], ck["lora"]["base"][k]) for k in ck["lora"]["base"])
    assert any(not torch.equal(ck3["lora"]["factors"][k], ck["lora"]["factors"][k]) for k in ck["lora"]["factors"])
    other = _args(root, exp, ["--lora_rank", "8"] + flags[2:], epochs="2")
    d4 = cli.exp_dir(cli.parse_arguments(other))
    os.makedirs(d4)
    shutil.copy(os.path.join(d, "last.pt"), os.path.join(d4, "last.pt"))
    with pytest.raises(SystemExit, match="resume with the --lora_\\* flags"):
        cli.main(other)
