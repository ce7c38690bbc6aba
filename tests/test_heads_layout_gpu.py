"""GPU: the workspace and LDS layouts of the heads kernels (HeadsWs, HeadsLds in csrc/heads.hip).  A wrong offset must fail here, not
corrupt quietly: every mode runs on a private workspace of exactly nbest_heads_ws_bytes between two sentinel regions, and the R-Drop
call - the mode with the largest LDS layout - runs at exactly the 64 KB bound and is refused one row above it."""
import pytest
import torch

from test_distill_gpu import WIDE_SPACE

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = ("top", "bott", "final", "loss_parts", "dcls", "dWh", "dbh")
PAD = 4096                   # sentinel bytes on each side of the private workspace
KW = dict(drop_p=0.3, seed=4321, drop_stream=900)


def _inputs(ls, R, B, H, seed):
    gen = torch.Generator().manual_seed(seed)
    hidden = torch.randn(B, H, generator=gen)
    Wh, bh = torch.randn(R, H, generator=gen) * 0.05, torch.randn(R, generator=gen) * 0.05
    y = (torch.rand(B, ls.n_bottom, generator=gen) < 0.1).float()
    t_logits = torch.randn(B, R, generator=gen)
    t_top, t_bott, t_fin = torch.rand(B, ls.n_top, generator=gen), torch.rand(B, R - ls.n_top, generator=gen), torch.rand(B, ls.n_bottom, generator=gen)
    return [x.to(DEV).contiguous() for x in (hidden, Wh, bh, y, t_logits, t_top, t_bott, t_fin)]


@pytest.mark.parametrize("mode", ["plain", "kd", "kd_t", "rdrop"])
def test_private_workspace_of_exactly_ws_bytes_between_sentinels(mode):
    """wide space (the strided 70-column head), B = 2 (R-Drop: B2 = 2), H = 80, dropout 0.3: the call on a workspace of exactly
    nbest_heads_ws_bytes leaves the bytes before and after it untouched and returns the bits of the call on the shared scratch"""
    from nbest_amd import hipabi as hb
    from nbest_amd.config import LabelSpace
    ls = LabelSpace(WIDE_SPACE, ["s0", "a-x", "a-NONE"] + ["b-%d" % i for i in range(69)] + ["b-NONE"])
    dls = hb.DeviceLabelSpace(ls, DEV)
    B, H, R = 2, 80, dls.n_rows
    hidden, Wh, bh, y, t_logits, t_top, t_bott, t_fin = _inputs(ls, R, B, H, seed=17)
    call = {"plain": lambda **kw: hb.stc_heads(hidden, H, Wh, bh, dls, y, B, H, **kw),
            "kd": lambda **kw: hb.stc_heads_kd(hidden, H, Wh, bh, dls, y, t_top, t_bott, t_fin, 0.3, B, H, **kw),
            "kd_t": lambda **kw: hb.stc_heads_kd_t(hidden, H, Wh, bh, dls, y, t_logits, 0.3, 2.0, B, H, **kw),
            "rdrop": lambda **kw: hb.stc_heads_rdrop(hidden, H, Wh, bh, dls, y, 0.3, B, H, **kw)}[mode]
    n = hb.lib().nbest_heads_ws_bytes(B, R, H)
    buf = torch.full((PAD + n + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    private = dict(zip(KEYS, call(ws=buf[PAD:PAD + n], **KW)))
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == 0xA5).all()) and bool((buf[PAD + n:] == 0xA5).all()), "a heads kernel wrote outside its workspace"
    assert not bool((buf[PAD:PAD + n] == 0xA5).all())                    # the workspace was the one in use
    shared = dict(zip(KEYS, call(**KW)))
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(private[k], shared[k]), k
    assert bool(torch.isfinite(private["loss_parts"]).all())


def _rdrop_lds_bytes(H, R, n_heads, waves=8):
    """HeadsLds in kRDrop, restated: two CLS rows, logits + layers + the twin's logits, two sets of mask words, 3 + 1 partials per wave"""
    return 4 * (2 * H + 3 * R + 2 * (n_heads + 1) * ((H + 31) // 32) + 4 * waves)


def test_rdrop_runs_at_the_64_kb_bound_and_is_refused_above_it():
    """H = 2048 (the largest the entry point takes) and one single-bottom top + one head: R = 4000 rows need exactly 65536 bytes of LDS
    and the call succeeds; R = 4001 is refused with NBEST_ERR_SHAPE and nothing is launched (the pre-filled dWh and the private
    workspace keep their bytes)"""
    from nbest_amd import hipabi as hb
    from nbest_amd.config import LabelSpace
    B2, H = 2, 2048
    assert _rdrop_lds_bytes(H, 4000, 1) == 64 * 1024 and _rdrop_lds_bytes(H, 4001, 1) > 64 * 1024
    for R, fits in ((4000, True), (4001, False)):
        nk = R - 2
        ls = LabelSpace({0: [0], 1: list(range(1, nk + 1))}, ["s0"] + ["b-%d" % i for i in range(nk - 1)] + ["b-NONE"])
        dls = hb.DeviceLabelSpace(ls, DEV)
        assert dls.n_rows == R
        hidden, Wh, bh, y = _inputs(ls, R, B2, H, seed=R)[:4]
        dWh, dbh = torch.full((R, H), 7.0, device=DEV), torch.full((R,), 7.0, device=DEV)
        ws = torch.full((hb.lib().nbest_heads_ws_bytes(B2, R, H),), 0xA5, dtype=torch.uint8, device=DEV)
        if fits:
            out = dict(zip(KEYS, hb.stc_heads_rdrop(hidden, H, Wh, bh, dls, y, 0.3, B2, H, dWh=dWh, dbh=dbh, ws=ws, **KW)))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["loss_parts"]).all()) and out["loss_parts"][3].item() > 0
            assert not bool((dWh == 7.0).all())
        else:
            with pytest.raises(RuntimeError, match=r"stc_heads_rdrop failed \(-2\).*65548 bytes of LDS per block exceed 64 KB"):
                hb.stc_heads_rdrop(hidden, H, Wh, bh, dls, y, 0.3, B2, H, dWh=dWh, dbh=dbh, ws=ws, **KW)
            torch.cuda.synchronize()
            assert bool((dWh == 7.0).all()) and bool((dbh == 7.0).all()) and bool((ws == 0xA5).all())
