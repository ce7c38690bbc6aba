"""LoRA on merged weights (Hu et al., 2022): the encoder stays frozen and a rank-r update dW = (alpha / r) B A is trained on a
few of its matrices.  The arena keeps the MERGED matrix W = W0 + s B A, so the encoder, every inference path and ``model.pt`` are
exactly what they are without LoRA; the factors live in an adapter arena of their own and meet the encoder's arenas in two
kernels per optimizer step (include/nbest_hip.h K9l): nbest_lora_grad projects the dense gradient the weight-gradient GEMMs
left in ``arena.g`` onto the factors (dA = s B^T dW, dB = s dW A^T - what autograd gives for x -> (W0 + s B A) x), and after
BertAdam has updated them nbest_lora_merge rewrites the adapted blocks of ``arena.p`` / ``arena.w16`` from the base copy.

A *block* is a contiguous row range of one arena matrix: ``query`` / ``key`` / ``value`` are the three row blocks of the fused
[3H, H] matrix and can be adapted on their own.
"""
import hashlib
import math

import torch
import torch.nn as nn

from . import hipabi as hb

ALIGN = 64          # elements: every A, B and base block starts 256-byte aligned
FORMAT = "nbest_amd.lora.v1"

# target -> tensor name inside "bert_encoder.encoder.layer.<l>."; the order of the block table within a layer
TARGETS = (("query", "attention.self.query.weight"), ("key", "attention.self.key.weight"), ("value", "attention.self.value.weight"),
           ("attn_out", "attention.output.dense.weight"), ("ffn_up", "intermediate.dense.weight"), ("ffn_down", "output.dense.weight"))
TARGET_NAMES = tuple(t for t, _ in TARGETS)


def parse_targets(targets):
    """'query,value' or a sequence of names -> the tuple of targets in table order; unknown, repeated or no names raise ValueError"""
    if isinstance(targets, str):
        targets = [t.strip() for t in targets.split(",") if t.strip()]
    targets = list(targets)
    if not targets:
        raise ValueError("nbest_amd lora: no targets (choose from %s)" % ", ".join(TARGET_NAMES))
    for t in targets:
        if t not in TARGET_NAMES:
            raise ValueError("nbest_amd lora: unknown target %r (choose from %s)" % (t, ", ".join(TARGET_NAMES)))
    if len(set(targets)) != len(targets):
        raise ValueError("nbest_amd lora: a target is named twice in %s" % (targets,))
    return tuple(t for t in TARGET_NAMES if t in targets)


def check_config(rank, alpha, L, layers=None):
    """(rank, alpha, layers) checked: 1 <= rank <= 64, alpha finite and > 0, layers a sorted tuple inside 0 .. L - 1 (None: all)"""
    if int(rank) != rank or not 1 <= int(rank) <= hb.LORA_MAX_RANK:
        raise ValueError("nbest_amd lora: rank must be an integer in 1 .. %d, not %r" % (hb.LORA_MAX_RANK, rank))
    alpha = float(alpha)
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise ValueError("nbest_amd lora: alpha must be finite and > 0, not %r" % (alpha,))
    layers = tuple(range(L)) if layers is None else tuple(sorted(set(int(l) for l in layers)))
    if not layers or layers[0] < 0 or layers[-1] >= L:
        raise ValueError("nbest_amd lora: layers must be a non-empty subset of 0 .. %d, not %r" % (L - 1, layers))
    return int(rank), alpha, layers


def exp_dir_part(rank, alpha, targets):
    """what --lora_rank adds to exp_dir: lora_r<R>_a<A>_<targets joined by '+'>"""
    return "lora_r%d_a%g_%s" % (rank, alpha, "+".join(parse_targets(targets)))


def _up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


class LoraBlock:
    __slots__ = ("name", "layer", "target", "rows", "cols", "p_off", "base_off", "a_off", "b_off")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class LoraState:
    """the adapter side of a model with LoRA enabled: the block table, the adapter arena (``p``, ``g``, and ``m`` / ``v`` once an
    optimizer is built; A [r, cols] and B [rows, r] of every block, each aligned to 64 elements), the base buffer (a packed copy of
    the adapted blocks only), the descriptor tables, and ``params``: name -> nn.Parameter views into ``p`` with ``.grad`` views into
    ``g``, as ParamArena's."""

    def __init__(self, arena, rank, alpha, targets=("query", "value"), layers=None, device=None):
        L = arena.cfg.num_hidden_layers
        self.rank, self.alpha, self.layers = check_config(rank, alpha, L, layers)
        self.targets = parse_targets(targets)
        self.scale = self.alpha / self.rank
        self.device = torch.device(arena.device if device is None else device)
        self.blocks, off, boff = [], 0, 0
        for l in self.layers:
            for t, tn in TARGETS:
                if t not in self.targets:
                    continue
                s = arena.by_name["bert_encoder.encoder.layer.%d.%s" % (l, tn)]
                rows, cols = s.shape
                b = LoraBlock(name=s.name, layer=l, target=t, rows=rows, cols=cols, p_off=s.offset, base_off=boff, a_off=off,
                              b_off=_up(off + self.rank * cols))
                off = _up(b.b_off + rows * self.rank)
                boff = _up(boff + rows * cols)
                self.blocks.append(b)
        self.total, self.base_total = off, boff
        self.adapted = frozenset(b.name for b in self.blocks)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.p = torch.zeros(self.total, **f32)
        self.g = torch.zeros(self.total, **f32)
        self.m = self.v = None
        self.base = torch.zeros(self.base_total, **f32)
        self.table = hb.LoraTable([dict(p_off=b.p_off, base_off=b.base_off, a_off=b.a_off, b_off=b.b_off, rows=b.rows, cols=b.cols,
                                        rank=self.rank, scale=self.scale) for b in self.blocks], self.device)
        self.ws = torch.empty(max(self.table.ws_bytes, 16), dtype=torch.uint8, device=self.device) if self.device.type == "cuda" else None
        self.slots = []                          # (name, offset, shape) of the adapter tensors, in arena order
        self.params = {}
        for b in self.blocks:
            for suffix, o, shape in ((".lora_A", b.a_off, (self.rank, b.cols)), (".lora_B", b.b_off, (b.rows, self.rank))):
                self.slots.append((b.name + suffix, o, shape))
                prm = nn.Parameter(self.view(self.p, b.name + suffix, o, shape))
                prm.grad = self.view(self.g, b.name + suffix, o, shape)
                self.params[b.name + suffix] = prm
        self._by_name = {n: (o, shape) for n, o, shape in self.slots}

    # ---- views ---------------------------------------------------------------------------------
    def view(self, buf, name, off=None, shape=None):
        if off is None:
            off, shape = self._by_name[name]
        return buf[off:off + shape[0] * shape[1]].view(shape)

    def base_view(self, b):
        return self.base[b.base_off:b.base_off + b.rows * b.cols].view(b.rows, b.cols)

    @property
    def n_trainable(self):
        return sum(shape[0] * shape[1] for _, _, shape in self.slots)

    def config(self):
        return dict(rank=self.rank, alpha=self.alpha, targets=list(self.targets), layers=list(self.layers))

    # ---- initial values / base -----------------------------------------------------------------
    def init_factors(self, seed=0):
        """A ~ U(-1/sqrt(in), 1/sqrt(in)) (kaiming_uniform_(a = sqrt(5)): peft's default), B = 0"""
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        self.p.zero_()
        for b in self.blocks:
            bound = 1.0 / math.sqrt(b.cols)
            a = (torch.rand(self.rank, b.cols, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
            self.view(self.p, b.name + ".lora_A").copy_(a)

    def capture_base(self, arena):
        """the adapted blocks of ``arena.p`` as they are now become the base W0"""
        for b in self.blocks:
            self.base_view(b).copy_(arena.view(arena.p, b.name))

    def restore_base(self, arena):
        for b in self.blocks:
            arena.view(arena.p, b.name).copy_(self.base_view(b))

    def base_digest(self):
        """SHA-1 of the fp32 little-endian bytes of the base blocks, in table order"""
        h = hashlib.sha1()
        for b in self.blocks:
            h.update(self.base_view(b).detach().cpu().contiguous().numpy().astype("<f4", copy=False).tobytes())
        return h.hexdigest()

    # ---- the two kernels -----------------------------------------------------------------------
    def merge(self, arena):
        hb.lora_merge(arena.p, arena.w16, self.base, self.p, self.table)

    def project_grad(self, arena):
        hb.lora_grad(arena.g, self.p, self.g, self.table, self.ws)

    # ---- optimizer descriptors (nbest_tensor_desc, as ParamArena.build_descs) -------------------
    def build_descs(self, lr, wd=0.01):
        chunk = hb.lib().nbest_bertadam_chunk()
        arr = (hb.TensorDesc * max(len(self.slots), 1))()
        blk = 0
        for d, (_, off, shape) in zip(arr, self.slots):
            d.offset, d.numel, d.lr, d.wd, d.active, d.block_start = off, shape[0] * shape[1], lr, wd, 1, blk
            blk += (d.numel + chunk - 1) // chunk
        dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        return dev, len(self.slots), blk


# ---- host restatements (fp64) --------------------------------------------------------------------
def lora_reference_merge(base, A, B, scale):
    """W0 + scale B A in fp64: base [rows, cols], A [r, cols], B [rows, r]"""
    return base.double() + float(scale) * (B.double() @ A.double())


def lora_reference_grad(g, A, B, scale):
    """(dA, dB) in fp64 of the dense gradient g [rows, cols]: dA = scale B^T g, dB = scale g A^T"""
    g = g.double()
    return float(scale) * (B.double().t() @ g), float(scale) * (g @ A.double().t())


# ---- the model's methods (model.NBestSTCModel forwards to these) -----------------------------------
def enable(model, rank, alpha, targets=("query", "value"), layers=None, seed=0, _under_mask=False):
    if getattr(model, "lora", None) is not None:
        raise RuntimeError("nbest_amd: enable_lora on a model that has LoRA enabled (call disable_lora first)")
    if model.fp8_forward:
        raise RuntimeError("nbest_amd: enable_lora on an fp8w model is not built (the e4m3 weight copies are quantised from the "
                           "full master after every step; LoRA under fp8 has not been measured)")
    if model.head_mask is not None and not _under_mask:
        raise RuntimeError("nbest_amd: enable_lora under a head mask is not built (call set_head_mask(None) first)")
    st = LoraState(model.arena, rank, alpha, targets, layers)
    st.init_factors(seed)
    st.capture_base(model.arena)
    st.saved_flags = [(p, p.requires_grad) for _, p in model._params]
    for n, p in model._params:
        if not n.startswith("clf."):
            p.requires_grad_(False)
    model.lora = st
    model._plans.clear()
    return st


def disable(model, restore_base=False):
    st = model.lora
    if st is None:
        raise RuntimeError("nbest_amd: disable_lora on a model without LoRA")
    if restore_base:
        st.restore_base(model.arena)
        model.arena.refresh_compute_copy()
    for p, f in st.saved_flags:
        p.requires_grad_(f)
    model.lora = None
    model._plans.clear()


def state_dict(model):
    st = model.lora
    if st is None:
        raise RuntimeError("nbest_amd: lora_state_dict on a model without LoRA")
    sd = dict(format=FORMAT, base_digest=st.base_digest(), **st.config())
    for n, _, _ in st.slots:
        sd[n] = st.view(st.p, n).detach().cpu().clone()
    a = model.arena
    for s in a.slots:
        if s.name.startswith("clf."):
            sd[s.name] = a.view(a.p, s.name).detach().cpu().clone()
    return sd


def load(model, sd, keep=True):
    """apply an adapter file to a model that holds the base weights: enable LoRA with the file's configuration (or check it
    against the one enabled), check shapes and the base digest, install factors and heads, merge.  ``keep=False``: LoRA is
    switched off again afterwards - the model is a plain one with merged weights (what --lora_adapter scores; works under a
    head mask, since nothing trains)"""
    if sd.get("format") != FORMAT:
        raise ValueError("nbest_amd load_lora: not an adapter file (format %r, expected %r)" % (sd.get("format"), FORMAT))
    rank, alpha, layers = check_config(sd["rank"], sd["alpha"], model.cfg.num_hidden_layers, sd["layers"])
    targets = parse_targets(sd["targets"])
    fresh = model.lora is None
    if fresh:
        enable(model, rank, alpha, targets, layers, _under_mask=not keep)
    st = model.lora
    try:
        if (st.rank, st.alpha, st.targets, st.layers) != (rank, alpha, targets, layers):
            raise ValueError("nbest_amd load_lora: the file's configuration %r differs from the enabled one %r"
                             % (dict(rank=rank, alpha=alpha, targets=list(targets), layers=list(layers)), st.config()))
        a = model.arena
        heads = [s for s in a.slots if s.name.startswith("clf.")]
        for n, shape in [(n, shape) for n, _, shape in st.slots] + [(s.name, s.shape) for s in heads]:
            if n not in sd:
                raise ValueError("nbest_amd load_lora: the file lacks %s" % n)
            if tuple(sd[n].shape) != tuple(shape):
                raise ValueError("nbest_amd load_lora: shape mismatch for %s: %s vs %s" % (n, tuple(sd[n].shape), tuple(shape)))
        have = st.base_digest()
        if have != sd["base_digest"]:
            raise ValueError("nbest_amd load_lora: the adapter was trained on other base weights: base_digest of the file %s, of "
                             "this model %s (an already merged model.pt is not a base)" % (sd["base_digest"], have))
    except Exception:
        if fresh:
            disable(model)
        raise
    for n, _, _ in st.slots:
        st.view(st.p, n).copy_(sd[n])
    for s in heads:
        a.view(a.p, s.name).copy_(sd[s.name])
    if a.w16 is not None:
        for s in heads:
            a.view(a.w16, s.name).copy_(a.view(a.p, s.name))
    merge(model)
    if not keep:
        disable(model)


def checkpoint_entry(model):
    """the ``lora`` entry of last.pt: configuration, factors and base blocks (the moments are in the optimizer's state)"""
    st = model.lora
    return dict(config=st.config(), factors={n: st.view(st.p, n).detach().cpu().clone() for n, _, _ in st.slots},
                base={b.name: st.base_view(b).detach().cpu().clone() for b in st.blocks})


def restore_checkpoint(model, entry):
    """base blocks and factors of a ``checkpoint_entry`` into the enabled LoraState (same configuration), then merge: the arena
    holds the checkpoint's merged weights again, rebuilt by the same kernel that wrote them"""
    st = model.lora
    if entry["config"] != st.config():
        raise ValueError("nbest_amd lora: the checkpoint's configuration %r differs from the enabled one %r" % (entry["config"], st.config()))
    for b in st.blocks:
        st.base_view(b).copy_(entry["base"][b.name])
    for n, _, _ in st.slots:
        st.view(st.p, n).copy_(entry["factors"][n])
    merge(model)


def adapter_from_checkpoint(ck):
    """a ``lora_state_dict`` (the content of lora.pt) from a loaded last.pt of a --lora_rank run"""
    entry = ck["lora"]
    h = hashlib.sha1()
    for t in entry["base"].values():                     # table order: the dict was written in it
        h.update(t.detach().cpu().contiguous().numpy().astype("<f4", copy=False).tobytes())
    sd = dict(format=FORMAT, base_digest=h.hexdigest(), **entry["config"])
    sd.update({n: t.clone() for n, t in entry["factors"].items()})
    sd.update({n: t.clone() for n, t in ck["model"].items() if n.startswith("clf.")})
    return sd


def merge(model):
    """rewrite the adapted blocks of arena.p / arena.w16 from base + s B A and refresh the derived weight images"""
    st = model.lora
    if st is None:
        raise RuntimeError("nbest_amd: lora_merge on a model without LoRA")
    st.merge(model.arena)
    model.arena.refresh_transposed()
