"""TOD_ASR_Transformer_STC-compatible model whose encoder, heads and losses run as hand-written HIP.

Mirrors the reference interface of /root/reference/models/model.py:
  * ``make_model(opt)``                                                        (:7-9)
  * ``model(opt, input_ids, trans_input_ids, seg_ids=, trans_seg_ids=, classifier_input_type=)``
    -> ``(top_scores, bottom_scores_dict, final_scores, asr_cls, trans_cls)``  (:35-73); ``return_attns=True`` (eval / no_grad)
    -> ``(top_scores, bottom_scores_dict, final_scores, attns, asr_cls, trans_cls)``  (:68-69)
  * ``save_model / load_model`` with the reference's state-dict keys            (:75-83)
  * parameters named ``bert_encoder.*`` / ``clf.*`` with HF sub-names, so the learning-rate and
    weight-decay grouping of /root/reference/n_best_asr_bert.py:540-550 applies unchanged.

Training does not go through torch autograd: ``forward_backward`` enqueues the whole step
(2 encoder passes when --add_l2_loss, heads + losses, backward) through the C-ABI and leaves the
gradients in the flat arena ``arena.g`` (also visible as ``param.grad`` views).
"""
import collections
import ctypes as C
import math
import os

import torch
import torch.nn as nn

from . import hipabi as hb
from . import lora as _lora
from . import prune
from .arena import ParamArena
from .config import EncoderConfig, LabelSpace, NAMED


def position_ids_for(cfg, input_ids):
    """BERT: arange(S).  RoBERTa family: cumsum(ids != pad) * (ids != pad) + pad (pad-offset positions)."""
    B, S = input_ids.shape
    if cfg.family in ("roberta", "xlm-roberta"):
        nonpad = input_ids.ne(cfg.pad_token_id).long()
        return (torch.cumsum(nonpad, dim=1) * nonpad + cfg.pad_token_id).contiguous()
    return torch.arange(S, dtype=torch.long, device=input_ids.device).unsqueeze(0).expand(B, S).contiguous()


class _Holder(nn.Module):
    """module tree node that only carries arena-backed parameters under HF names"""


def _attach(root, dotted, param):
    mod = root
    parts = dotted.split(".")
    for p in parts[:-1]:
        if not hasattr(mod, p):
            mod.add_module(p, _Holder())
        mod = getattr(mod, p)
    mod.register_parameter(parts[-1], param)


class FreezePlan(collections.namedtuple("FreezePlan", "key trainable first_trainable no_input_grad with_embeddings skip")):
    """what a training pass derives from the parameters' ``requires_grad`` flags: ``trainable`` names (never the pooler),
    ``first_trainable`` (nothing of the embeddings or of the layers below it is trainable: those run without a stash),
    ``no_input_grad`` (the embeddings are frozen: the backward forms no gradient below its lowest layer), ``with_embeddings``
    (the embedding backward runs) and ``skip`` (ctypes uint8 [4 L]: frozen QKV / attention-out / FFN-up / FFN-down matrices,
    whose weight-gradient GEMMs the backward leaves out; None = none)"""
    __slots__ = ()

    @property
    def skip_ptr(self):
        return None if self.skip is None else C.cast(self.skip, C.c_void_p)


def freeze_plan(model):
    """the FreezePlan of the model's current ``requires_grad`` flags (cached per flag pattern)"""
    flags = tuple(p.requires_grad and "pooler" not in n for n, p in model._params)
    lora = getattr(model, "lora", None)
    ckey = flags if lora is None else (flags, id(lora))
    plan = model._plans.get(ckey)
    if plan is not None:
        return plan
    trainable = frozenset(n for (n, _), f in zip(model._params, flags) if f)
    # LoRA: a matrix with an adapted block needs its dense gradient (nbest_lora_grad projects it onto the factors), so for the
    # backward it counts as trainable; it is not in ``trainable``, which the optimizer and the .grad views read
    live = trainable if lora is None else trainable | lora.adapted
    L = model.cfg.num_hidden_layers
    emb = any(n.startswith("bert_encoder.embeddings.") for n in live)
    layer = [any(n.startswith("bert_encoder.encoder.layer.%d." % l) for n in live) for l in range(L)]
    first = 0 if emb else next((l for l in range(L) if layer[l]), L)
    pre = "bert_encoder.encoder.layer.%d."
    mats = (["attention.self.%s.weight" % q for q in ("query", "key", "value")], ["attention.output.dense.weight"],
            ["intermediate.dense.weight"], ["output.dense.weight"])
    skip = [int(not any((pre % l) + m in live for m in ms)) for l in range(L) for ms in mats]
    plan = FreezePlan(flags, trainable, first, int(not emb), emb, (C.c_uint8 * len(skip))(*skip) if any(skip) else None)
    if len(model._plans) >= 64:
        model._plans.clear()
    model._plans[ckey] = plan
    return plan


class _Pass:
    """descriptor of one encoder pass shape (B, S); the activation stash it writes belongs to the slot.  Slots 0 / 1 are the
    training path's ASR / transcript passes; a named slot ("infer") is a forward-only inference descriptor without fp8 fields.
    ``first_trainable``: layers below it run without a stash (FreezePlan).  ``gate_stash``: the stash also keeps every layer's
    gated context (nbest_encoder_desc.head_gate_stash: a trainable head mask) - it is sized with the flag set."""

    def __init__(self, model, B, S, slot, first_trainable=0, gate_stash=False):
        a, cfg = model.arena, model.cfg
        train = isinstance(slot, int)
        d = hb.EncoderDesc()
        d.dtype = hb.dtype_code(model.compute_dtype)
        d.B, d.S, d.H, d.L, d.heads, d.F = B, S, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size
        d.vocab, d.max_pos, d.n_types = cfg.vocab_size, cfg.max_position_embeddings, cfg.type_vocab_size
        d.ln_eps = cfg.layer_norm_eps
        d.word_pad_id = cfg.pad_token_id
        d.pos_pad_id = cfg.pad_token_id if cfg.family in ("roberta", "xlm-roberta") else -1
        pre = "bert_encoder.embeddings."
        d.off_word = a.by_name[pre + "word_embeddings.weight"].offset
        d.off_pos = a.by_name[pre + "position_embeddings.weight"].offset
        d.off_type = a.by_name[pre + "token_type_embeddings.weight"].offset
        d.off_emb_ln_g = a.by_name[pre + "LayerNorm.weight"].offset
        d.off_emb_ln_b = a.by_name[pre + "LayerNorm.bias"].offset
        d.layers_host = C.cast(a.layer_offsets, C.POINTER(hb.LayerOffsets))
        d.drop_stream_base = 1000 * slot if train else 0
        d.first_trainable = first_trainable
        d.wgrad_group = model.wgrad_group
        if model.fp8_forward and train:    # set before the stash is sized: the fp8 mode keeps e4m3 copies of the GEMM inputs per layer
            d.w8, d.w8_inv_scale = a.w8.data_ptr(), a.w8_inv_scale.data_ptr()
        self.desc = d
        self.gate_stash = bool(gate_stash)
        if gate_stash:                     # the layout follows the flag only with a gate set (the pointer is set anew by every call)
            d.head_gate_stash, d.head_gate = 1, model.head_mask.data_ptr()
        self.act_bytes = hb.lib().nbest_encoder_act_bytes(C.byref(d))
        self.B, self.S = B, S


class _PassRecord(collections.namedtuple("_PassRecord", "ps slot inputs perm hidden gen plan cls_top gate_stash")):
    """one call's encoder pass: its _Pass, slot, (ids, seg, pos, mask), token permutation (None: sorted on the device when the
    backward asks), hidden states [B*S, H] (a view into the slot's stash), the generation of that stash it wrote, the
    FreezePlan it ran with (None: everything trainable, full stash) and whether its top layer ran on the CLS rows only (then
    only rows b S of ``hidden`` are written, and the backward must run with the same descriptor flag), and whether the stash keeps
    the gated contexts (head_gate_stash: the same holds)"""
    __slots__ = ()

    @property
    def cls(self):
        return self.hidden.view(self.ps.B, self.ps.S, -1)[:, 0, :]


class _STCBridge(torch.autograd.Function):
    """The reference's training seam VERBATIM (/root/reference/n_best_asr_bert.py:255-274): ``model(opt, ...)`` returns graph-attached
    scores, the loop builds ANY loss from them (cal_total_loss there), calls ``total_loss.backward()`` and ``optimizer.step()``.
    Forward = the HIP forward (both encoder passes + heads); backward = nbest_stc_heads_vjp for the upstream gradients autograd
    hands over, then nbest_encoder_backward for the pass(es) that received a gradient.  Parameter gradients are ADDED into the
    flat arena (``param.grad`` are views of it; call ``model.zero_grad()`` first, as the reference loop does).  The fused
    ``forward_backward`` (losses + gradients analytically in the heads kernel) is what ``train_step`` uses; this bridge costs one
    extra small launch and materialised score tensors, and exists so that a reference maintainer need not touch the loop."""

    @staticmethod
    def forward(ctx, anchor, model, input_ids, trans_input_ids, seg_ids, trans_seg_ids, feats_from_transcript):
        ctx.set_materialize_grads(False)
        from_t = bool(feats_from_transcript and trans_input_ids is not None)
        ws = hb.heads_ws(input_ids.shape[0], model.dls.n_rows, model.cfg.hidden_size, model.device)
        plan = model._training_plan()
        ra, rt, (top, bott, fin, _, _, _, _) = model._passes_and_heads(input_ids, seg_ids, trans_input_ids, trans_seg_ids, True,
                                                                       from_transcript=from_t, ws=ws, plan=plan)
        ctx.model, ctx.ra, ctx.rt, ctx.ws, ctx.seed, ctx.from_t = model, ra, rt, ws, model._step_seed(), from_t
        ctx.save_for_backward(top, bott)
        trans_cls = rt.cls.float() if rt is not None else torch.zeros(0, device=model.device)
        return top, bott, fin, ra.cls.float(), trans_cls

    @staticmethod
    def backward(ctx, dtop, dbott, dfin, dasr, dtrans):
        m = ctx.model
        m._check_stash(ctx.ra, ctx.rt)
        _require_trainable(ctx.ra.plan)
        top, bott = ctx.saved_tensors
        B, H = top.shape[0], m.cfg.hidden_size
        z = lambda g, like: torch.zeros_like(like) if g is None else g.contiguous().float()
        fin_like = torch.empty(B, m.labels.n_bottom, dtype=torch.float32, device=m.device)
        dWh, dbh = m.arena.heads_grad_wb()
        dcls = hb.stc_heads_vjp(m.arena.heads_wb()[0], m.dls, top, bott, z(dtop, top), z(dbott, bott), z(dfin, fin_like), B, H, dWh, dbh, ctx.ws,
                                accumulate=True, drop_p=m.dropout, seed=ctx.seed, drop_stream=900)
        d_asr = dasr.contiguous().float() if dasr is not None else None
        d_tr = dtrans.contiguous().float() if (dtrans is not None and ctx.rt is not None) else None
        if ctx.from_t:
            d_tr = dcls if d_tr is None else d_tr + dcls
        else:
            d_asr = dcls if d_asr is None else d_asr + dcls
        if d_tr is not None and ctx.rt is not None:
            m._backward_pass(ctx.rt, d_tr, accumulate=True)
        if d_asr is not None:
            m._backward_pass(ctx.ra, d_asr, accumulate=True)
        m._end_of_step(True)
        return (None,) * 7


def _check_distill(distill, B, dls):
    """forward_backward's ``distill`` argument -> dict(top, bott, final, alpha) or dict(logits, alpha, temperature) with a float alpha
    in [0, 1] (and a finite float temperature > 0); exactly these two key sets pass, everything else is refused before anything is
    enqueued"""
    if not isinstance(distill, dict) or set(distill) not in ({"top", "bott", "final", "alpha"}, {"logits", "alpha", "temperature"}):
        raise ValueError("nbest_amd: distill must be dict(top=, bott=, final=, alpha=) (a teacher's predict() scores and the weight "
                         "of the soft loss) or dict(logits=, alpha=, temperature=) (its predict(return_logits=True) logits)")
    alpha = float(distill["alpha"])
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("nbest_amd: distill alpha %r: must be in [0, 1]" % (distill["alpha"],))
    if "logits" in distill:
        try:
            T = float(distill["temperature"])
        except (TypeError, ValueError):
            T = float("nan")
        if not (T > 0.0 and math.isfinite(T)):
            raise ValueError("nbest_amd: distill temperature %r: must be a finite number > 0" % (distill["temperature"],))
        t = distill["logits"]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != (B, dls.n_rows):
            raise ValueError("nbest_amd: distill['logits'] must be an fp32 device tensor of shape [%d, %d] (the teacher's "
                             "predict(return_logits=True)['logits'])" % (B, dls.n_rows))
        return dict(logits=t.contiguous(), alpha=alpha, temperature=T)
    widths = dict(top=dls.labels.n_top, bott=dls.n_rows - dls.labels.n_top, final=dls.labels.n_bottom)
    for k in ("top", "bott", "final"):
        t = distill[k]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != (B, widths[k]):
            raise ValueError("nbest_amd: distill[%r] must be an fp32 device tensor of shape [%d, %d] (the teacher's predict()[%r])"
                             % (k, B, widths[k], k))
    return dict(top=distill["top"].contiguous(), bott=distill["bott"].contiguous(), final=distill["final"].contiguous(), alpha=alpha)


def _check_rdrop(rdrop, B, distill=None):
    """forward_backward's ``rdrop`` argument -> dict(alpha) with a finite float alpha >= 0; the batch of ``B`` rows must be even (rows b
    and b + B / 2 are twins) and carry no ``distill``; refused before anything is enqueued"""
    if not isinstance(rdrop, dict) or set(rdrop) != {"alpha"}:
        raise ValueError("nbest_amd: rdrop must be dict(alpha=) (the weight of the twins' consistency term)")
    if distill is not None:
        raise ValueError("nbest_amd: rdrop together with distill is not built (one soft term per step: loss_parts[3] carries it)")
    try:
        alpha = float(rdrop["alpha"])
    except (TypeError, ValueError):
        alpha = float("nan")
    if not (alpha >= 0.0 and math.isfinite(alpha)):
        raise ValueError("nbest_amd: rdrop alpha %r: must be a finite number >= 0" % (rdrop["alpha"],))
    if B < 2 or B % 2:
        raise ValueError("nbest_amd: rdrop needs a batch of 2 P rows (rows b and b + P are twins), got %d rows" % B)
    return dict(alpha=alpha)


def _check_adv(adv, need_grad=True, distill=None, rdrop=None):
    """forward_backward's ``adv`` argument -> dict(epsilon) with a finite float epsilon >= 0; it needs the backward (``need_grad``) and
    carries no ``distill`` and no ``rdrop``; refused before anything is enqueued"""
    if not isinstance(adv, dict) or set(adv) != {"epsilon"}:
        raise ValueError("nbest_amd: adv must be dict(epsilon=) (the L2 norm of the perturbation of each utterance's word embeddings)")
    if not need_grad:
        raise ValueError("nbest_amd: adv with need_grad=False: the perturbation is formed from the backward's input gradient")
    if distill is not None:
        raise ValueError("nbest_amd: adv together with distill is not built (the adversarial pass has the hard terms only)")
    if rdrop is not None:
        raise ValueError("nbest_amd: adv together with rdrop is not built (the adversarial pass has the hard terms only)")
    try:
        eps = float(adv["epsilon"])
    except (TypeError, ValueError):
        eps = float("nan")
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError("nbest_amd: adv epsilon %r: must be a finite number >= 0" % (adv["epsilon"],))
    return dict(epsilon=eps)


def _check_contrast(contrast, B, trans_input_ids=None, adv=None, device=None):
    """forward_backward's ``contrast`` argument -> dict(weight, temperature, keys): a finite float weight >= 0, a finite float
    temperature > 0 and keys None or an int64 [B] tensor; it needs the transcript tensors and carries no ``adv``; refused before
    anything is enqueued"""
    if not isinstance(contrast, dict) or not {"weight", "temperature"} <= set(contrast) or not set(contrast) <= {"weight", "temperature", "keys"}:
        raise ValueError("nbest_amd: contrast must be dict(weight=, temperature=, keys=None) (the in-batch ASR / transcript CLS "
                         "contrastive term)")
    if adv is not None:
        raise ValueError("nbest_amd: contrast together with adv is not built (the adversarial pass has the hard terms only)")
    if trans_input_ids is None:
        raise ValueError("nbest_amd: contrast needs trans_input_ids (the positives are the transcripts' CLS rows)")
    vals = {}
    for name in ("weight", "temperature"):
        try:
            vals[name] = float(contrast[name])
        except (TypeError, ValueError):
            vals[name] = float("nan")
    if not (vals["weight"] >= 0.0 and math.isfinite(vals["weight"])):
        raise ValueError("nbest_amd: contrast weight %r: must be a finite number >= 0" % (contrast["weight"],))
    if not (vals["temperature"] > 0.0 and math.isfinite(vals["temperature"])):
        raise ValueError("nbest_amd: contrast temperature %r: must be a finite number > 0" % (contrast["temperature"],))
    if B > 4096:
        raise ValueError("nbest_amd: contrast on a batch of %d rows: at most 4096 (the B x B similarity matrix)" % B)
    keys = contrast.get("keys")
    if keys is not None:
        if not torch.is_tensor(keys) or keys.dtype != torch.int64 or tuple(keys.shape) != (B,):
            raise ValueError("nbest_amd: contrast keys must be an int64 [%d] tensor (trainer.transcript_keys)" % B)
        if device is not None and keys.device.type != torch.device(device).type:       # ("cuda" names the current device)
            raise ValueError("nbest_amd: contrast keys are on %s, the model on %s" % (keys.device, device))
        keys = keys.contiguous()
    return dict(weight=vals["weight"], temperature=vals["temperature"], keys=keys)


class _CompactHeads:
    """What ``predict`` under ``set_head_mask(mask, compact=True)`` runs on: the kept head indices (host; one copy of the mask off
    the device), the table of nbest_head_prune_plan on the host and the device, the image buffers, and - bf16 - the descriptors
    nbest_pack_weights packs the Wqkv' and Wo' of layers 0 .. L-2 by (the last layer is read unpacked).  The images themselves are
    rebuilt by every ``build``: there is no weights version to key a cache on."""

    def __init__(self, model, mask):
        cfg, dev = model.cfg, model.device
        H, heads = cfg.hidden_size, cfg.num_attention_heads
        bf16 = model.compute_dtype == torch.bfloat16
        self.kept = prune.kept_heads(mask, even=bf16)
        self.tab, (qb, ob, bb) = hb.head_prune_plan(self.kept, heads, model.compute_dtype, model.arena.layer_offsets)
        self.tab_dev = torch.frombuffer(bytearray(bytes(self.tab)), dtype=torch.uint8).to(dev)
        esz = 2 if bf16 else 4
        self.w = torch.empty((qb + ob) // esz, dtype=model.compute_dtype, device=dev)
        self.b = torch.empty(bb // 4, dtype=torch.float32, device=dev)
        self.wp = self.pdescs = None
        if bf16 and len(self.kept) > 1:
            mats = []
            for t in list(self.tab)[:-1]:
                mats += [(t.dst_wqkv, 3 * 64 * t.k, H), (t.dst_wo, H, 64 * t.k)]
            arr = (hb.MatrixDesc * len(mats))()
            n_st = 0
            for i, (off, n, k) in enumerate(mats):
                bn = hb.lib().nbest_pack_bn(n)
                if not (bn > 0 and k % 32 == 0 and n % bn == 0):      # all or nothing, as the arena's own packed copies
                    arr = None
                    break
                arr[i].offset, arr[i].rows, arr[i].cols, arr[i].tile_start, arr[i].pad = off, n, k, n_st, bn
                n_st += (n // bn) * (k // 32)
            if arr is not None:
                self.pdescs = (torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev), len(mats), n_st)
                self.wp = torch.empty_like(self.w)

    def build(self, model, packed):
        """gather the images from the model's current weights (and pack them: ``packed``, bf16); returns the packed image or None"""
        a = model.arena
        hb.head_prune_pack(a.weights, a.p, model.head_mask, self.tab, model.cfg.num_attention_heads, self.w, self.b, self.tab_dev)
        if not (packed and self.pdescs is not None):
            return None
        pd, pn, pt = self.pdescs
        hb.check(hb.lib().nbest_pack_weights(hb.ptr(self.w), hb.ptr(self.wp), hb.ptr(pd), pn, pt, hb.stream_ptr()), "pack_weights")
        return self.wp


def _require_trainable(plan):
    if plan is not None and not plan.trainable:
        raise RuntimeError("nbest_amd: no parameter requires grad: a backward has nothing to compute (every tensor of the model "
                           "has requires_grad=False)")


class NBestSTCModel(nn.Module):
    def __init__(self, cfg: EncoderConfig, labels: LabelSpace, device="cuda", compute_dtype=torch.bfloat16, dropout=0.0,
                 seed=999, fp8_forward=False, fp8_backward=None, wgrad_group=hb.WGRAD_GROUP_PLAN):
        super().__init__()
        self.cfg, self.labels, self.compute_dtype = cfg, labels, compute_dtype
        self.dropout = float(dropout)                  # --dropout: feature dropout of the STC heads
        self.device = torch.device(device)
        # weight gradients without K-splits (nbest_encoder_desc.wgrad_group, hipabi.WGRAD_GROUP_*): the library's plan decides, never (every
        # layer's split-K launches), two layers per launch wherever the shapes allow, or rolling windows of 256 tiles across the layers
        self.wgrad_group = int(wgrad_group)
        # training passes run the top layer on the CLS rows only (nbest_encoder_desc.cls_top): nothing downstream reads another row
        # of the final hidden state.  False: the full-width top layer (what the passes _cls_top_ok excludes run anyway)
        self.cls_top = True
        self.arena =ParamArena(cfg, labels, self.device, compute_dtype)
        # "fp8w" (BASELINE configs[4]): forward GEMMs on the block-scaled fp8 MFMA from an e4m3 copy of the weights; the
        # master weights, the backward and everything between the GEMMs stay as in the bf16 path
        self.fp8_forward = bool(fp8_forward)
        # ... and the four dgrad and four weight-gradient GEMMs of every layer from e4m3 copies of their gradient operands, scaled
        # per tensor from the amax the same tensor had in the previous backward pass (delayed scaling), times the e4m3 weight copy
        # (dgrad) / the e4m3 activation copies the forward stashed per layer (wgrad, fp32 out); the first backward pass runs the
        # bf16 GEMMs and only records the amax history.
        self.fp8_backward = self.fp8_forward if fp8_backward is None else bool(fp8_backward)
        self._gamax_valid = False
        # ... and the forward's four GEMM inputs per layer (x, ctx, x1, gelu(u)) are e4m3 copies with a DELAYED per-tensor scale
        # 2^floor(log2(224 / amax of the same tensor in the previous step)); the first step after (re)loading weights is a
        # calibration step: bf16 GEMMs, amax recorded (round 3 cast activations at unit scale and saturated silently beyond 448)
        self._aamax_valid = False
        # batches folded into the inference history arena.iamax (fp8_calibrate; a loaded calibration counts as 1): predict(fp8=True)
        # needs one, and new weights drop it
        self.fp8_calibrated = 0
        if self.fp8_forward:
            if compute_dtype != torch.bfloat16:
                raise RuntimeError("nbest_amd: fp8_forward rides on the bf16 path")
            self.arena.enable_fp8_forward()
        elif self.fp8_backward:
            raise RuntimeError("nbest_amd: fp8_backward needs fp8_forward (it shares the e4m3 weight copy)")
        self.bert_encoder = _Holder()
        self.clf = _Holder()
        for s in self.arena.slots:
            p = nn.Parameter(self.arena.view(self.arena.p, s.name), requires_grad="pooler" not in s.name)
            if p.requires_grad:
                p.grad = self.arena.view(self.arena.g, s.name)
            root, rest = s.name.split(".", 1)
            _attach(getattr(self, root), rest, p)
        self._params = [(s.name, self.get_parameter(s.name)) for s in self.arena.slots]
        self._plans = {}                   # requires_grad pattern -> FreezePlan
        self._plan_key = None              # the pattern of the last training pass
        self.dls = hb.DeviceLabelSpace(labels, self.device)
        self.seed = int(seed)
        self.step_counter = 0
        self._passes = {}                  # (B, S, slot) -> _Pass: descriptors only (a few hundred bytes each)
        self._stash = {}                   # slot -> ONE grow-only activation stash, sized for the largest B*S seen
        self._stash_gen = collections.Counter()    # slot -> generation of its stash: moves on whenever a pass is handed the stash
        self._ws = None                    # grow-only workspace of the encoder passes
        self._dh = None                    # grow-only scratch of the backward's input gradient
        self._adv_delta = None             # grow-only fp32 perturbation of the word rows (forward_backward(adv=))
        self._adv_ws = None                # ... and the row sums of squares nbest_embed_adv_delta leaves between its launches
        self._infer_ws = None              # grow-only workspace of predict() (nbest_encoder_infer)
        self._anchor = None                # autograd bridge: a leaf that makes the outputs of forward() require grad
        self._head_mask = None             # set_head_mask: fp32 [L, heads] on the device (not a parameter, not in state_dict)

    # ---- plumbing ------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        self.arena.g.zero_()

    def _drop_fp8_history(self):
        """new weights: the gradient amax history of the fp8 backward belongs to the old ones - the next backward pass runs the
        bf16 GEMMs and records a fresh one (as the very first pass does)"""
        if self.fp8_backward and self._gamax_valid:
            self._gamax_valid = False
            self.arena.gamax.zero_()
            self.arena.gamax_slots.zero_()
        if self.fp8_forward and self._aamax_valid:
            self._aamax_valid = False
            self.arena.aamax.zero_()
            self.arena.aamax_slots.zero_()
        self._drop_fp8_calibration()

    def _drop_fp8_calibration(self):
        """new weights: the static scales of predict(fp8=True) belong to the old ones"""
        if self.fp8_forward and self.fp8_calibrated:
            self.fp8_calibrated = 0
            self.arena.iamax.zero_()
            self.arena.iamax_slots.zero_()

    def _refuse_load_under_lora(self, what):
        if self.lora is not None:
            raise RuntimeError("nbest_amd: %s with LoRA enabled: the base copy of the adapted blocks would go stale; load the "
                               "weights first, then enable_lora / load_lora" % what)

    def load_state_dict(self, *args, **kwargs):
        self._refuse_load_under_lora("load_state_dict")
        self._drop_fp8_calibration()
        return super().load_state_dict(*args, **kwargs)

    def load_reference_state(self, sd, strict=True):
        self._refuse_load_under_lora("load_reference_state")
        self._drop_fp8_history()
        return self.arena.load_state(sd, strict)

    def save_model(self, path):
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, path)

    def load_model(self, path):
        self._refuse_load_under_lora("load_model")
        self._drop_fp8_history()
        self.arena.load_state(torch.load(path, map_location="cpu", weights_only=True))

    def load_pretrained_encoder(self, path):
        """HF-format encoder weights from a LOCAL file or directory (model.safetensors / pytorch_model.bin) into the
        arena: what ``Model.from_pretrained(name)`` gives the reference (n_best_asr_bert.py:480-487), minus the fetch.

        Keys are matched after stripping the task prefix (``bert.`` / ``roberta.``) and renaming the TF-era
        ``LayerNorm.gamma/beta``; MLM/NSP heads and position-id buffers in the file are ignored; the STC heads keep
        their initialisation.  Returns the encoder tensors the file did not hold (the pooler may be absent).
        """
        import os
        if os.path.isdir(path):
            cands = [os.path.join(path, f) for f in ("model.safetensors", "pytorch_model.bin")]
            found = [c for c in cands if os.path.exists(c)]
            if not found:
                raise FileNotFoundError("no model.safetensors / pytorch_model.bin under %s" % path)
            path = found[0]
        self._refuse_load_under_lora("load_pretrained_encoder")
        self._drop_fp8_history()
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            raw = load_file(path, device="cpu")
        else:
            raw = torch.load(path, map_location="cpu", weights_only=True)
        sd = {}
        for k, v in raw.items():
            for pre in ("bert_encoder.", "bert.", "roberta.", "xlm_roberta."):
                if k.startswith(pre):
                    k = k[len(pre):]
                    break
            k = k.replace("LayerNorm.gamma", "LayerNorm.weight").replace("LayerNorm.beta", "LayerNorm.bias")
            if k.startswith(("embeddings.", "encoder.", "pooler.")) and not k.endswith("position_ids"):
                sd["bert_encoder." + k] = v
        want = [s.name for s in self.arena.slots if s.name.startswith("bert_encoder.")]
        missing = [n for n in want if n not in sd]
        hard = [n for n in missing if "pooler" not in n]
        if hard:
            raise RuntimeError("checkpoint lacks encoder tensors: %s" % hard[:5])
        self.arena.load_state(sd, strict=False)
        return missing

    # ---- LoRA (nbest_amd/lora.py) ------------------------------------------------------------------
    lora = None                            # the LoraState while LoRA is enabled

    def enable_lora(self, rank, alpha, targets=("query", "value"), layers=None, seed=0):
        """Parameter-efficient fine-tuning (Hu et al., 2022): freeze every tensor but the STC heads (``clf.*``) and train a rank-r
        update W = W0 + (alpha / rank) B A on the ``targets`` (from query, key, value, attn_out, ffn_up, ffn_down) of ``layers``
        (None: all).  A ~ U(-1/sqrt(in), 1/sqrt(in)) from ``seed``, B = 0: a forward gives the bits it gave before.  The arenas
        keep the MERGED weights, so every forward, ``predict`` and ``state_dict`` run unchanged; ``forward_backward`` leaves the
        dense gradient of the adapted matrices in ``arena.g`` (the layers below the lowest adapted one run without a stash or a
        backward, the base tensors' ``.grad`` is None) and ``HipBertAdam.step`` projects it onto the factors, updates them and the
        heads, and merges.  ``self.lora`` (lora.LoraState) holds the factors as ``params``.  Refused: an fp8w model, a head mask in
        force, a second call.  Adapter dropout is not built (it cannot act on merged weights)."""
        return _lora.enable(self, rank, alpha, targets, layers, seed)

    def disable_lora(self, restore_base=False):
        """leave LoRA: the ``requires_grad`` flags return to what they were; the weights stay merged, or with ``restore_base``
        the adapted blocks get the base bits back"""
        _lora.disable(self, restore_base)

    def lora_merge(self):
        """rewrite the adapted blocks from base + (alpha / rank) B A (after changing ``self.lora.params`` by hand)"""
        _lora.merge(self)

    def lora_state_dict(self):
        """what a task ships: format tag, rank, alpha, targets, layers, ``base_digest`` (SHA-1 of the fp32 little-endian bytes of
        the base blocks in table order), ``<tensor name>.lora_A`` / ``.lora_B`` and the ``clf.*`` tensors (the heads train too)"""
        return _lora.state_dict(self)

    def load_lora(self, sd):
        """apply a ``lora_state_dict`` to this model, which must hold the base weights it was trained on (ValueError names both
        digests otherwise): installs the factors and heads, merges"""
        self._drop_fp8_calibration()
        _lora.load(self, sd)

    # ---- head mask (HF's head_mask) ---------------------------------------------------------------
    _head_mask_trainable = False           # set_head_mask(trainable=True): forward_backward(need_grad=True) runs under the mask
    @property
    def head_mask(self):
        """the mask set_head_mask installed (fp32 [L, heads] on the device), or None"""
        return self._head_mask

    @property
    def head_mask_trainable(self):
        """True while the mask in force was installed with ``set_head_mask(mask, trainable=True)``"""
        return self._head_mask_trainable

    _head_mask_compact = False             # set_head_mask(compact=True): predict runs only the kept heads (nbest_encoder_infer_pruned)
    _prune = None                          # ... and what it runs them on: _CompactHeads (table, image buffers, pack descriptors)
    @property
    def head_mask_compact(self):
        """True while the mask in force was installed with ``set_head_mask(mask, compact=True)``"""
        return self._head_mask_compact

    def set_head_mask(self, mask, trainable=False, compact=False):
        """Gate the attention heads, as ``BertModel.forward(head_mask=)``: ``mask`` [L, heads] of any floats (0 prunes head h of
        layer l, 1 is the identity) multiplies each head's attention context after dropout and P.V, before the attention-output
        projection; None removes it.  Held on the device, not part of ``state_dict``.  While set it applies to the eval / no_grad
        ``forward``, ``forward_backward(need_grad=False)`` (what eval_epoch runs), ``predict``, ``attribute`` and ``head_gate_grad``;
        the attention maps (``return_attns``, ``cls_attn``) stay the un-gated probabilities.  Without ``trainable``,
        ``forward_backward(need_grad=True)`` and the autograd-bridge forward raise, and so does the stash forward of an fp8w model
        (its ``predict`` / ``attribute`` run the bf16 copy and work).  Without a mask every pass enqueues what it always did.
        ``trainable=True`` (needs a mask): ``forward_backward(need_grad=True)`` - and with it ``train_step`` - runs under the mask:
        the fine-tune of a pruned model (Michel et al., 2019).  Every stash pass, eval passes included, then keeps each layer's gated
        context next to the un-gated one (nbest_encoder_desc.head_gate_stash; one more [B S, H] tensor per stashed layer), the
        attention-output weight gradient reads it, and the gradient entering the attention backward is scaled by the gate; the
        scores of an eval pass are the bits of the same mask set without the flag.  The weights of a head with gate 0 get exactly
        zero gradients.  Frozen parameters (FreezePlan: frozen layers gate in place), ``accumulate``, ``chunks``, ``add_l2_loss``
        (the transcript pass runs under the same mask), ``distill=`` and ``rdrop=`` (they change the heads call and the batch only)
        and the top layer on the CLS rows (``cls_top``) work as without a mask.  Still refused: the autograd-bridge forward, an
        fp8w model, ``adv=``, and data parallelism (``train_step``).  ``head_gate_grad``, ``attribute`` and ``predict`` run their own
        descriptors as before.
        ``compact=True`` (needs a mask, refuses ``trainable=True``): ``predict`` runs only the heads the mask keeps (gate != 0) -
        per layer a [3 64k, H] QKV matrix, a k-head attention and an [H, 64k] output matrix with the gate folded into its columns
        (nbest_head_prune_pack, nbest_encoder_infer_pruned); no gate launch.  The kept indices are computed on the host here, at set
        time: ONE device-to-host copy of the [L, heads] mask; nothing else synchronises.  The compact images are rebuilt from the
        current weights at every ``predict`` call (one gather, plus one pack of the bf16 images).  In bf16 a layer with an odd
        number of kept heads also runs its lowest-numbered pruned head, whose output columns are zeros (the bf16 GEMM tiles need
        64 k to be a multiple of 128).  ``predict(return_attns=True)`` raises ValueError while it is set (the CLS maps are indexed by
        original head).  Everything else that honours a mask - the eval ``forward``, ``forward_backward(need_grad=False)``,
        ``attribute``, ``head_gate_grad`` - keeps running the gated full-width path under the same mask."""
        if mask is None:
            if trainable:
                raise ValueError("nbest_amd set_head_mask: trainable=True needs a mask (got None)")
            if compact:
                raise ValueError("nbest_amd set_head_mask: compact=True needs a mask (got None)")
            self._head_mask, self._head_mask_trainable = None, False
            self._head_mask_compact, self._prune = False, None
            return
        if compact and trainable:
            raise ValueError("nbest_amd set_head_mask: compact=True with trainable=True: training with compacted heads is not built")
        L, heads = self.cfg.num_hidden_layers, self.cfg.num_attention_heads
        m = torch.as_tensor(mask)
        if tuple(m.shape) != (L, heads):
            raise ValueError("nbest_amd set_head_mask: the mask must be [L=%d, heads=%d] (got %s)" % (L, heads, list(m.shape)))
        if compact and heads > hb.HEAD_PRUNE_MAX_HEADS:
            raise ValueError("nbest_amd set_head_mask: compact=True supports at most %d heads (got %d)" % (hb.HEAD_PRUNE_MAX_HEADS, heads))
        m = m.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
        ch = _CompactHeads(self, m) if compact else None             # (raises before anything of the model changes)
        self._head_mask = m
        self._head_mask_trainable = bool(trainable)
        self._head_mask_compact, self._prune = bool(compact), ch

    def _refuse_training_under_mask(self, what, bridge=False):
        if self._head_mask is None:
            return
        if not self._head_mask_trainable:
            raise RuntimeError("nbest_amd: %s with a head mask set: training under a head mask is not built (the attention-output "
                               "weight gradient needs the gated context); call set_head_mask(None) first, or set the mask with "
                               "trainable=True and train through forward_backward" % what)
        if bridge:
            raise RuntimeError("nbest_amd: %s with a trainable head mask set: training under a head mask runs through "
                               "forward_backward / train_step only" % what)
        if self.fp8_forward:
            raise RuntimeError("nbest_amd: %s with a trainable head mask on an fp8w model is not built (the fp8 forward has no "
                               "gated context)" % what)

    def _set_head_gate(self, d, grad=None):
        """the head-gate fields of descriptor ``d`` for this call: the mask in force (None: no gate, today's launches)"""
        d.head_gate = None if self._head_mask is None else self._head_mask.data_ptr()
        d.head_gate_grad = None if grad is None else grad.data_ptr()

    def _desc(self, B, S, slot, first_trainable=0):
        """the (cached) descriptor of a pass shape; allocates nothing.  A training-path pass (integer slot) under a trainable head
        mask is a descriptor of its own: its stash is larger (head_gate_stash)"""
        gate_stash = self._head_mask_trainable and isinstance(slot, int)
        key = (B, S, slot, first_trainable, gate_stash)
        if key not in self._passes:
            if len(self._passes) >= 4096:
                self._passes.clear()
            self._passes[key] = _Pass(self, B, S, slot, first_trainable, gate_stash)
        return self._passes[key]

    def _training_plan(self):
        """the FreezePlan of a training pass from the parameters' current ``requires_grad`` flags: frozen tensors get
        ``.grad = None``, tensors trainable again their arena view back; a new frozen set drops the fp8 gradient amax history
        (layers that had no backward have none: the next backward is a bf16 calibration pass)"""
        plan = freeze_plan(self)
        if plan.key != self._plan_key:
            for (n, p), f in zip(self._params, plan.key):
                if "pooler" in n:
                    continue
                if not f:
                    p.grad = None
                elif p.grad is None:
                    p.grad = self.arena.view(self.arena.g, n)
            if self._plan_key is not None and self.fp8_backward and self._gamax_valid:
                self._gamax_valid = False
                self.arena.gamax.zero_()
                self.arena.gamax_slots.zero_()
            self._plan_key = plan.key
        return plan

    def _grow(self, table, key, n, dtype=torch.uint8):
        """``table[key]``: a device buffer of at least n elements that only grows (``table``: ``self._stash`` keyed by slot, or
        ``vars(self)`` for the workspace attributes).  Real data pads every batch to its own longest row, so sizes change almost every
        step: one buffer sized for the largest seen is reused instead of a fresh tensor of a new size per step.  The old buffer is
        released before the new one is allocated: two generations are never held at once."""
        buf = table.get(key)
        if buf is None or buf.numel() < n:
            table[key] = buf = None
            table[key] = buf = torch.empty(n, dtype=dtype, device=self.device)
        return buf

    def _pass(self, B, S, slot, first_trainable=0):
        """the descriptor of a training pass shape, with the slot's activation stash (ASR pass / transcript pass) and the
        workspace grown to fit it.  Handing the stash to a pass moves its generation on: records of earlier passes are stale."""
        ps = self._desc(B, S, slot, first_trainable)
        self._grow(self._stash, slot, ps.act_bytes)
        self._grow(vars(self), "_ws", hb.lib().nbest_encoder_ws_bytes(C.byref(ps.desc)))
        self._stash_gen[slot] += 1
        return ps

    def _check_stash(self, *records):
        """a backward reads the activations its forward left in the slot's stash: refuse, before anything is enqueued, if another
        pass has written the stash since"""
        for r in records:
            if r is not None and r.gen != self._stash_gen[r.slot]:
                raise RuntimeError("nbest_amd: another forward ran on this model between this forward() and its backward(): the "
                                   "activations of its %s pass are overwritten" % ("ASR", "transcript")[r.slot])

    def _step_seed(self):
        """dropout counter base of this step: the element index a kernel hashes is the position inside THIS rank's
        shard, so data-parallel ranks must not share a seed (every rank would drop the same positions of its shard)"""
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        return self.seed + 7919 * self.step_counter + 15485863 * rank

    def _inputs(self, ids, seg):
        """(ids, seg, pos, key mask) of one pass as the encoder entry points take them"""
        cfg = self.cfg
        ids = ids.contiguous()
        mask = (ids > 0).to(torch.uint8)               # quirk Q1: ids > 0 for EVERY family (models/model.py:43)
        pos = position_ids_for(cfg, ids)
        if cfg.family == "xlm-roberta":
            seg = None                                  # models/model.py:42-43: XLM-R never gets token types
        elif seg is not None:
            seg = seg.contiguous()
        return ids, seg, pos, mask

    def _encode(self, slot, ids, seg, train, perm=None, plan=None, full_top=False):
        """one encoder pass through the C-ABI into the slot's stash; returns its _PassRecord.
        ``perm``: the pass's tokens sorted by word id (hipabi.word_perm; host-built by the data loaders) - only the backward
        reads it; None = sorted on the device when a backward pass asks for it.  ``plan``: the FreezePlan of a pass a backward
        may follow (None: full stash)."""
        B, S = ids.shape
        ps = self._pass(B, S, slot, plan.first_trainable if plan is not None else 0)
        ids, seg, pos, mask = inputs = self._inputs(ids, seg)
        d = ps.desc
        d.hidden_drop = self.cfg.hidden_dropout_prob if train else 0.0
        d.attn_drop = self.cfg.attention_probs_dropout_prob if train else 0.0
        d.seed = self._step_seed()
        self._set_head_gate(d)
        # a trainable mask: every stash forward keeps the gated contexts.  (_desc keys the cached descriptors on the flag and _Pass
        # sets it, so this, the record's field and the backward's restore repeat ps.gate_stash: stated per call like cls_top)
        d.head_gate_stash = int(ps.gate_stash)
        self._set_weights(d, "forward")
        d.cls_top = int(not full_top and self._cls_top_ok(train, S, plan))
        act, ws = self._stash[slot][:ps.act_bytes], self._ws
        out = C.c_void_p()
        hb.check(hb.lib().nbest_encoder_forward(C.byref(d), hb.ptr(self.arena.weights), hb.ptr(self.arena.p), hb.ptr(ids),
                                                hb.ptr(seg), hb.ptr(pos), hb.ptr(mask), hb.ptr(act), act.numel(),
                                                hb.ptr(ws), ws.numel(), C.byref(out), hb.stream_ptr()),
                 "encoder_forward")
        off = out.value - act.data_ptr()
        M, H = B * S, self.cfg.hidden_size
        esz = 2 if self.compute_dtype == torch.bfloat16 else 4
        hidden = act[off:off + M * H * esz].view(self.compute_dtype).view(M, H)
        return _PassRecord(ps, slot, inputs, perm, hidden, self._stash_gen[slot], plan, bool(d.cls_top), ps.gate_stash)

    def _cls_top_ok(self, train, S, plan):
        """a training pass runs its top layer on the CLS rows (``self.cls_top``) unless the library refuses the combination: the fp8
        modes, a head mask that is not trainable.  Whatever is frozen (``plan``): an all-frozen encoder gives its heads the CLS rows a trainable one gives.
        Eval passes keep the full-width layer: ``return_attns`` reads its lse from the stash."""
        return self.cls_top and train and S >= 2 and not self.fp8_forward and (self._head_mask is None or self._head_mask_trainable)

    def _packed_bf16_ok(self):
        """the packed bf16 weight copies (arena.wpk / wpkt) exist and are current: they are refreshed with the bf16 transposed
        copy, which goes stale while the backward runs in fp8"""
        return self.arena.wpk is not None and not self.arena.w16t_stale

    def _set_weights(self, d, call):
        """the weight-copy and fp8 fields of descriptor ``d`` for a "forward", "backward" or "infer" call.  The forward and the
        backward of one step see the same values; an inference descriptor has no fp8 fields (_Pass) and reads the bf16 copy."""
        a = self.arena
        fp8_bwd = self.fp8_backward and call != "infer" and self._gamax_valid and self._aamax_valid
        if call == "backward" and a.w16t_stale and not fp8_bwd:
            a.refresh_w16t()                      # a bf16 backward after fp8 steps (history dropped, mode switched)
        ok = self._packed_bf16_ok()
        d.wpk = a.wpk.data_ptr() if ok else None
        d.wpkt = a.wpkt.data_ptr() if ok else None
        if call == "infer":
            return
        ok8 = a.w8p is not None
        d.w8p = a.w8p.data_ptr() if ok8 else None
        d.w8tp = a.w8tp.data_ptr() if ok8 else None
        if self.fp8_forward and call == "forward":
            # activation amax history of the fp8 forward: the same two generations for every pass of a step (ASR + transcript pass
            # record into the same words: the next step's scale covers both); the backward reads the fields its forward set
            d.aamax_prev, d.aamax_new = a.aamax.data_ptr(), a.aamax_slots.data_ptr()
            d.fp8_act = int(self._aamax_valid)
        if self.fp8_backward:                     # the forward leaves out the bf16 tensors an fp8 backward will not read
            d.w8t = a.w8t.data_ptr()
            d.gamax_prev, d.gamax_new = a.gamax.data_ptr(), a.gamax_slots.data_ptr()
            d.fp8_bwd = int(fp8_bwd)              # the fp8 weight gradients read the fp8 forward's activation copies
            a.lazy_w16t = fp8_bwd                 # steady state: every dgrad reads w8t, nobody reads the bf16 transposed copy

    def _end_of_step(self, ran_backward, advance=True):
        """this step's recorded amax (slots) becomes the history of the next one - after the backward, which reads the forward's
        copies scaled by the old history; ``advance``: a training step moves the dropout streams on (an eval forward does not)"""
        if self.fp8_forward:
            hb.fp8_amax_fold(self.arena.aamax_slots, self.arena.aamax)
            self._aamax_valid = True
        if ran_backward and self.fp8_backward:
            hb.fp8_amax_fold(self.arena.gamax_slots, self.arena.gamax)
            self._gamax_valid = True
        if advance:
            self.step_counter += 1

    def _backward_pass(self, rec, dcls, accumulate, chunks=None, on_chunk_done=None):
        """the encoder backward of the pass ``rec`` recorded (its activations must still be in the slot's stash)"""
        ps, d = rec.ps, rec.ps.desc
        B, S, H = ps.B, ps.S, self.cfg.hidden_size
        self._set_weights(d, "backward")
        d.cls_top = int(rec.cls_top)              # as the forward that wrote this stash
        d.head_gate_stash = int(rec.gate_stash)   # likewise
        # gradient w.r.t. the final hidden states [B*S, H] (zero except the CLS rows), in a grow-only buffer like the stash
        dh = self._grow(vars(self), "_dh", B * S * H, self.compute_dtype)[:B * S * H].view(B * S, H)
        dh = hb.cls_grad_scatter(dcls, B, S, H, self.compute_dtype, out=dh)
        ids, seg, pos, mask = rec.inputs
        perm = rec.perm if rec.perm is not None else hb.word_perm(ids)
        d.word_perm = perm.data_ptr()
        act, ws = self._stash[rec.slot][:ps.act_bytes], self._ws
        plan = rec.plan
        ft = plan.first_trainable if plan is not None else 0
        d.no_input_grad = plan.no_input_grad if plan is not None else 0
        d.wgrad_skip_host = plan.skip_ptr if plan is not None else None
        with_emb = plan.with_embeddings if plan is not None else True
        bounds = chunks or [(0, self.cfg.num_hidden_layers)]
        for (lo, hi) in sorted(bounds, reverse=True):
            lo_t = max(lo, ft)                    # nothing below first_trainable is stashed or trainable
            if hi > lo_t:
                hb.check(hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(self.arena.weights), hb.ptr(self.arena.w16t),
                                                         hb.ptr(self.arena.p),
                                                         hb.ptr(self.arena.g), hb.ptr(ids), hb.ptr(seg), hb.ptr(pos), hb.ptr(mask),
                                                         hb.ptr(act), act.numel(), hb.ptr(dh), hb.ptr(ws), ws.numel(),
                                                         int(accumulate), lo_t, hi, int(lo_t == 0 and with_emb), hb.stream_ptr()),
                         "encoder_backward")
            if on_chunk_done is not None:
                on_chunk_done(lo, hi)

    def _heads(self, hidden, S, labels_f, need_grad, train, accumulate=False, ws=None, distill=None, rdrop=None):
        """``ws``: a private heads workspace (the autograd bridge keeps it for stc_heads_vjp); None = the shared scratch.
        ``distill`` / ``rdrop``: forward_backward's checked arguments - the same two launches through nbest_stc_heads_kd,
        nbest_stc_heads_kd_t or nbest_stc_heads_rdrop (one hb.SoftTerm says which)"""
        B, H = hidden.shape[0] // S, self.cfg.hidden_size
        Wh, bh = self.arena.heads_wb()
        dWh, dbh = self.arena.heads_grad_wb()
        if labels_f is None:
            labels_f = torch.zeros(B, self.labels.n_bottom, dtype=torch.float32, device=self.device)
        soft = None
        if rdrop is not None:
            soft = hb.SoftTerm("rdrop", rdrop["alpha"])
        elif distill is not None and "logits" in distill:
            soft = hb.SoftTerm("kd_t", distill["alpha"], distill["temperature"], (distill["logits"],))
        elif distill is not None:
            soft = hb.SoftTerm("kd", distill["alpha"], None, (distill["top"], distill["bott"], distill["final"]))
        return hb.stc_heads(hidden, S * H, Wh, bh, self.dls, labels_f.contiguous(), B, H, need_grad=need_grad,
                            accumulate=accumulate, drop_p=self.dropout if train else 0.0,
                            seed=self._step_seed(), drop_stream=900, dWh=dWh, dbh=dbh, ws=ws, soft=soft)

    def _passes_and_heads(self, ids, seg, trans_ids, trans_seg, train, from_transcript=False, labels_f=None, need_grad=False,
                          accumulate=False, perm=None, trans_perm=None, ws=None, plan=None, after_asr=None, distill=None, rdrop=None,
                          full_top=False):
        """the ASR pass, the transcript pass when ``trans_ids`` is given, then the heads on the CLS rows of the one
        ``from_transcript`` picks.  Returns (ASR record, transcript record or None, the stc_heads outputs).
        ``after_asr(record)``: called right after the ASR pass, before any other pass can touch a stash."""
        ra = self._encode(0, ids, seg, train, perm, plan, full_top)
        if after_asr is not None:
            after_asr(ra)
        rt = None if trans_ids is None else self._encode(1, trans_ids, trans_seg, train, trans_perm, plan, full_top)
        r = rt if from_transcript else ra
        return ra, rt, self._heads(r.hidden, r.ps.S, labels_f, need_grad, train, accumulate, ws, distill, rdrop)

    def _bottoms_dict(self, bott):
        out, col = {}, 0
        for t in self.labels.multi:
            n = len(self.labels.top2bottom[t])
            out["lin_%d" % t] = bott[:, col:col + n]
            col += n
        return out

    # ---- reference-compatible forward (models/model.py:35-73) -----------------------------------
    def forward(self, opt, input_ids, trans_input_ids=None, seg_ids=None, trans_seg_ids=None, return_attns=False,
                classifier_input_type="asr", distill=None):
        """Training mode under autograd: graph-attached outputs (``_STCBridge``), so the reference's
        ``total_loss.backward(); optimizer.step()`` loop body runs unmodified.  Otherwise (eval / no_grad): plain tensors.
        ``return_attns`` (eval / no_grad only): also ``attns``, a tuple of L fp32 tensors [B, heads, S, S] - the attention
        probabilities of every layer of the ASR pass (the reference's return_attns branch), 4th in the 6-tuple."""
        if distill is not None:
            raise RuntimeError("nbest_amd: distill= belongs to forward_backward (the fused step: train_step, the CLI); the forward "
                               "returns scores - build the soft loss from them and a teacher's predict() yourself")
        if self.training and torch.is_grad_enabled():
            if return_attns:
                raise RuntimeError("nbest_amd: return_attns=True: attention maps are an eval / predict output - call model.eval() "
                                   "or run the forward under torch.no_grad() (a training forward has no post-dropout maps)")
            self._refuse_training_under_mask("the training forward (autograd bridge)", bridge=True)
            if self._anchor is None:
                self._anchor = torch.zeros(1, device=self.device, requires_grad=True)    # what makes the outputs require grad
            top, bott, fin, asr_cls, trans_cls = _STCBridge.apply(self._anchor, self, input_ids.contiguous(),
                                                                  None if trans_input_ids is None else trans_input_ids.contiguous(), seg_ids,
                                                                  trans_seg_ids, classifier_input_type == "transcript")
            return top, self._bottoms_dict(bott), fin, asr_cls, (trans_cls if trans_input_ids is not None else None)
        with torch.no_grad():
            return self._forward_plain(input_ids, trans_input_ids, seg_ids, trans_seg_ids, classifier_input_type, return_attns)

    def _forward_plain(self, input_ids, trans_input_ids, seg_ids, trans_seg_ids, classifier_input_type, return_attns=False):
        attns = []
        after = (lambda rec: attns.extend(self._attention_maps(rec))) if return_attns else None
        ra, rt, (top, bott, fin, _, _, _, _) = self._passes_and_heads(input_ids, seg_ids, trans_input_ids, trans_seg_ids, self.training,
                                                                      from_transcript=classifier_input_type == "transcript",
                                                                      after_asr=after, full_top=return_attns)
        self._end_of_step(False, advance=False)
        trans_cls = None if rt is None else rt.cls.float()
        if return_attns:
            return top, self._bottoms_dict(bott), fin, tuple(attns), ra.cls.float(), trans_cls
        return top, self._bottoms_dict(bott), fin, ra.cls.float(), trans_cls

    def _attention_maps(self, rec):
        """fp32 [B, heads, S, S] per layer: the attention probabilities of the pass ``rec`` recorded, from the qkv and lse its
        forward left in the slot's stash (nbest_encoder_act_view + nbest_attention_probs)"""
        self._check_stash(rec)
        ps = rec.ps
        B, S, H, heads = ps.B, ps.S, self.cfg.hidden_size, self.cfg.num_attention_heads
        act = self._stash[rec.slot]
        base, esz = act.data_ptr(), (2 if self.compute_dtype == torch.bfloat16 else 4)
        n_qkv, n_lse = B * S * 3 * H * esz, B * heads * S * 4
        out = []
        for l in range(self.cfg.num_hidden_layers):
            qp, lp = hb.encoder_act_view(ps.desc, act, l)
            qkv = act[qp - base:qp - base + n_qkv].view(self.compute_dtype)
            lse = act[lp - base:lp - base + n_lse].view(torch.float32)
            out.append(hb.attention_probs(qkv, rec.inputs[3], lse, B, S, heads))
        return out

    def _stash_attention_views(self, rec):
        """per layer (qkv [B S, 3H] compute dtype, lse fp32 [B, heads, S]): views of what the pass ``rec`` left in its stash"""
        ps = rec.ps
        B, S, H, heads = ps.B, ps.S, self.cfg.hidden_size, self.cfg.num_attention_heads
        act = self._stash[rec.slot]
        base, esz = act.data_ptr(), (2 if self.compute_dtype == torch.bfloat16 else 4)
        n_qkv, n_lse = B * S * 3 * H * esz, B * heads * S * 4
        for l in range(self.cfg.num_hidden_layers):
            qp, lp = hb.encoder_act_view(ps.desc, act, l)
            yield (act[qp - base:qp - base + n_qkv].view(self.compute_dtype), act[lp - base:lp - base + n_lse].view(torch.float32))

    # ---- attention rollout of the CLS row (Abnar & Zuidema, 2020) --------------------------------
    @torch.no_grad()
    def attention_rollout(self, input_ids, seg_ids=None, residual=0.5):
        """The CLS row of A~_{L-1} ... A~_0, A~_l = residual I + (1 - residual) mean_h A_l: how much of the top [CLS] state rests on
        each input token once the mixing of the layers below is accounted for.  One eval forward of the ASR pass with the full
        stash (the pass of ``forward(return_attns=True)``, never with dropout, whatever ``model.training`` says), then L launches
        of nbest_attention_rollout_step on the stashed qkv / lse, from the top layer down, on a one-hot [CLS] row: no attention
        map is written, no host synchronisation.
        Returns dict(top, bott, final, pred, rollout fp32 [B, S], layers fp32 [L, B, S]): the scores are the bits of the eval
        forward and ``decode``; ``layers[l]`` is the CLS row of A~_{L-1} ... A~_l, so ``layers[0]`` is ``rollout`` and
        ``layers[L-1]`` the last layer's head-mean CLS attention mixed with ``residual``.
        Touches what an eval forward touches (the ASR stash; an fp8w model folds its activation amax as its ``return_attns``
        forward does) and nothing else: no gradients, optimizer moments or ``step_counter``.
        ValueError for a residual outside [0, 1] or not finite; RuntimeError while a head mask is set (not built: a head mean
        under a gate is not defined here) and for an S the position table does not hold."""
        rho = float(residual)
        if not (0.0 <= rho <= 1.0):                                     # (NaN fails both comparisons)
            raise ValueError("nbest_amd attention_rollout: residual must be a finite number in [0, 1] (got %r)" % (residual,))
        if self._head_mask is not None:
            raise RuntimeError("nbest_amd attention_rollout: rollout under a head mask (gated or compact) is not built (the mean "
                               "over heads under a gate is not defined here); call set_head_mask(None) first")
        cfg = self.cfg
        B, S = input_ids.shape
        first_pos = cfg.pad_token_id + 1 if cfg.family in ("roberta", "xlm-roberta") else 0
        if S > 512 or S + first_pos > cfg.max_position_embeddings:     # refused before anything is enqueued
            raise RuntimeError("nbest_amd attention_rollout: S=%d does not fit the position table (%d rows)"
                               % (S, cfg.max_position_embeddings))
        L, heads = cfg.num_hidden_layers, cfg.num_attention_heads
        rows = torch.zeros(L + 1, B, S, dtype=torch.float32, device=self.device)
        rows[L, :, 0] = 1.0                                             # e_CLS; rows[l] = the CLS row of A~_{L-1} ... A~_l

        def after(rec):
            self._check_stash(rec)
            views = list(self._stash_attention_views(rec))
            for l in range(L - 1, -1, -1):
                hb.attention_rollout_step(views[l][0], rec.inputs[3], views[l][1], rows[l + 1], rho, B, S, heads, out=rows[l])

        _, _, (top, bott, fin, _, _, _, _) = self._passes_and_heads(input_ids, seg_ids, None, None, False, after_asr=after, full_top=True)
        self._end_of_step(False, advance=False)
        return dict(top=top, bott=bott, final=fin, pred=self.decode(top, bott), rollout=rows[0], layers=rows[:L])

    # ---- one training forward + backward (n_best_asr_bert.py:249-264) ---------------------------
    def forward_backward(self, input_ids, labels_f, seg_ids=None, trans_input_ids=None, trans_seg_ids=None,
                         add_l2_loss=False, mse_grad_scale=1.0, chunks=None, on_chunk_done=None, need_grad=True,
                         accumulate=False, encoder_grad_scale=1.0, tok_perm=None, trans_tok_perm=None, distill=None, rdrop=None,
                         adv=None, contrast=None, advance=True):
        """Returns dict(top, bott, final, loss_parts[4] (device), asr_cls, trans_cls).  Gradients of the sum
        BCE(final) + BCE(top) + mean-CE (+ MSE) are left in ``arena.g``.  The transcript pass runs only
        when its output is used (--add_l2_loss); the reference computes and discards it otherwise (Q4).
        ``accumulate``: add to the gradients already in ``arena.g`` (gradient accumulation) instead of overwriting them.
        ``encoder_grad_scale``: multiplies the gradient entering the encoder (the CLS rows) - a loss-scaling knob; the tests use it to
        make every gradient amax of the fp8 backward jump between two consecutive steps.
        ``tok_perm`` / ``trans_tok_perm``: int32 [B*S] token indices sorted (stably) by word id, for the deterministic embedding
        backward; the data loaders build them on the host next to the ids (None: sorted on the device).
        Frozen parameters (``requires_grad`` False) get no gradient (FreezePlan); with none trainable this raises.
        ``distill`` = dict(top=, bott=, final=, alpha=): knowledge distillation.  top / bott / final are a teacher's scores for the
        same utterances - fp32 device tensors in ``predict``'s shapes - and 0 <= alpha <= 1.  The heads of the ASR pass then run
        nbest_stc_heads_kd: ``loss_parts[3]`` is the soft loss (the three terms with the teacher's scores in place of the labels,
        unscaled) and the gradients left in ``arena.g`` are those of (1 - alpha) * hard + alpha * soft (+ MSE, unweighted).  With
        ``add_l2_loss`` too, loss_parts[3] stays the soft loss and the MSE is returned as ``mse``.  Same launches as without.
        ``distill`` = dict(logits=, alpha=, temperature=): the same at a temperature T (finite, > 0).  logits is the teacher's
        ``predict(return_logits=True)["logits"]``, fp32 [B, R]; the heads run nbest_stc_heads_kd_t, which divides both models'
        logits by T: ``loss_parts[3]`` is T^2 x the soft loss of the tempered scores and enters the gradient with weight alpha.
        The returned top / bott / final and the hard terms are the T = 1 quantities.
        ``rdrop`` = dict(alpha=): R-Drop.  The batch handed in has 2 P rows and rows b / b + P are a pair (the same holds for
        ``labels_f``, ``seg_ids`` and the transcript tensors, which work as for any batch); the twins are usually two copies of an
        utterance, which the position-keyed dropout hashes run under independent masks, but need not be.  The heads of the ASR pass
        run nbest_stc_heads_rdrop: ``loss_parts[3]`` is the sum over the P pairs of the symmetric KL between the twins' outputs
        (unscaled) and the gradients left in ``arena.g`` are those of the hard loss of all 2 P rows + alpha * that (+ MSE).  alpha
        finite and >= 0; not together with ``distill``.  With ``add_l2_loss`` the MSE comes back as ``mse``.  Same launches as without.
        ``adv`` = dict(epsilon=): adversarial training on the word embeddings, the fast gradient method (Miyato et al., 2017).  The
        clean step runs first, exactly as without the argument (with the caller's ``accumulate``).  Its ASR backward leaves the
        gradient of the step's whole loss (MSE term included) w.r.t. the embedding LayerNorm output; nbest_embed_adv_delta turns it
        into the gradient g w.r.t. each token's word embedding and into delta = epsilon g / ||g||, the norm taken per utterance over
        its non-padding tokens (an utterance whose norm is zero or not finite gets delta = 0).  The ASR pass then runs again with
        delta added to the word rows (nbest_encoder_desc.emb_delta), the heads with the hard terms only, and its backward ADDS its
        parameter gradients: ``arena.g`` holds those of L(x) + L(x + delta), delta a constant.  No transcript pass and no MSE term in
        the second pass.  ``step_counter`` does not move between the two passes, so both run under the SAME dropout bits (encoder
        and heads): the perturbation is adversarial for exactly the network instance that produced the gradient.  The dict gains
        ``adv_loss_parts`` (fp32 [4], device: the perturbed pass's three hard terms, slot 3 zero) and ``adv_norm`` (fp32 [B]: ||g||
        per utterance); everything else returned is the clean pass's.  epsilon finite and >= 0 (0 runs the second pass with a zero
        delta).  Needs ``need_grad``, trainable embeddings, no head mask, no fp8 model; not together with ``distill`` or ``rdrop``.
        No host synchronisation; about twice the launches of the plain step plus three.
        ``contrast`` = dict(weight=, temperature=, keys=None): the in-batch contrastive term between the ASR and the transcript CLS
        rows (nbest_cls_contrast: each utterance's ASR row must pick its own transcript's row out of the batch's, and the other way
        round).  The transcript pass runs (as for ``add_l2_loss``, undetached); after the MSE, if any, the kernel adds weight * dL
        to the CLS gradients of both passes, so ``arena.g`` holds the gradients of hard (+ MSE) (+ soft) + weight * L.  ``keys``:
        int64 [B] (trainer.transcript_keys): rows with an equal key - identical transcripts - stay out of each other's
        denominators; None keeps every pair.  The dict gains ``contrast``, fp32 [4] on the device: L summed over the batch and
        unweighted, the number of rows whose own transcript is their nearest kept one, B, 0.  ``loss_parts`` is untouched.  The
        negatives are the rows of THIS call: under gradient accumulation those of the micro-batch.  ``need_grad=False``: the loss
        only.  weight finite and >= 0, temperature finite and > 0; needs ``trans_input_ids``; not with ``adv``, not on an fp8w model
        and not under a head mask (not built).  Four launches more than the same step without it, no host synchronisation.
        ``advance=False``: ``step_counter`` stays where it is, so the NEXT call runs under the same dropout bits (encoder and heads) -
        the first pass of a SAM step (trainer.train_step(sam_rho=)), whose second pass must see the network instance that produced
        the gradient.  Everything else is as without it."""
        if contrast is not None:
            contrast = _check_contrast(contrast, input_ids.shape[0], trans_input_ids, adv, self.device)
            if self._head_mask is not None:
                raise RuntimeError("nbest_amd: contrast with a head mask set is not built (the contrastive term under a head mask, "
                                   "trainable or not)")
            if self.fp8_forward:
                raise RuntimeError("nbest_amd: contrast on an fp8w model is not built (its CLS rows carry e4m3 noise of the size of "
                                   "the cosine differences the term resolves)")
        if adv is not None:
            adv = _check_adv(adv, need_grad, distill, rdrop)
            if self._head_mask is not None:
                raise RuntimeError("nbest_amd: adv with a head mask set is not built (FGM under a head mask, trainable or not)")
            if self.fp8_forward:
                raise RuntimeError("nbest_amd: adv on an fp8w model is not built (the fp8 forward has no perturbed embedding)")
        if rdrop is not None:
            rdrop = _check_rdrop(rdrop, input_ids.shape[0], distill)
        if distill is not None:
            distill = _check_distill(distill, input_ids.shape[0], self.dls)
        plan = None
        if need_grad:
            self._refuse_training_under_mask("forward_backward(need_grad=True)")
            plan = self._training_plan()
            _require_trainable(plan)
            if adv is not None and (plan.first_trainable > 0 or not plan.with_embeddings):
                raise RuntimeError("nbest_amd: adv needs trainable embeddings (the perturbation is formed from the gradient w.r.t. "
                                   "the word embeddings, which a backward over frozen embeddings does not form)")
        ra, rt, (top, bott, fin, loss, dcls, _, _) = self._passes_and_heads(
            input_ids, seg_ids, trans_input_ids if (add_l2_loss or contrast is not None) else None, trans_seg_ids, self.training, labels_f=labels_f,
            need_grad=need_grad, accumulate=accumulate, perm=tok_perm, trans_perm=trans_tok_perm, plan=plan, distill=distill, rdrop=rdrop)
        B, H = ra.ps.B, self.cfg.hidden_size
        dt = mse = con = None
        if rt is not None:
            dt = torch.empty(B, H, dtype=torch.float32, device=self.device) if need_grad else None
        if rt is not None and add_l2_loss:
            mse = hb.cls_mse(ra.hidden, ra.ps.S * H, rt.hidden, rt.ps.S * H, B, H, dcls, dt, grad_scale=mse_grad_scale)
            if distill is None and rdrop is None:
                loss[3:4].copy_(mse)
        if contrast is not None:
            ws = self._grow(vars(self), "_contrast_ws", hb.cls_contrast_ws_bytes(B, H))
            con = hb.cls_contrast(ra.hidden, ra.ps.S * H, rt.hidden, rt.ps.S * H, B, H, contrast["weight"], contrast["temperature"],
                                  keys=contrast["keys"], da=dcls if need_grad else None, dt=dt, accumulate_dt=mse is not None, ws=ws)
        if need_grad and encoder_grad_scale != 1.0:
            dcls.mul_(encoder_grad_scale)
            if dt is not None:
                dt.mul_(encoder_grad_scale)
        if need_grad:
            if rt is not None:
                # transcript pass first (whole stack, no overlap hooks), then the ASR pass accumulates on top
                self._backward_pass(rt, dt, accumulate=accumulate)
                self._backward_pass(ra, dcls, accumulate=True, chunks=chunks, on_chunk_done=on_chunk_done)
            else:
                self._backward_pass(ra, dcls, accumulate=accumulate, chunks=chunks, on_chunk_done=on_chunk_done)
        adv_out = None
        if adv is not None:
            adv_out = self._adversarial_pass(ra, labels_f, adv["epsilon"], plan, chunks, on_chunk_done, encoder_grad_scale)
        self._end_of_step(need_grad, advance=advance)
        out = dict(top=top, bott=bott, final=fin, loss_parts=loss, asr_cls=ra.cls, trans_cls=None if rt is None else rt.cls)
        if adv_out is not None:
            out["adv_loss_parts"], out["adv_norm"] = adv_out
        if con is not None:
            out["contrast"] = con
        if (distill is not None or rdrop is not None) and mse is not None:
            out["mse"] = mse
        return out

    def _adversarial_pass(self, ra, labels_f, epsilon, plan, chunks=None, on_chunk_done=None, encoder_grad_scale=1.0):
        """the second half of an FGM step (forward_backward(adv=)): the clean ASR pass ``ra`` has run its backward, so ``self._dh``
        holds the gradient w.r.t. its embedding LayerNorm output.  Forms delta, runs the ASR pass again on the perturbed word rows
        (slot 0: the clean stash is finished with) and adds its gradients to ``arena.g``.  Same step seed, same dropout bits.
        Returns (adv_loss_parts, adv_norm).  Nothing here waits for the device."""
        a, cfg = self.arena, self.cfg
        B, S, H = ra.ps.B, ra.ps.S, cfg.hidden_size
        ids, seg, pos, mask = ra.inputs
        d = ra.ps.desc
        pre = "bert_encoder.embeddings."
        word, ttab, ptab = (a.view(a.weights, pre + n) for n in ("word_embeddings.weight", "token_type_embeddings.weight", "position_embeddings.weight"))
        gamma = a.view(a.p, pre + "LayerNorm.weight")
        dh = self._dh[:B * S * H].view(B * S, H)
        delta = self._grow(vars(self), "_adv_delta", B * S * H, torch.float32)[:B * S * H].view(B * S, H)
        ws = self._grow(vars(self), "_adv_ws", hb.lib().nbest_embed_adv_ws_bytes(B, S))
        norm = torch.empty(B, dtype=torch.float32, device=self.device)
        hb.embed_adv_delta(ids, seg, pos, mask, word, ttab, ptab, gamma, dh, B, S, cfg.layer_norm_eps, epsilon, drop_p=d.hidden_drop,
                           seed=d.seed, drop_stream=d.drop_stream_base, out=delta, norm=norm, ws=ws)
        perm = ra.perm if ra.perm is not None else hb.word_perm(ids)
        d.emb_delta = delta.data_ptr()
        try:                                                 # whatever raises, the cached descriptor keeps no pointer of this call
            rb = self._encode(0, ids, seg, self.training, perm, plan)
            _, _, _, adv_loss, dcls, _, _ = self._heads(rb.hidden, S, labels_f, True, self.training, accumulate=True)
            if encoder_grad_scale != 1.0:
                dcls.mul_(encoder_grad_scale)
            self._backward_pass(rb, dcls, accumulate=True, chunks=chunks, on_chunk_done=on_chunk_done)
        finally:
            d.emb_delta = None
        return adv_loss, norm

    # ---- inference (forward only, CLS rows of the last layer) ------------------------------------
    def predict(self, input_ids, seg_ids=None, return_attns=False, return_logits=False, fp8=False, token_keep=None,
                return_token_kept=False):
        """Scores and decoded labels of one batch through nbest_encoder_infer: no activation stash, no dropout (in either
        mode), the heads on the compact CLS rows.  Returns dict(top, bott, final, cls [B, H] compute dtype, pred int32 [B, n_top]).
        ``return_attns``: also ``cls_attn``, fp32 [L, B, heads, S] - the CLS row's attention probabilities of every layer
        (nbest_encoder_infer_attn); the other outputs are the same bits as without it.
        ``return_logits``: also ``logits``, fp32 [B, R] - the logits of the heads in the order of the head matrix's rows (the top
        classifier, then the softmax heads in head order), from nbest_stc_heads_logits on the same CLS rows: one launch after the
        heads call, which is unchanged; without the flag nothing new is enqueued.
        Touches no training state: stashes, gradients, optimizer moments, step_counter and the fp8 amax histories stay as they
        are.  An fp8w model runs its bf16 weight copy, unpacked (as its calibration pass reads it).
        Under ``set_head_mask(mask, compact=True)``: the compact images are gathered from the current weights (and packed, where
        the packed bf16 copies are in use), then nbest_encoder_infer_pruned runs only the kept heads; ``return_attns`` raises
        ValueError.
        ``fp8=True`` (a model built with ``fp8_forward=True``, after ``fp8_calibrate``): nbest_encoder_infer_fp8 - the full-width GEMMs
        of layers 0 .. L-2 and the last layer's K|V projection on the block-scaled fp8 MFMA, with the STATIC activation scales of the
        calibration (2^floor(log2(224 / amax)): a value up to twice the calibrated amax is representable, beyond that the e4m3 cast
        saturates silently); the B CLS rows of the last layer and the heads stay bf16.  RuntimeError on a model without the fp8
        forward, before a calibration and under a head mask (compact or not); ValueError with ``return_attns``.  Without the
        argument nothing changes: the bf16 path, bit for bit.
        ``token_keep`` (L - 1 positive, non-increasing ints): nbest_encoder_infer_tokens - after layer l every utterance keeps
        [CLS] plus the ``token_keep[l] - 1`` other tokens that received the most attention in that layer (head mean of the column
        sums over the unmasked queries; unmasked before padding, ties to the lower index), and the layers above run on the shorter
        sequence.  S_0 = S, S_{l+1} = min(token_keep[l], S_l); a layer that drops nothing launches nothing, so a schedule of entries
        >= S gives the bits of the call without it.  ``return_token_kept``: also ``token_kept``, int32 [L - 1, B, S] (the original
        positions that leave layer l, ascending, then -1) and ``token_counts``, the host list [S_0, ..., S_{L-1}].  ValueError for a
        wrong length, an entry < 1, an increasing schedule, ``return_attns`` with it, or ``return_token_kept`` without it;
        RuntimeError with ``fp8=True`` and under any head mask (not built).  ``None``: today's path, bit for bit."""
        cfg = self.cfg
        if token_keep is not None:
            keep = [int(x) for x in token_keep]
            if len(keep) != cfg.num_hidden_layers - 1:
                raise ValueError("nbest_amd predict: token_keep needs L - 1 = %d entries (got %d)" % (cfg.num_hidden_layers - 1, len(keep)))
            if any(x < 1 for x in keep):
                raise ValueError("nbest_amd predict: token_keep entries must be >= 1 (got %r)" % (keep,))
            if any(y > x for x, y in zip(keep, keep[1:])):
                raise ValueError("nbest_amd predict: token_keep must be non-increasing (got %r)" % (keep,))
            if return_attns:
                raise ValueError("nbest_amd predict: return_attns with token_keep is not built (cls_attn would change width per layer)")
            if fp8:
                raise RuntimeError("nbest_amd predict: token_keep with fp8=True is not built")
            if self._head_mask is not None:
                raise RuntimeError("nbest_amd predict: token_keep under a head mask (gated or compact) is not built (the mean over "
                                   "heads under a gate is not defined here); call set_head_mask(None) first")
        elif return_token_kept:
            raise ValueError("nbest_amd predict: return_token_kept needs token_keep")
        if fp8:
            if not self.fp8_forward:
                raise RuntimeError("nbest_amd predict(fp8=True): the model was not built with fp8_forward=True (--dtype fp8w)")
            if return_attns:
                raise ValueError("nbest_amd predict(fp8=True): return_attns is not built for the fp8 inference")
            if self._head_mask is not None:
                raise RuntimeError("nbest_amd predict(fp8=True): head masks (compact or not) are not supported in fp8; clear the mask")
            if not self.fp8_calibrated:
                raise RuntimeError("nbest_amd predict(fp8=True): no activation scales - run model.fp8_calibrate(batch) on representative "
                                   "batches (or load_fp8_calibration) first")
            return self._heads_out(self._infer_fp8(input_ids, seg_ids, calibrate=False), return_logits)
        if return_attns and self._head_mask_compact:
            raise ValueError("nbest_amd predict: return_attns under a compact head mask is not built (the CLS maps are indexed by "
                             "original head); set the mask without compact=True")
        B, S = input_ids.shape
        H = cfg.hidden_size
        first_pos = cfg.pad_token_id + 1 if cfg.family in ("roberta", "xlm-roberta") else 0
        if S > 512 or S + first_pos > cfg.max_position_embeddings:     # refused before anything is enqueued (encoder.hip check_desc)
            raise RuntimeError("nbest_amd predict: S=%d does not fit the position table (%d rows)" % (S, cfg.max_position_embeddings))
        d = self._desc(B, S, "infer").desc
        ids, seg, pos, mask = self._inputs(input_ids, seg_ids)
        d.hidden_drop = d.attn_drop = 0.0
        d.seed = 0
        self._set_head_gate(d)
        self._set_weights(d, "infer")
        ws_bytes = hb.lib().nbest_encoder_infer_ws_bytes if token_keep is None else hb.lib().nbest_encoder_infer_tokens_ws_bytes
        ws = self._grow(vars(self), "_infer_ws", ws_bytes(C.byref(d)))
        a = self.arena
        cls = torch.empty(B, H, dtype=self.compute_dtype, device=self.device)
        if token_keep is not None:
            kept = torch.empty(len(keep), B, S, dtype=torch.int32, device=self.device) if return_token_kept else None
            hb.encoder_infer_tokens(d, a.weights, a.p, ids, seg, pos, mask, ws, cls, keep, kept)
            out = self._heads_out(cls, return_logits)
            if return_token_kept:
                counts = [S]
                for x in keep:
                    counts.append(min(x, counts[-1]))
                out["token_kept"], out["token_counts"] = kept, counts
            return out
        cls_attn = torch.empty(cfg.num_hidden_layers, B, cfg.num_attention_heads, S, dtype=torch.float32,
                               device=self.device) if return_attns else None
        if self._head_mask_compact:
            d.head_gate = None                                # the gate lives in the compact Wo'
            pk = self._prune.build(self, packed=d.wpk is not None)
            hb.encoder_infer_pruned(d, a.weights, a.p, ids, seg, pos, mask, ws, cls, self._prune.tab, self._prune.w, pk, self._prune.b)
        else:
            hb.encoder_infer(d, a.weights, a.p, ids, seg, pos, mask, ws, cls, cls_attn)
        out = self._heads_out(cls, return_logits)
        if return_attns:
            out["cls_attn"] = cls_attn
        return out

    def _heads_out(self, cls, return_logits):
        """the heads of an inference pass on its CLS rows [B, H]: the dict predict returns (without cls_attn)"""
        B, H = cls.shape
        Wh, bh = self.arena.heads_wb()
        labels_f = torch.zeros(B, self.labels.n_bottom, dtype=torch.float32, device=self.device)
        top, bott, fin, _, _, _, _ = hb.stc_heads(cls, H, Wh, bh, self.dls, labels_f, B, H, need_grad=False, drop_p=0.0)
        out = dict(top=top, bott=bott, final=fin, cls=cls, pred=self.decode(top, bott))
        if return_logits:
            out["logits"] = hb.stc_heads_logits(cls, H, Wh, bh, self.dls, B, H)
        return out

    # ---- fp8 inference: an explicit calibration, then static scales --------------------------------------------------------
    def _infer_fp8(self, input_ids, seg_ids, calibrate):
        """one nbest_encoder_infer_fp8 pass -> cls [B, H].  ``calibrate``: the bf16 launches of predict plus the amax records of the
        GEMM inputs into arena.iamax_slots; else the fp8 pass on the history arena.iamax, which records nothing.  A descriptor of its
        own ("infer8"): the fp8 fields are set per call, the training descriptors and histories are not touched."""
        cfg, a = self.cfg, self.arena
        B, S = input_ids.shape
        first_pos = cfg.pad_token_id + 1 if cfg.family in ("roberta", "xlm-roberta") else 0
        if S > 512 or S + first_pos > cfg.max_position_embeddings:
            raise RuntimeError("nbest_amd predict: S=%d does not fit the position table (%d rows)" % (S, cfg.max_position_embeddings))
        d = self._desc(B, S, "infer8").desc
        ids, seg, pos, mask = self._inputs(input_ids, seg_ids)
        d.hidden_drop = d.attn_drop = 0.0
        d.seed = 0
        d.head_gate = d.head_gate_grad = None
        self._set_weights(d, "infer")
        d.w8, d.w8_inv_scale = a.w8.data_ptr(), a.w8_inv_scale.data_ptr()
        d.w8p = a.w8p.data_ptr() if a.w8p is not None else None
        d.fp8_act = int(not calibrate)
        d.aamax_prev = None if calibrate else a.iamax.data_ptr()
        d.aamax_new = a.iamax_slots.data_ptr() if calibrate else None
        ws = self._grow(vars(self), "_infer_ws", hb.lib().nbest_encoder_infer_fp8_ws_bytes(C.byref(d)))
        cls = torch.empty(B, cfg.hidden_size, dtype=self.compute_dtype, device=self.device)
        hb.encoder_infer_fp8(d, a.weights, a.p, ids, seg, pos, mask, ws, cls)
        return cls

    def fp8_calibrate(self, input_ids, seg_ids=None, reset=False):
        """Record the activation scales predict(fp8=True) runs on, from one batch: the calibration pass of nbest_encoder_infer_fp8 (the
        launches of the bf16 predict plus one amax launch per fp8 GEMM input) and the heads, then the recorded amax folded into the
        inference history with a maximum (nbest_fp8_amax_fold_max), so several calls cover several batches; ``reset=True`` starts
        over.  Returns what ``predict`` returns for the batch - the bits of the bf16 predict.  No host synchronisation; no training
        state is touched.  The scale of a tensor is 2^floor(log2(224 / amax)): a value up to twice the calibrated amax is
        representable, beyond that the e4m3 cast saturates silently - calibrate on data like the data to be labelled."""
        if not self.fp8_forward:
            raise RuntimeError("nbest_amd fp8_calibrate: the model was not built with fp8_forward=True (--dtype fp8w)")
        if self._head_mask is not None:
            raise RuntimeError("nbest_amd fp8_calibrate: head masks are not supported in fp8; clear the mask")
        if reset:
            self.arena.iamax.zero_()
            self.fp8_calibrated = 0
        cls = self._infer_fp8(input_ids, seg_ids, calibrate=True)
        hb.fp8_amax_fold_max(self.arena.iamax_slots, self.arena.iamax)
        self.fp8_calibrated += 1
        return self._heads_out(cls, False)

    def fp8_calibration(self):
        """the inference history as fp32 [L, 4] (a copy): the calibrated amax of x, ctx, x1, gelu(u) per layer (the last layer: x only)"""
        if not self.fp8_forward:
            raise RuntimeError("nbest_amd fp8_calibration: the model was not built with fp8_forward=True")
        return self.arena.iamax.view(torch.float32).view(self.cfg.num_hidden_layers, 4).clone()

    def load_fp8_calibration(self, t):
        """install a history ``fp8_calibration()`` returned (for these weights: a server keeps it next to model.pt); counts as one batch"""
        if not self.fp8_forward:
            raise RuntimeError("nbest_amd load_fp8_calibration: the model was not built with fp8_forward=True")
        t = torch.as_tensor(t, dtype=torch.float32)
        if tuple(t.shape) != (self.cfg.num_hidden_layers, 4) or not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
            raise ValueError("nbest_amd load_fp8_calibration: expected finite non-negative fp32 [L=%d, 4]" % self.cfg.num_hidden_layers)
        self.arena.iamax.copy_(t.contiguous().view(torch.int32).view(-1).to(self.device))
        self.arena.iamax_slots.zero_()
        self.fp8_calibrated = 1

    # ---- integrated-gradients attribution (forward + input-gradient backward, no parameter gradient) ------------------------
    def default_baseline(self, input_ids):
        """the default IG baseline: every non-padding token except position 0 ([CLS] / <s>) replaced by the pad id"""
        pad = self.cfg.pad_token_id
        base = torch.where(input_ids.ne(pad), torch.full_like(input_ids, pad), input_ids)
        base[:, 0] = input_ids[:, 0]
        return base

    def attribute(self, input_ids, seg_ids=None, targets=None, steps=32, baseline_ids=None, max_rows=256):
        """Integrated gradients (Sundararajan et al., 2017) of the STC final score F = final[row, c] w.r.t. the word embeddings of
        the ASR pass, one share per token: A[t] = (1/m) sum_k dF/dE_t(a_k) . (word[x_t] - word[x'_t]), a_k = (k + 1/2) / m,
        E_t(a) = ((1 - a) word[x'_t] + a word[x_t]) + type + position (positions, token types and key mask those of x).
        ``targets``: [P, 2] (row, bottom label); None = every label predict() decodes, rows in order.  ``baseline_ids``: x' (must
        keep the padding of input_ids); None = default_baseline.  Path rows (m per pair) and a forward-only a = 0 and a = 1 row per
        utterance run in encoder calls of at most ``max_rows`` sequences; a pair's rows are never split and every call holds at least
        one pair, so a call exceeds ``max_rows`` only when one pair's m + 2 rows do (any ``steps`` >= 1 runs).
        Returns dict(attr fp32 [P, S], row, label (int64 [P]), score = F at a = 1, baseline_score = F at a = 0 (fp32 [P])):
        sum_t attr ~ score - baseline_score (completeness, up to the Riemann error of m points).
        Touches no training state, as predict(); an fp8w model attributes on its bf16 weight copy.  One GPU."""
        cfg, a = self.cfg, self.arena
        m, max_rows = int(steps), int(max_rows)
        if m < 1:
            raise ValueError("nbest_amd attribute: steps must be >= 1 (got %d)" % m)
        if max_rows < 1:
            raise ValueError("nbest_amd attribute: max_rows must be >= 1 (got %d)" % max_rows)
        B, S = input_ids.shape
        H, L = cfg.hidden_size, cfg.num_hidden_layers
        first_pos = cfg.pad_token_id + 1 if cfg.family in ("roberta", "xlm-roberta") else 0
        if S > 512 or S + first_pos > cfg.max_position_embeddings:
            raise RuntimeError("nbest_amd attribute: S=%d does not fit the position table (%d rows)" % (S, cfg.max_position_embeddings))
        ids = input_ids.to(self.device).long().contiguous()
        pad = cfg.pad_token_id
        if baseline_ids is None:
            base = self.default_baseline(ids)
        else:
            base = baseline_ids.to(self.device).long().contiguous()
            if base.shape != ids.shape:
                raise ValueError("nbest_amd attribute: baseline_ids %s != input_ids %s" % (tuple(base.shape), tuple(ids.shape)))
            if bool(base[ids.eq(pad)].ne(pad).any()):
                raise ValueError("nbest_amd attribute: baseline_ids must keep the padding of input_ids (pad id %d)" % pad)
        seg = None if seg_ids is None else seg_ids.to(self.device).long().contiguous()
        if targets is None:
            pred = self.predict(ids, seg)["pred"].cpu().tolist()
            targets = [(b, c) for b in range(B) for c in pred[b] if c >= 0]
        tg = [(int(b), int(c)) for b, c in (targets.tolist() if torch.is_tensor(targets) else targets)]
        for b, c in tg:
            if not (0 <= b < B and 0 <= c < self.labels.n_bottom):
                raise ValueError("nbest_amd attribute: target (%d, %d) outside rows [0, %d) / labels [0, %d)" % (b, c, B, self.labels.n_bottom))
        P = len(tg)
        f = dict(dtype=torch.float32, device=self.device)
        out = dict(attr=torch.zeros(P, S, **f), row=torch.tensor([b for b, _ in tg], dtype=torch.long),
                   label=torch.tensor([c for _, c in tg], dtype=torch.long), score=torch.zeros(P, **f), baseline_score=torch.zeros(P, **f))
        if P == 0:
            return out
        # calls: a pair's m rows never split, every call holds at least one pair (then it may exceed max_rows); an utterance's
        # a = 0 / a = 1 rows ride in the call of its first pair
        calls, cur, rows, seen = [], [], 0, set()
        for i, (b, _) in enumerate(tg):
            cost = m + (0 if b in seen else 2)
            if cur and rows + cost > max_rows:
                calls.append(cur)
                cur, rows = [], 0
            cur.append(i)
            rows += cost
            seen.add(b)
        calls.append(cur)
        pre = "bert_encoder.embeddings."
        w16 = a.weights
        word, ttab, ptab = (a.view(w16, pre + n) for n in ("word_embeddings.weight", "token_type_embeddings.weight", "position_embeddings.weight"))
        gamma = a.view(a.p, pre + "LayerNorm.weight")
        Wh, bh = a.heads_wb()
        R, nt, nb = self.dls.n_rows, self.labels.n_top, self.labels.n_bottom
        path_alpha = (torch.arange(m, dtype=torch.float64) + 0.5) / m
        extras, ends = set(), {}                             # utterances whose a = 0 / a = 1 rows already ran; their final rows
        for call in calls:
            rows_b = [tg[i][0] for i in call]
            xs = []
            for b in rows_b:
                if b not in extras and b not in xs:
                    xs.append(b)
            extras.update(xs)
            n = len(call)
            Bc = n * m + 2 * len(xs)
            seq = torch.tensor([b for b in rows_b for _ in range(m)] + [b for b in xs for _ in range(2)], dtype=torch.long, device=self.device)
            alpha = torch.cat([path_alpha.repeat(n), torch.tensor([0.0, 1.0], dtype=torch.float64).repeat(len(xs))]).to(**f)
            ids_c, base_c = ids[seq].contiguous(), base[seq].contiguous()
            ids_c, seg_c, pos_c, mask_c = self._inputs(ids_c, None if seg is None else seg[seq])
            ps = self._desc(Bc, S, "attrib")
            d = ps.desc
            act = self._grow(self._stash, "attrib", ps.act_bytes)[:ps.act_bytes]
            ws = self._grow(vars(self), "_attr_ws", hb.lib().nbest_encoder_ws_bytes(C.byref(d)))
            d.hidden_drop = d.attn_drop = 0.0
            d.seed = 0
            d.base_ids, d.alpha = base_c.data_ptr(), alpha.data_ptr()
            self._set_head_gate(d)                           # a mask gates the forward and scales the backward's dctx; no gate gradient
            self._set_weights(d, "infer")
            hid = C.c_void_p()
            hb.check(hb.lib().nbest_encoder_forward(C.byref(d), hb.ptr(a.weights), hb.ptr(a.p), hb.ptr(ids_c), hb.ptr(seg_c), hb.ptr(pos_c),
                                                    hb.ptr(mask_c), hb.ptr(act), act.numel(), hb.ptr(ws), ws.numel(), C.byref(hid),
                                                    hb.stream_ptr()), "encoder_forward(attribute)")
            esz = 2 if self.compute_dtype == torch.bfloat16 else 4
            off = hid.value - act.data_ptr()
            hidden = act[off:off + Bc * S * H * esz].view(self.compute_dtype).view(Bc * S, H)
            hws = self._grow(vars(self), "_attr_heads_ws", hb.lib().nbest_heads_ws_bytes(Bc, R, H))
            top, bott, fin, _, _, _, _ = hb.stc_heads(hidden, S * H, Wh, bh, self.dls, torch.zeros(Bc, nb, **f), Bc, H, need_grad=False,
                                                      drop_p=0.0, ws=hws)
            dfin = torch.zeros(Bc, nb, **f)
            lab = torch.tensor([tg[i][1] for i in call], dtype=torch.long, device=self.device)
            dfin[torch.arange(n * m, device=self.device), lab.repeat_interleave(m)] = 1.0
            dWh_s, dbh_s = torch.empty(R, H, **f), torch.empty(R, **f)   # the heads' parameter gradients: scratch, never read
            dcls = hb.stc_heads_vjp(Wh, self.dls, top, bott, torch.zeros(Bc, nt, **f), torch.zeros(Bc, R - nt, **f), dfin, Bc, H, dWh_s, dbh_s,
                                    hws, accumulate=False)
            dh = self._grow(vars(self), "_attr_dh", Bc * S * H, self.compute_dtype)[:Bc * S * H].view(Bc * S, H)
            dh = hb.cls_grad_scatter(dcls, Bc, S, H, self.compute_dtype, out=dh)
            d.no_param_grad = 1
            wt = None if a.w16t_stale else a.w16t           # a stale transposed copy is not read (and not refreshed): transposed reads of wts
            if wt is None:
                d.wpkt = None
            hb.check(hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(a.weights), hb.ptr(wt), hb.ptr(a.p), None, hb.ptr(ids_c),
                                                     hb.ptr(seg_c), hb.ptr(pos_c), hb.ptr(mask_c), hb.ptr(act), act.numel(), hb.ptr(dh),
                                                     hb.ptr(ws), ws.numel(), 0, 0, L, 0, hb.stream_ptr()), "encoder_backward(attribute)")
            d.no_param_grad = 0
            d.base_ids = d.alpha = None
            # the pairs of a call are consecutive targets: their rows of attr are written in place
            hb.embed_attrib(ids_c, base_c, alpha, seg_c, pos_c, word, ttab, ptab, gamma, dh, n, m, S, cfg.layer_norm_eps,
                            out=out["attr"][call[0]:call[-1] + 1])
            for j, b in enumerate(xs):                       # F at a = 0 and a = 1 of the utterances whose extra rows ran here
                ends[b] = fin[n * m + 2 * j:n * m + 2 * j + 2]
        for i, (b, c) in enumerate(tg):
            out["baseline_score"][i] = ends[b][0, c]
            out["score"][i] = ends[b][1, c]
        return out

    # ---- head importance: the gradient of the loss w.r.t. the head gates (Michel et al., 2019) ----------------------------------
    def head_gate_grad(self, input_ids, labels_f, seg_ids=None):
        """d L_b / d xi[l, h] for every utterance b of the batch: ``grad`` fp32 [L, B, heads], the gradient of the training loss of
        the ASR pass (BCE(final) + BCE(top) + mean-CE, a sum over utterances - no MSE term) w.r.t. a gate xi on head h of layer l,
        at the current mask (ones when none is set).  A pruned head (gate 0) has a gradient too, in general non-zero.
        The stash forward without dropout (in either mode), the heads' analytic backward, then nbest_encoder_backward with
        no_param_grad and head_gate_grad: no parameter gradient is formed (the heads' go to scratch).  Returns dict(grad,
        loss_parts[4] (device)).  Touches no training state, as predict() and attribute() (a stash slot of its own); an fp8w model
        runs its bf16 weight copy.  One GPU."""
        cfg, a = self.cfg, self.arena
        B, S = input_ids.shape
        H, L, heads = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
        first_pos = cfg.pad_token_id + 1 if cfg.family in ("roberta", "xlm-roberta") else 0
        if S > 512 or S + first_pos > cfg.max_position_embeddings:
            raise RuntimeError("nbest_amd head_gate_grad: S=%d does not fit the position table (%d rows)" % (S, cfg.max_position_embeddings))
        f = dict(dtype=torch.float32, device=self.device)
        ids, seg, pos, mask = self._inputs(input_ids.to(self.device).long(), None if seg_ids is None else seg_ids.to(self.device).long())
        gate = self._head_mask if self._head_mask is not None else torch.ones(L, heads, **f)
        grad = torch.empty(L, B, heads, **f)
        ps = self._desc(B, S, "headgrad")
        d = ps.desc
        act = self._grow(self._stash, "headgrad", ps.act_bytes)[:ps.act_bytes]
        ws = self._grow(vars(self), "_hg_ws", hb.lib().nbest_encoder_ws_bytes(C.byref(d)))
        d.hidden_drop = d.attn_drop = 0.0
        d.seed = 0
        d.head_gate, d.head_gate_grad = gate.data_ptr(), None
        try:                                                 # whatever raises, the cached descriptor keeps no pointer of this call
            self._set_weights(d, "infer")
            hid = C.c_void_p()
            hb.check(hb.lib().nbest_encoder_forward(C.byref(d), hb.ptr(a.weights), hb.ptr(a.p), hb.ptr(ids), hb.ptr(seg), hb.ptr(pos),
                                                    hb.ptr(mask), hb.ptr(act), act.numel(), hb.ptr(ws), ws.numel(), C.byref(hid),
                                                    hb.stream_ptr()), "encoder_forward(head_gate_grad)")
            esz = 2 if self.compute_dtype == torch.bfloat16 else 4
            off = hid.value - act.data_ptr()
            hidden = act[off:off + B * S * H * esz].view(self.compute_dtype).view(B * S, H)
            Wh, bh = a.heads_wb()
            R = self.dls.n_rows
            hws = self._grow(vars(self), "_hg_heads_ws", hb.lib().nbest_heads_ws_bytes(B, R, H))
            dWh_s, dbh_s = torch.empty(R, H, **f), torch.empty(R, **f)       # the heads' parameter gradients: scratch, never read
            _, _, _, loss, dcls, _, _ = hb.stc_heads(hidden, S * H, Wh, bh, self.dls, labels_f.to(**f).contiguous(), B, H, need_grad=True,
                                                     accumulate=False, drop_p=0.0, dWh=dWh_s, dbh=dbh_s, ws=hws)
            dh = self._grow(vars(self), "_hg_dh", B * S * H, self.compute_dtype)[:B * S * H].view(B * S, H)
            dh = hb.cls_grad_scatter(dcls, B, S, H, self.compute_dtype, out=dh)
            d.no_param_grad = 1
            d.head_gate_grad = grad.data_ptr()
            wt = None if a.w16t_stale else a.w16t               # as attribute(): a stale transposed copy is neither read nor refreshed
            if wt is None:
                d.wpkt = None
            hb.check(hb.lib().nbest_encoder_backward(C.byref(d), hb.ptr(a.weights), hb.ptr(wt), hb.ptr(a.p), None, hb.ptr(ids), hb.ptr(seg),
                                                     hb.ptr(pos), hb.ptr(mask), hb.ptr(act), act.numel(), hb.ptr(dh), hb.ptr(ws), ws.numel(),
                                                     0, 0, L, 0, hb.stream_ptr()), "encoder_backward(head_gate_grad)")
        finally:
            d.no_param_grad = 0
            d.head_gate = d.head_gate_grad = None
        return dict(grad=grad, loss_parts=loss)

    def decode(self, top, bott, out=None):
        """device decode of pred_one_sample -> int32 [B, n_top] bottom-label index or -1 (``out``: see hipabi.stc_decode)"""
        return hb.stc_decode(top, bott, self.dls, out=out)


def make_model(opt):
    """Drop-in for /root/reference/models/model.py:7-9.  ``opt`` carries the reference's fields:
    pre_trained_model ('bert' | 'xlm-roberta' | ...), top2bottom_dict, dropout, device; optional build
    extensions: encoder_config (EncoderConfig), compute_dtype, idx2label, random_seed."""
    cfg = getattr(opt, "encoder_config", None) or NAMED[getattr(opt, "pre_trained_model", None) or "bert"]()
    labels = LabelSpace(opt.top2bottom_dict, list(getattr(opt, "idx2label", []) or []))
    return NBestSTCModel(cfg, labels, device=getattr(opt, "device", "cuda"),
                         compute_dtype=getattr(opt, "compute_dtype", torch.bfloat16), dropout=getattr(opt, "dropout", 0.0),
                         seed=getattr(opt, "random_seed", 999), fp8_forward=getattr(opt, "fp8_forward", False),
                         fp8_backward=getattr(opt, "fp8_backward", None))
