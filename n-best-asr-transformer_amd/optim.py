"""BertAdam (and torch Adam / HF AdamW: ``HipAdam``) over the flat parameter arena, one multi-tensor HIP launch set per step.

Interface and semantics of /root/reference/models/optimization.py:183-302 as driven by
/root/reference/n_best_asr_bert.py:540-561: each parameter tensor is its own group (lr = bert_lr for
``bert_encoder.*`` else lr; weight_decay 0.01 except bias / LayerNorm), gradient clipped PER TENSOR to
L2 norm 1.0, no bias correction, eps 1e-6, ``warmup_linear`` schedule evaluated at the step count
BEFORE the increment.
"""
import contextlib

import torch
import torch.distributed as dist

from . import hipabi as hb
from .model import freeze_plan


def warmup_linear(step, t_total, warmup):
    """optimization.py:162-171 (+ :60-61: t_total < 0 disables the schedule)"""
    if t_total < 0:
        return 1.0
    x = float(step) / float(t_total)
    if x < warmup:
        return x / warmup
    return max((x - 1.0) / (warmup - 1.0), 0.0)


def ema_decay_at(t, decay):
    """decay of the weight average at optimizer step ``t`` (1-based: the step being taken): the usual warm-up
    min(decay, (1 + t) / (10 + t)), so that a short run's average is not dominated by the initial weights"""
    return min(float(decay), (1.0 + t) / (10.0 + t))


class HipBertAdam:
    """``shard`` (data parallel, new functionality - the reference is single-process): the optimizer SHARDED over the ranks instead
    of replicated.  Every rank owns a contiguous range of the optimizer's blocks (16 384 elements of one tensor each; about 1/world of
    the elements, separately for the encoder-layer / head tensors and for the embedding tables, which are updated after their own, last,
    gradient exchange) and with it that range of the arenas:
      * gradients travel as REDUCE to the owner (trainer.GradReducer(owner_ranges=...)) - half the bytes of the all-reduce;
      * per-tensor clip: each rank computes the block sums of squares of its own blocks into a zeroed vector, which is
        SUM-all-reduced (n_blocks floats, 27 KB for bert-base): x + 0 is exact, so every rank holds exactly the numbers one process
        computes, and the clip coefficients - hence the updates - are bit-identical to the replicated optimizer's;
      * each rank updates p, m, v and the bf16 compute copy of its own range only (1/world of the optimizer's HBM traffic);
      * the owners then broadcast what the next step reads: the bf16 compute copy of their range (2 B per parameter) and, gathered
        into one small buffer, the fp32 values of the tensors the kernels read from the master arena (biases, LayerNorm parameters,
        STC heads: 0.26 M of bert-base's 109.6 M parameters).  Bytes per parameter and step: 4 (reduce) + 2 (bf16 copy) against 8 for
        the all-reduce: 0.75 x.  With fp32 compute (the parity path) the fp32 range itself is broadcast.
    A rank's fp32 master and moments are then current only inside its own range: ``gather_master()`` (called by ``state_dict`` and
    before a checkpoint is written) re-assembles them everywhere.  Not combined with the fp8 mode (the e4m3 weight copies are
    quantised from the full fp32 master after every step): ``shard`` is ignored there.

    ``ema_decay`` (new functionality; None: nothing allocated, nothing launched): ``arena.ema``, an fp32 arena of the layout of ``p``
    that starts as its clone, follows the trainable tensors as ema += (1 - d_t) (p - ema), d_t = ema_decay_at(t, ema_decay), by one
    nbest_ema_update per descriptor table right after that table's update (under data parallelism the main table's runs under the
    embedding exchange, like its update; the replicas compute the same bits).  A frozen tensor is skipped: its average is its
    value.  ``ema_weights()`` swaps the average in for an evaluation or a checkpoint.  Not built for the sharded optimizer (the
    master is current only on each range's owner: the kernel would need an owner-range form and every evaluation a gather):
    ``shard`` together with ``ema_decay`` raises.

    ``sam_perturb`` / ``sam_restore`` (new functionality: sharpness-aware minimization, trainer.train_step(sam_rho=)): the weight-
    space half of a SAM / ASAM step through the K9s kernels.  ``sam_perturb(rho)`` moves every trainable tensor to w + e,
    e = rho g / ||g|| with ONE norm over both descriptor tables (adaptive: e = rho T^2 g / ||T g||, T = |w| + eta), keeps w in
    ``sam_backup`` (fp32, the size of ``p``; None until the first call) and refreshes the bf16 copy and the derived weight images;
    the next ``step_main()`` (or ``sam_restore()``) moves w back, to the bit, before it steps.  Frozen tensors are neither moved nor
    in the norm.  Not built for the sharded optimizer or with LoRA; refused while the EMA weights are swapped in."""

    def __init__(self, model, lr, bert_lr=None, warmup=-1, t_total=-1, b1=0.9, b2=0.999, e=1e-6, max_grad_norm=1.0, shard=False,
                 ema_decay=None, lora_lr=None):
        self.lora_lr = lr if lora_lr is None else lora_lr
        self._lora = None           # the model.lora the adapter descriptors below were built for
        self._lora_part = None      # (descs, n_tensors, n_blocks, workspace) of the adapter arena
        if getattr(model, "lora", None) is not None:
            self._refuse_with_lora(shard, ema_decay)
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.0 <= ema_decay < 1.0:
                raise ValueError("ema_decay must be in [0, 1), not %r" % (ema_decay,))
            if shard:
                raise ValueError("ema_decay is not built for the sharded optimizer (shard=True): the fp32 master is current only on "
                                 "each range's owner")
        self.ema_decay, self._in_ema = ema_decay, False
        self.model, self.arena = model, model.arena
        self.lr, self.bert_lr = lr, lr if bert_lr is None else bert_lr
        self.warmup, self.t_total = max(warmup, 0.0), t_total
        self.b1, self.b2, self.e, self.max_grad_norm = b1, b2, e, max_grad_norm
        self.step_count = 0
        self.sam_backup, self.sam_norm, self.sam_pending = None, None, False   # sam_perturb: w, the device [1] norm, w + e is in p
        self._sam_partial = self._sam_clip = None
        a = self.arena
        self._frozen_key = None     # requires_grad pattern the descriptors were built for (model.FreezePlan.key)
        self._trainable = None      # its trainable tensor names (None: every tensor but the pooler)
        if hasattr(model, "_params"):
            plan = freeze_plan(model)
            self._frozen_key, self._trainable = plan.key, plan.trainable
        if a.m is None:
            a.m = torch.zeros_like(a.p)
            a.v = torch.zeros_like(a.p)
        # two launch sets: everything but the embedding tables, and the embedding tables.  Under data parallelism the
        # tables' gradients are the last to be exchanged (the embedding backward is the last kernel); updating the other
        # 85 M parameters meanwhile hides most of that exchange.
        is_emb = lambda name: name.startswith("bert_encoder.embeddings.")
        self.parts = []
        self._selects = (lambda n: not is_emb(n), is_emb)
        for sel in self._selects:
            descs, n_t, n_b = self._build_descs(sel)
            ws = torch.empty((n_b + n_t + 16) * 4, dtype=torch.uint8, device=a.device)
            self.parts.append((descs, n_t, n_b, ws))
        self.rank, self.world = 0, 1
        if dist.is_available() and dist.is_initialized():
            self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.sharded = bool(shard) and self.world > 1 and getattr(a, "w8", None) is None
        self.owner_ranges = None
        if self.sharded:
            self._plan_shards()
        if self.ema_decay is not None:
            self.reset_ema()

    # ---- weight average ------------------------------------------------------------------------------------------------------
    def reset_ema(self):
        """start the average over from the current weights (for a caller who loads weights after building the optimizer)"""
        if self.ema_decay is None:
            raise RuntimeError("reset_ema: the optimizer was built without ema_decay")
        if self._in_ema:
            raise RuntimeError("reset_ema inside ema_weights(): the arenas are exchanged")
        self.arena.ema = self.arena.p.clone()

    def _ema_update(self, part):
        """ema += (1 - d_t) (p - ema) over the active tensors of one descriptor table, t = the step being taken"""
        descs, n_t, n_b, _ = self.parts[part]
        if self.ema_decay is None or n_t == 0:
            return
        a = self.arena
        w = 1.0 - ema_decay_at(self.step_count + 1, self.ema_decay)
        hb.check(hb.lib().nbest_ema_update(hb.ptr(a.ema), hb.ptr(a.p), hb.ptr(descs), n_t, n_b, w, hb.stream_ptr()), "ema_update")

    def _ema_exchange(self):
        a = self.arena
        for descs, n_t, n_b, _ in self.parts:
            if n_t:
                hb.check(hb.lib().nbest_ema_exchange(hb.ptr(a.p), hb.ptr(a.ema), hb.ptr(a.w16), hb.ptr(descs), n_t, n_b, hb.stream_ptr()),
                         "ema_exchange")
        a.refresh_transposed()          # the derived images an optimizer step refreshes: transposed / packed (or lazily), e4m3

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights():`` - the model computes with (and ``state_dict()`` / ``save_model`` hold) the averaged
        weights: p and ema are exchanged in place (nbest_ema_exchange, no temporary arena), the bf16 copy is rewritten and the
        derived weight images refreshed as after an optimizer step; the exit exchanges them back, to the bit.  No optimizer step
        inside, no nesting.  The fp8 amax histories are left as they are."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights: the optimizer was built without ema_decay")
        if self._in_ema:
            raise RuntimeError("ema_weights() is already entered: it does not nest")
        if self.sam_pending:
            raise RuntimeError("ema_weights() while a SAM perturbation is pending: the model holds w + e (step or sam_restore() first)")
        self._ema_exchange()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._ema_exchange()

    def _refuse_step_in_ema(self):
        if self._in_ema:
            raise RuntimeError("optimizer step inside ema_weights(): the model holds the averaged weights")

    def _ema_state(self):
        """the state_dict entries of the average ({} without one)"""
        if self.ema_decay is None:
            return {}
        if self._in_ema:
            raise RuntimeError("state_dict inside ema_weights(): the arenas are exchanged; take it outside")
        a = self.arena
        return dict(ema={s.name: a.view(a.ema, s.name).detach().cpu().clone() for s in a.slots}, ema_decay=self.ema_decay)

    def _load_ema_state(self, sd, into):
        """``into``: how this optimizer is named in the kind-mismatch message"""
        has = sd.get("ema") is not None
        if has != (self.ema_decay is not None):
            raise ValueError("optimizer state %s a weight average cannot be loaded into %s %s one (--ema_decay must match the run "
                             "that wrote it)" % ("with" if has else "without", into, "without" if has else "with"))
        if has:
            if self._in_ema:
                raise RuntimeError("load_state_dict inside ema_weights(): the arenas are exchanged")
            a = self.arena
            for s in a.slots:
                a.view(a.ema, s.name).copy_(sd["ema"][s.name])

    # ---- sharpness-aware minimization (K9s) -------------------------------------------------------------------------------------
    def sam_perturb(self, rho, adaptive=False, eta=0.01):
        """p += e over the trainable tensors, e = rho g / ||g|| (``adaptive``: rho T^2 g / ||T g||, T = |p| + eta), g = ``arena.g``:
        the norms of both descriptor tables back to back, nbest_adam_clip_coef's fixed-order total into ``sam_norm`` (device [1]),
        one nbest_sam_perturb per table (which also saves p into ``sam_backup`` and rewrites the bf16 copy), then the derived weight
        images.  rho finite and >= 0 (0: nothing moves), eta finite and > 0.  No host synchronisation.  Raises before anything is
        enqueued when a perturbation is pending, the optimizer is sharded, LoRA is on or the EMA weights are swapped in."""
        rho, eta = float(rho), float(eta)
        if not (rho >= 0.0 and rho != float("inf")):
            raise ValueError("sam_perturb: rho must be finite and >= 0, not %r" % (rho,))
        if adaptive and not (eta > 0.0 and eta != float("inf")):
            raise ValueError("sam_perturb: eta must be finite and > 0, not %r" % (eta,))
        if self.sam_pending:
            raise RuntimeError("sam_perturb: a perturbation is pending (step or sam_restore() first)")
        if self.sharded:
            raise RuntimeError("nbest_amd: SAM with the sharded optimizer is not built (the fp32 master is current only on each "
                               "range's owner)")
        if getattr(self.model, "lora", None) is not None:
            raise RuntimeError("nbest_amd: SAM on a model with LoRA enabled is not built (the perturbation would have to follow "
                               "the factors, not the merged weights)")
        if self._in_ema:
            raise RuntimeError("sam_perturb inside ema_weights(): the model holds the averaged weights")
        self.sync_frozen()
        a, L, P, st = self.arena, hb.lib(), hb.ptr, hb.stream_ptr()
        if self.sam_backup is None:
            self.sam_backup = torch.zeros_like(a.p)
            self._sam_partial = torch.zeros(max(self.parts[0][2] + self.parts[1][2], 1), dtype=torch.float32, device=a.device)
            self._sam_clip = torch.zeros(2, dtype=torch.float32, device=a.device)         # [unused coefficient, total norm]
            self.sam_norm = self._sam_clip[1:2]
        base = 0
        for descs, n_t, n_b, _ in self.parts:
            if n_t:
                if adaptive:
                    hb.check(L.nbest_sam_norms(P(a.p), P(a.g), P(descs), n_t, n_b, eta, P(self._sam_partial[base:]), st), "sam_norms")
                else:
                    hb.check(L.nbest_bertadam_norms(P(a.g), P(descs), n_t, n_b, 0, n_b, P(self._sam_partial[base:]), st), "bertadam_norms")
            base += n_b
        hb.check(L.nbest_adam_clip_coef(P(self._sam_partial), self._sam_partial.numel(), 0.0, P(self._sam_clip), st), "adam_clip_coef")
        for descs, n_t, n_b, _ in self.parts:
            if n_t:
                hb.check(L.nbest_sam_perturb(P(a.p), P(a.g), P(self.sam_backup), P(a.w16), P(descs), n_t, n_b, P(self.sam_norm), rho,
                                             eta if adaptive else -1.0, st), "sam_perturb")
        self.sam_pending = True
        a.refresh_transposed()

    def _sam_restore_launch(self):
        """p = sam_backup (+ the bf16 copy) over the tables the pending perturbation used; the caller refreshes the derived images"""
        a = self.arena
        for descs, n_t, n_b, _ in self.parts:
            if n_t:
                hb.check(hb.lib().nbest_sam_restore(hb.ptr(a.p), hb.ptr(self.sam_backup), hb.ptr(a.w16), hb.ptr(descs), n_t, n_b,
                                                    hb.stream_ptr()), "sam_restore")
        self.sam_pending = False

    def sam_restore(self):
        """undo a pending sam_perturb without stepping: every bit of p, the bf16 copy and the derived images is what it was.
        ``ema_weights()`` refuses to be entered while a perturbation is pending, and this call inside it"""
        if not self.sam_pending:
            raise RuntimeError("sam_restore: no perturbation is pending")
        if self._in_ema:
            raise RuntimeError("sam_restore inside ema_weights(): the arenas are exchanged")
        self._sam_restore_launch()
        self.arena.refresh_transposed()

    # ---- sharding plan (identical on every rank: pure geometry) -------------------------------------------------------------
    def _plan_shards(self):
        a, W = self.arena, self.world
        self.blk_bounds, self.elem_ranges, self.small_idx, self.partials, self.coefs = [], [], [], [], []
        for part, sel in enumerate(self._selects):
            blocks = a.block_table(sel, self._active())
            n_t, n_b = self.parts[part][1], self.parts[part][2]
            assert len(blocks) == n_b, (len(blocks), n_b)
            weight = [n if act else 0 for _, n, act in blocks]
            total, acc, cuts = sum(weight), 0, [0]
            for i, w in enumerate(weight):                      # rank r's range ends where the running total passes (r + 1) / W of the elements
                acc += w
                while len(cuts) < W and acc * W >= total * len(cuts):
                    cuts.append(i + 1)
            while len(cuts) < W:
                cuts.append(n_b)
            cuts.append(n_b)
            bb = [(cuts[r], max(cuts[r], cuts[r + 1])) for r in range(W)]
            er = [(blocks[lo][0], blocks[hi - 1][0] + blocks[hi - 1][1]) if hi > lo else (0, 0) for lo, hi in bb]
            self.blk_bounds.append(bb)
            self.elem_ranges.append(er)
            idx = []
            smalls = a.fp32_read_slots(sel)
            for r, (lo, hi) in enumerate(er):
                pieces = [torch.arange(max(s.offset, lo), min(s.offset + s.numel, hi), dtype=torch.long) for s in smalls
                          if min(s.offset + s.numel, hi) > max(s.offset, lo)]
                idx.append((torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.long)).to(a.device))
            self.small_idx.append(idx)
            self.partials.append(torch.zeros(max(n_b, 1), dtype=torch.float32, device=a.device))
            self.coefs.append(torch.zeros(max(n_t, 1), dtype=torch.float32, device=a.device))
        # what trainer.GradReducer needs: per rank, the arena ranges whose reduced gradient it must receive
        self.owner_ranges = [[self.elem_ranges[p_][r] for p_ in range(len(self.parts)) if self.elem_ranges[p_][r][1] > self.elem_ranges[p_][r][0]]
                             for r in range(W)]

    # ---- LoRA (model.enable_lora): the adapter arena next to the main one ------------------------------------------------------
    def _refuse_with_lora(self, shard, ema_decay):
        if type(self) is not HipBertAdam:
            raise RuntimeError("nbest_amd: %s on a model with LoRA enabled is not built (its global-norm clip would have to span "
                               "the main and the adapter arena); use HipBertAdam" % type(self).__name__)
        if shard:
            raise RuntimeError("nbest_amd: the sharded optimizer on a model with LoRA enabled is not built")
        if ema_decay is not None:
            raise RuntimeError("nbest_amd: ema_decay on a model with LoRA enabled is not built (the average would have to follow "
                               "the factors, not the merged weights)")

    def _sync_lora(self):
        """the adapter descriptors, moments and workspace of the model's current LoraState (None: LoRA is off)"""
        st = getattr(self.model, "lora", None)
        if st is self._lora:
            return st
        if st is not None:
            self._refuse_with_lora(self.sharded, self.ema_decay)
            if st.m is None:
                st.m, st.v = torch.zeros_like(st.p), torch.zeros_like(st.p)
            descs, n_t, n_b = st.build_descs(self.lora_lr)
            self._lora_part = (descs, n_t, n_b, torch.empty((n_b + n_t + 16) * 4, dtype=torch.uint8, device=st.device))
        else:
            self._lora_part = None
        self._lora = st
        return st

    def _step_lora(self, st):
        """step_main with LoRA on: project the dense gradient onto the factors, BertAdam on the main arena (only the heads are
        active) and on the adapter arena (same schedule position, lora_lr, decay 0.01, per-tensor clip), merge"""
        st.project_grad(self.arena)
        self._launch(0)
        descs, n_t, n_b, ws = self._lora_part
        hb.check(hb.lib().nbest_bertadam_step(hb.ptr(st.p), hb.ptr(st.g), hb.ptr(st.m), hb.ptr(st.v), None, hb.ptr(descs), n_t, n_b,
                                              self.get_lr_mult(), self.b1, self.b2, self.e, self.max_grad_norm, hb.ptr(ws), ws.numel(),
                                              hb.stream_ptr()), "bertadam_step (adapter arena)")
        st.merge(self.arena)
        self.arena.refresh_transposed()

    def _lora_state(self):
        st = self._sync_lora()
        if st is None:
            return {}
        return dict(lora={n: dict(next_m=st.view(st.m, n).detach().cpu().clone(), next_v=st.view(st.v, n).detach().cpu().clone())
                          for n, _, _ in st.slots})

    def _load_lora_state(self, sd):
        st = self._sync_lora()
        has = sd.get("lora") is not None
        if has != (st is not None):
            raise ValueError("optimizer state %s adapter moments cannot be loaded into an optimizer of a model %s LoRA"
                             % ("with" if has else "without", "without" if has else "with"))
        if has:
            for n, _, shape in st.slots:
                m = sd["lora"].get(n)
                if m is None or tuple(m["next_m"].shape) != tuple(shape):
                    raise ValueError("optimizer state: adapter moments of %s are missing or of another shape (--lora_* must match "
                                     "the run that wrote it)" % n)
                st.view(st.m, n).copy_(m["next_m"])
                st.view(st.v, n).copy_(m["next_v"])

    def _build_descs(self, select):
        return self.arena.build_descs(self.lr, self.bert_lr, select=select, active=self._active())

    def _active(self):
        """``active(name)`` of the descriptors: the tensors whose ``requires_grad`` is set (the pooler never; None: all others)"""
        t = self._trainable
        return None if t is None else (lambda n: n in t)

    def sync_frozen(self):
        """rebuild the descriptors (and the sharding plan, which balances by active elements) when the model's frozen set has
        changed since they were built.  Called by every step; the trainer calls it before the forward, so that a sharded plan
        and the gradient exchange of that step agree.  A tensor frozen since construction has zero moments when it becomes
        trainable (nothing updates them meanwhile), as a torch optimizer creates its state on the first gradient it sees."""
        if not hasattr(self.model, "_params"):
            return False
        plan = freeze_plan(self.model)
        if plan.key == self._frozen_key:
            return False
        self._frozen_key, self._trainable = plan.key, plan.trainable
        for part, sel in enumerate(self._selects):
            descs, n_t, n_b = self._build_descs(sel)
            assert (n_t, n_b) == self.parts[part][1:3]
            self.parts[part] = (descs, n_t, n_b, self.parts[part][3])
        if self.sharded:
            # the cut points move (the plan balances by active elements): a range's new owner must start from the current master
            # and moments, which only its old owner holds - make them current everywhere first (a collective: every rank reaches
            # this at the same step, the frozen set being the same on every rank)
            self.gather_master()
            old = self.owner_ranges
            self._plan_shards()
            old[:] = self.owner_ranges          # the list trainer.GradReducer holds
            self.owner_ranges = old
        return True

    def get_lr_mult(self):
        return warmup_linear(self.step_count, self.t_total, self.warmup)

    def zero_grad(self):
        self.arena.g.zero_()

    def _launch(self, part):
        a = self.arena
        descs, n_t, n_b, ws = self.parts[part]
        if n_t == 0:
            return
        if self.sharded:
            return self._launch_sharded(part)
        hb.check(hb.lib().nbest_bertadam_step(hb.ptr(a.p), hb.ptr(a.g), hb.ptr(a.m), hb.ptr(a.v), hb.ptr(a.w16),
                                              hb.ptr(descs), n_t, n_b, self.get_lr_mult(),
                                              self.b1, self.b2, self.e, self.max_grad_norm, hb.ptr(ws),
                                              ws.numel(), hb.stream_ptr()), "bertadam_step")

    def _launch_sharded(self, part):
        a = self.arena
        descs, n_t, n_b, _ = self.parts[part]
        lo, hi = self.blk_bounds[part][self.rank]
        partial, coef = self.partials[part], self.coefs[part]
        partial.zero_()
        hb.check(hb.lib().nbest_bertadam_norms(hb.ptr(a.g), hb.ptr(descs), n_t, n_b, lo, hi, hb.ptr(partial), hb.stream_ptr()), "bertadam_norms")
        dist.all_reduce(partial, op=dist.ReduceOp.SUM)          # every block has ONE owner: the sum only fills in the other ranks' blocks
        hb.check(hb.lib().nbest_bertadam_update(hb.ptr(a.p), hb.ptr(a.g), hb.ptr(a.m), hb.ptr(a.v), hb.ptr(a.w16), hb.ptr(descs), n_t, n_b,
                                                lo, hi, hb.ptr(partial), hb.ptr(coef), self.get_lr_mult(), self.b1, self.b2, self.e,
                                                self.max_grad_norm, hb.stream_ptr()), "bertadam_update")
        self._broadcast_owned(part)

    def _broadcast_owned(self, part):
        """sharded mode: the owners hand out what the next step reads"""
        a = self.arena
        for r, (elo, ehi) in enumerate(self.elem_ranges[part]):
            if ehi <= elo:
                continue
            if a.w16 is None:                                   # fp32 compute: the kernels read the master arena itself
                dist.broadcast(a.p[elo:ehi], src=r)
                continue
            dist.broadcast(a.w16[elo:ehi], src=r)
            idx = self.small_idx[part][r]
            if idx.numel():
                buf = a.p.index_select(0, idx) if r == self.rank else torch.empty(idx.numel(), dtype=torch.float32, device=a.device)
                dist.broadcast(buf, src=r)
                if r != self.rank:
                    a.p.index_copy_(0, idx, buf)

    def gather_master(self, moments=True):
        """sharded mode: make the fp32 master (and the moments) current on every rank - before a checkpoint, a state_dict,
        or a switch back to replicated updates"""
        if not self.sharded:
            return
        a = self.arena
        for part in range(len(self.parts)):
            for r, (elo, ehi) in enumerate(self.elem_ranges[part]):
                if ehi > elo:
                    dist.broadcast(a.p[elo:ehi], src=r)
                    if moments:
                        dist.broadcast(a.m[elo:ehi], src=r)
                        dist.broadcast(a.v[elo:ehi], src=r)

    def step_main(self):
        """every tensor except the embedding tables (+ the k-contiguous weight copy the next forward / dgrad reads)"""
        self._refuse_step_in_ema()
        if self.sam_pending:            # back to w before anything steps (before the descriptors can change); the refresh below covers it
            self._sam_restore_launch()
        self.sync_frozen()
        st = self._sync_lora()
        if st is not None:
            return self._step_lora(st)
        self._launch(0)
        self._ema_update(0)
        self.arena.refresh_transposed()

    def step_embeddings(self):
        self._refuse_step_in_ema()
        self._launch(1)
        self._ema_update(1)
        self.step_count += 1

    def step(self):
        self.step_main()
        self.step_embeddings()

    def state_dict(self, gather=True):
        """per-parameter ``next_m`` / ``next_v`` keyed by parameter name plus the shared step count — the content of
        the reference optimizer's ``state[p]`` (optimization.py:256-262,300), independent of the arena layout.
        Sharded mode: ``gather_master`` is a COLLECTIVE - either every rank calls ``state_dict()``, or every rank calls
        ``gather_master()`` and the one rank that writes the checkpoint calls ``state_dict(gather=False)``."""
        if gather:
            self.gather_master()
        a = self.arena
        return dict(step=self.step_count, t_total=self.t_total, warmup=self.warmup,
                    state={s.name: dict(next_m=a.view(a.m, s.name).detach().cpu().clone(),
                                        next_v=a.view(a.v, s.name).detach().cpu().clone()) for s in a.slots}, **self._ema_state(),
                    **self._lora_state())

    def load_state_dict(self, sd):
        if sd.get("kind", "bertadam") != "bertadam":
            raise ValueError("optimizer state of kind %r cannot be loaded into BertAdam (--optim_choice must match the run that "
                             "wrote it)" % sd["kind"])
        self._load_ema_state(sd, "BertAdam")
        self._load_lora_state(sd)
        a = self.arena
        self.step_count = int(sd["step"])
        for s in a.slots:
            st = sd["state"][s.name]
            a.view(a.m, s.name).copy_(st["next_m"])
            a.view(a.v, s.name).copy_(st["next_v"])


def linear_schedule_with_warmup(k, warmup_steps, t_total):
    """learning-rate multiplier after k scheduler steps: transformers.get_linear_schedule_with_warmup's lambda
    (the reference's n_best_asr_bert.py:564-568)"""
    if k < warmup_steps:
        return float(k) / float(max(1, warmup_steps))
    return max(0.0, float(t_total - k) / float(max(1, t_total - warmup_steps)))


class LinearScheduleWithWarmup:
    """``opt.scheduler`` of --optim_choice adamw: a position k (``last_epoch``, as torch's LambdaLR) that ``step()`` advances and
    the optimizer reads as its learning-rate multiplier.  It is not advanced by the optimizer step itself, so the reference's
    loop body ``optimizer.step(); scheduler.step()`` runs verbatim (trainer.train_epoch calls ``step()`` the same way)."""

    def __init__(self, warmup_steps, t_total):
        self.warmup_steps, self.t_total, self.last_epoch = int(warmup_steps), int(t_total), 0

    def get_lr_mult(self):
        return linear_schedule_with_warmup(self.last_epoch, self.warmup_steps, self.t_total)

    def step(self):
        self.last_epoch += 1


class HipAdam(HipBertAdam):
    """--optim_choice adam | adamw (the reference's n_best_asr_bert.py:266-277,551-569) over the arena, through nbest_adam_*:

      * both: ONE gradient-norm clip over every trainable tensor (clip_grad_norm_(params, max_grad_norm); skipped when
        max_grad_norm <= 0, e.g. when the caller clips itself); the pooler never has a gradient and is left out, as torch
        skips ``p.grad is None``;
      * ``adam``: torch.optim.Adam(params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=l2) - ONE group: lr for every tensor
        (bert_lr is ignored, as there), coupled L2 decay on every tensor, bias correction, no schedule (``scheduler`` is None);
      * ``adamw``: HF AdamW(groups, lr, correct_bias=False) - BertAdam's groups (bert_lr for the encoder, decay 0.01 except
        bias / LayerNorm), eps 1e-6, decoupled decay on the updated parameters, no bias correction - with
        ``scheduler`` = get_linear_schedule_with_warmup(W = int(warmup * t_total), t_total).

    Because the clip is global, nothing may be updated before the LAST gradients (the embedding tables') are in: under data
    parallelism ``step_main`` only computes the block norms of the encoder / head tensors, ``step_embeddings`` adds the
    embedding tables' norms, the coefficient and every update.  Sharded mode: each rank writes its own blocks' norms into a
    zeroed vector that is SUM-all-reduced (x + 0 is exact: every rank computes the replicated coefficient); update, broadcasts
    and ``gather_master`` are BertAdam's."""

    KINDS = {"adam": hb.ADAM_L2, "adamw": hb.ADAMW}

    def __init__(self, model, kind="adamw", lr=5e-4, bert_lr=None, l2=0.0, warmup=0.0, t_total=-1, max_grad_norm=5.0, shard=False,
                 b1=0.9, b2=0.999, ema_decay=None):
        if kind not in self.KINDS:
            raise ValueError("HipAdam: kind must be 'adam' or 'adamw', not %r" % (kind,))
        self.kind, self.mode, self.l2 = kind, self.KINDS[kind], float(l2)
        if kind == "adam":
            bert_lr = lr
        super().__init__(model, lr, bert_lr=bert_lr, warmup=warmup, t_total=t_total, b1=b1, b2=b2,
                         e=1e-8 if kind == "adam" else 1e-6, max_grad_norm=max_grad_norm, shard=shard, ema_decay=ema_decay)
        self.scheduler = None
        if kind == "adamw":
            self.scheduler = LinearScheduleWithWarmup(int(self.warmup * t_total), t_total)
        # the block sums of squares of both descriptor tables back to back: ONE vector, ONE coefficient
        self.blk_base = [0, self.parts[0][2]]
        self.partial = torch.zeros(max(self.parts[0][2] + self.parts[1][2], 1), dtype=torch.float32, device=self.arena.device)
        self.clip = torch.ones(2, dtype=torch.float32, device=self.arena.device)       # [c, total norm]

    def _build_descs(self, select):
        if self.kind == "adam":
            return self.arena.build_descs(self.lr, self.lr, select=select, wd=self.l2, active=self._active())
        return self.arena.build_descs(self.lr, self.bert_lr, select=select, active=self._active())

    def get_lr_mult(self):
        return 1.0 if self.scheduler is None else self.scheduler.get_lr_mult()

    def _range(self, part):
        return self.blk_bounds[part][self.rank] if self.sharded else (0, self.parts[part][2])

    def _norms(self, part):
        a = self.arena
        descs, n_t, n_b, _ = self.parts[part]
        if n_t == 0 or self.max_grad_norm <= 0:
            return
        lo, hi = self._range(part)
        hb.check(hb.lib().nbest_bertadam_norms(hb.ptr(a.g), hb.ptr(descs), n_t, n_b, lo, hi, hb.ptr(self.partial[self.blk_base[part]:]),
                                               hb.stream_ptr()), "bertadam_norms")

    def step_main(self):
        """the block norms of every tensor but the embedding tables: nothing is updated before their gradients are in"""
        self._refuse_step_in_ema()
        if getattr(self.model, "lora", None) is not None:
            self._refuse_with_lora(self.sharded, self.ema_decay)
        if self.sam_pending:            # back to w before anything steps; step_embeddings' refresh covers it
            self._sam_restore_launch()
        self.sync_frozen()
        if self.sharded and self.max_grad_norm > 0:
            self.partial.zero_()
        self._norms(0)

    def step_embeddings(self):
        self._refuse_step_in_ema()
        a = self.arena
        self._norms(1)
        if self.max_grad_norm > 0:
            if self.sharded:
                dist.all_reduce(self.partial, op=dist.ReduceOp.SUM)
            hb.check(hb.lib().nbest_adam_clip_coef(hb.ptr(self.partial), self.partial.numel(), self.max_grad_norm, hb.ptr(self.clip),
                                                   hb.stream_ptr()), "adam_clip_coef")
        else:
            self.clip.fill_(1.0)
        t = self.step_count + 1
        bc1, bc2s = (1.0 - self.b1 ** t, (1.0 - self.b2 ** t) ** 0.5) if self.kind == "adam" else (1.0, 1.0)
        lr_mult = self.get_lr_mult()
        for part in range(len(self.parts)):
            descs, n_t, n_b, _ = self.parts[part]
            if n_t == 0:
                continue
            lo, hi = self._range(part)
            hb.check(hb.lib().nbest_adam_update(self.mode, hb.ptr(a.p), hb.ptr(a.g), hb.ptr(a.m), hb.ptr(a.v), hb.ptr(a.w16), hb.ptr(descs),
                                                n_t, n_b, lo, hi, hb.ptr(self.clip), lr_mult, bc1, bc2s, self.b1, self.b2, self.e,
                                                hb.stream_ptr()), "adam_update")
            self._ema_update(part)
        if self.sharded:
            for part in range(len(self.parts)):
                self._broadcast_owned(part)
        a.refresh_transposed()
        self.step_count += 1

    def state_dict(self, gather=True):
        """torch's per-parameter ``exp_avg`` / ``exp_avg_sq`` keyed by parameter name, the step count and the scheduler position
        (collective in sharded mode: see HipBertAdam.state_dict)"""
        if gather:
            self.gather_master()
        a = self.arena
        return dict(kind=self.kind, step=self.step_count, sched_step=None if self.scheduler is None else self.scheduler.last_epoch,
                    t_total=self.t_total, warmup=self.warmup,
                    state={s.name: dict(exp_avg=a.view(a.m, s.name).detach().cpu().clone(),
                                        exp_avg_sq=a.view(a.v, s.name).detach().cpu().clone()) for s in a.slots}, **self._ema_state())

    def load_state_dict(self, sd):
        kind = sd.get("kind", "bertadam")
        if kind != self.kind:
            raise ValueError("optimizer state of kind %r cannot be loaded into HipAdam(kind=%r) (--optim_choice must match the run "
                             "that wrote it)" % (kind, self.kind))
        self._load_ema_state(sd, "HipAdam(kind=%r)" % self.kind)
        a = self.arena
        self.step_count = int(sd["step"])
        if self.scheduler is not None:
            self.scheduler.last_epoch = int(sd["sched_step"])
        for s in a.slots:
            st = sd["state"][s.name]
            a.view(a.m, s.name).copy_(st["exp_avg"])
            a.view(a.v, s.name).copy_(st["exp_avg_sq"])
