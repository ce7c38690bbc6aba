"""Training / evaluation loops of the fine-tuning path, data-parallel over RCCL.

Host-side mirror of /root/reference/n_best_asr_bert.py:
  train_epoch (:232-294), eval_epoch (:297-388), pred_one_sample (:198-215),
  read_wcn_data / collate_fn labels (/root/reference/utils/dataset/tod_asr_util.py:43-71,114-123).

Data parallelism (new functionality; the reference is single-process): one process per GPU, every rank
holds the full arenas, the minibatch is sharded across ranks.  The reference's BCE / NLL terms are SUM
reductions (n_best_asr_bert.py:572-574), so gradients are all-reduced with SUM (not mean) and the MSE
term (a mean over B_global x H) is pre-scaled by B_local / B_global on each rank (shards may differ by one utterance).  The backward runs in layer chunks; as soon as a
chunk's gradients are complete their slice of the flat gradient arena is all-reduced asynchronously
(RCCL on its own stream over xGMI; 6 chunks of 2 layers for bert-base) while the remaining backward - ending with the embedding backward -
keeps the compute stream busy.  Per-tensor clipping + BertAdam run after the last reduce.
"""
import hashlib
import json
import os
import re
import time

import numpy as np
import torch
import torch.distributed as dist

from . import hipabi as hb
from .fscore import compute_f1, update_f1
from .inputs import collate, encode_utterance, prepare_inputs_for_roberta, utterance_segments
from .model import freeze_plan


# ------------------------------------------------------------------------------------------------
# distributed helpers
# ------------------------------------------------------------------------------------------------
def dist_info():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def init_distributed(backend=None):
    """read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torchrun); no-op for a single process"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "RANK" not in os.environ:          # plain `python bench.py`: single process, no process group
        return 0, 1, 0
    # under torchrun a process group is created even for one rank, so the RCCL path (communicator, async
    # bucketed all-reduce, barrier) is the same code at every N and can be exercised on a 1-GPU box
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend is None and os.environ.get("NBEST_DP_REHEARSAL") == "1":
        # one-GPU rehearsal of the multi-rank code path (tests): every rank on cuda:0, gloo as the transport
        backend, local = "gloo", 0
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    return rank, world, local


def broadcast_parameters(model):
    """identical replicas: rank 0's master arena wins"""
    if dist.is_available() and dist.is_initialized():
        dist.broadcast(model.arena.p, src=0)
        model.arena.refresh_compute_copy()


def shard_bounds(n, rank, world):
    """contiguous shard of n samples for this rank (sizes differ by at most one)"""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def _all_gather_flat(out, inp):
    """async all-gather of equal-sized tensors into one flat buffer (RCCL: the fused collective; gloo - CPU tests and the
    one-GPU rehearsal - gathers into views of it)"""
    if dist.get_backend() == "nccl":
        return dist.all_gather_into_tensor(out, inp, async_op=True)
    n = inp.shape[0]
    return dist.all_gather([out[r * n:(r + 1) * n] for r in range(dist.get_world_size())], inp, async_op=True)


class GradReducer:
    """bucketed asynchronous SUM all-reduce of slices of the flat gradient arena.

    Word-embedding table: with a 250 002-row vocabulary (XLM-R: 768 MB of fp32 gradient, 1 GB for the large model) only the
    <= B_local * (S + S_t) rows of tokens in the rank's shard are non-zero, and the table is the LAST bucket (the embedding
    backward is the last kernel), so nothing hides it.  ``sparse_word_grad`` (default: tables over 256 MB, i.e. XLM-R but not
    BERT's 94 MB) exchanges ``(row ids, row values)`` instead: every rank all-gathers its touched rows (32 x 128 tokens:
    <= 12.6 MB per rank instead of 768 MB through the all-reduce) and rebuilds the summed table locally - own rows zeroed,
    then every rank's rows added in rank order, so all replicas perform the same additions in the same order and stay
    bit-identical.  Position / token-type tables and the embedding LayerNorm stay in a (small) dense bucket."""

    def __init__(self, arena, n_chunks=6, sparse_word_grad=None, owner_ranges=None):
        """``owner_ranges`` (optim.HipBertAdam(shard=True).owner_ranges): per rank, the arena ranges it owns under the sharded
        optimizer - every bucket then travels as a REDUCE of its intersection with each owner's range to that owner (half the bytes
        of the all-reduce; the non-owners never read those gradients) instead of a SUM all-reduce."""
        self.arena = arena
        self.owner_ranges = owner_ranges
        self.rank, self.world = dist_info()
        L = len(arena.layer_range)
        n_chunks = max(1, min(n_chunks, L))
        edges = [round(i * L / n_chunks) for i in range(n_chunks + 1)]
        self.chunks = [(edges[i], edges[i + 1]) for i in range(n_chunks) if edges[i + 1] > edges[i]]
        self.pending = []
        self.pending_emb = []
        ws = arena.by_name["bert_encoder.embeddings.word_embeddings.weight"]
        self.word = (ws.offset, ws.offset + ws.numel, ws.shape)
        self.sparse = (ws.numel * 4 > (256 << 20)) if sparse_word_grad is None else bool(sparse_word_grad)
        self._tok = None          # (unique row ids of this rank's shard, async count exchange) of the running step
        self._sparse = None
        self._side = None         # side stream + pinned buffer that bring the per-rank row counts to the host
        self._cnt_host = None
        self.trainable = None     # arena ranges of the trainable tensors (set_trainable); None = every tensor
        self.word_frozen = False
        self._trainable_names = None

    def set_trainable(self, names):
        """only the gradients of the tensors ``names`` (model.FreezePlan.trainable) are exchanged from the next step on: frozen
        ranges are never launched, a frozen word table skips the sparse row exchange and its count all-gather.  Every rank must
        pass the same set.  With every tensor but the pooler trainable the buckets are the full ones.  Cached per set (one pass
        over the slots when it changes)."""
        if names is self._trainable_names:
            return
        self._trainable_names = names
        ranges, cur, all_on = [], None, True
        for s in sorted(self.arena.slots, key=lambda s: s.offset):
            if s.name not in names:
                all_on = all_on and "pooler" in s.name
                cur = None                               # a frozen tensor (or the pooler) ends the running range
            elif cur is not None:
                cur[1] = s.offset + s.numel              # nothing frozen in between: one range
            else:
                cur = [s.offset, s.offset + s.numel]
                ranges.append(cur)
        if all_on:
            self.trainable, self.word_frozen = None, False
            return
        self.trainable = [tuple(r) for r in ranges]
        self.word_frozen = "bert_encoder.embeddings.word_embeddings.weight" not in names

    # ---- sparse word-embedding rows ------------------------------------------------------------------------------------
    def set_step_tokens(self, *id_tensors, rows=None):
        """call BEFORE the step's forward: ``rows`` = sorted unique token ids of this rank's shard (a device tensor whose
        size the host already knows - EncodedSplit / bench.py build it on the host, so nothing synchronises), or the
        token-id tensors themselves (then the unique rows are computed on the device, which costs one host
        synchronisation at the start of the step).  The per-rank row counts are exchanged asynchronously right away."""
        if not (self.sparse and self.world > 1) or self.word_frozen:
            return
        dev = self.arena.device
        if rows is None:
            toks = [t.reshape(-1) for t in id_tensors if t is not None and t.numel()]
            rows = torch.unique(torch.cat(toks)) if toks else torch.empty(0, dtype=torch.long, device=dev)
        n = torch.tensor([rows.numel()], dtype=torch.long, device=dev)
        counts = torch.zeros(self.world, dtype=torch.long, device=dev)
        work = _all_gather_flat(counts, n)
        # The host needs the counts (they size the row exchange) - but must not wait for the COMPUTE stream to get them: that
        # would drain the whole backward before the row all-gathers, the optimizer and the next step are enqueued (round 2 did a
        # counts.tolist() there).  So the counts go to pinned host memory on a side stream, behind the collective only, with an
        # event; by the time the embedding backward has been enqueued that event completed long ago.
        ev = None
        if dev.type == "cuda":
            if self._side is None:
                self._side = torch.cuda.Stream(device=dev)
                self._cnt_host = torch.empty(self.world, dtype=torch.long).pin_memory()
            with torch.cuda.stream(self._side):
                work.wait()                                   # orders the side stream behind the collective, not the host
                self._cnt_host.copy_(counts, non_blocking=True)
                counts.record_stream(self._side)
                ev = torch.cuda.Event()
                ev.record(self._side)
        self._tok = (rows, counts, work, ev)

    def _start_sparse(self):
        rows, counts, work, ev = self._tok
        if ev is not None:
            ev.synchronize()                                  # the side-stream copy only; the compute stream keeps running
            cnt = self._cnt_host.tolist()
        else:                                                 # CPU tensors (gloo tests): the collective completes on the host
            work.wait()
            cnt = counts.tolist()
        cap = max(max(cnt), 1)
        lo, hi, shape = self.word
        G = self.arena.g[lo:hi].view(shape)
        dev = G.device
        if dev.type == "cuda":                                # library kernels (nbest_rows_gather): ids / values with padding in one launch
            ids, vals = hb.rows_gather(G, rows, cap)
        else:                                                 # gloo rehearsal on CPU tensors (tests/test_dp_gloo.py)
            ids = torch.full((cap,), -1, dtype=torch.long, device=dev)
            vals = torch.zeros(cap, shape[1], dtype=G.dtype, device=dev)
            if rows.numel():
                ids[:rows.numel()] = rows
                vals[:rows.numel()] = G.index_select(0, rows)
        all_ids = torch.empty(self.world * cap, dtype=torch.long, device=dev)
        all_vals = torch.empty(self.world * cap, shape[1], dtype=G.dtype, device=dev)
        w1 = _all_gather_flat(all_ids, ids)
        w2 = _all_gather_flat(all_vals, vals)
        self._sparse = (w1, w2, rows, cnt, cap, all_ids, all_vals, G)
        self._tok = None

    def _finish_sparse(self):
        w1, w2, rows, cnt, cap, all_ids, all_vals, G = self._sparse
        w1.wait()
        w2.wait()
        on_gpu = G.device.type == "cuda"
        if rows.numel():
            hb.rows_zero(G, rows) if on_gpu else G.index_fill_(0, rows, 0.0)
        for r in range(self.world):                                     # the same additions in the same order on every rank
            if cnt[r]:
                i, v = all_ids[r * cap:r * cap + cnt[r]], all_vals[r * cap:r * cap + cnt[r]]
                hb.rows_add(G, i, v) if on_gpu else G.index_add_(0, i, v)      # ids unique within a rank's block: plain += , no atomics
        self._sparse = None

    # ---- dense buckets -------------------------------------------------------------------------------------------------
    def _launch(self, lo, hi, last=False):
        if not (dist.is_available() and dist.is_initialized() and hi > lo):
            return
        if self.trainable is not None:                          # the trainable pieces of the bucket only
            for tlo, thi in self.trainable:
                if min(hi, thi) > max(lo, tlo):
                    self._launch_range(max(lo, tlo), min(hi, thi), last)
            return
        self._launch_range(lo, hi, last)

    def _launch_range(self, lo, hi, last):
        todo = self.pending_emb if last else self.pending
        if self.owner_ranges is None:
            todo.append(dist.all_reduce(self.arena.g[lo:hi], op=dist.ReduceOp.SUM, async_op=True))
            return
        for r, ranges in enumerate(self.owner_ranges):          # the same sequence of collectives on every rank
            for olo, ohi in ranges:
                a, b = max(lo, olo), min(hi, ohi)
                if b > a:
                    todo.append(dist.reduce(self.arena.g[a:b], dst=r, op=dist.ReduceOp.SUM, async_op=True))

    def layers_ready(self, l_lo, l_hi):
        if not self.pending and not self.pending_emb:
            self._launch(*self.arena.heads_range)    # head gradients were complete before the encoder backward began
        self._launch(self.arena.layer_range[l_lo][0], self.arena.layer_range[l_hi - 1][1])
        if l_lo == 0:                                # embedding backward is the last kernel of the chunk
            if self.sparse and self.world > 1 and not self.word_frozen:
                if self._tok is None:
                    raise RuntimeError("GradReducer: sparse word-embedding exchange needs set_step_tokens() before the step")
                self._launch(self.word[1], self.arena.emb_range[1], last=True)
                self._start_sparse()
            else:
                self._launch(*self.arena.emb_range, last=True)

    def wait_layers(self):
        """heads + encoder layers exchanged (the embedding tables may still be in flight)"""
        for w in self.pending:
            w.wait()
        self.pending = []

    def wait(self):
        self.wait_layers()
        for w in self.pending_emb:
            w.wait()
        self.pending_emb = []
        if self._sparse is not None:
            self._finish_sparse()

    def reduce_all(self):
        """exchange the whole gradient arena as it stands, in the bucket order of an overlapped step (used where no backward
        pass is running to overlap with: gradient-accumulation groups, ranks with an empty slice)"""
        for lo, hi in reversed(self.chunks):
            self.layers_ready(lo, hi)
        self.wait()

    def contribute_nothing(self):
        """a rank whose slice of a (short, final) batch is empty still joins every collective of the step, in the same
        order as the ranks that ran a backward pass, with zero gradients"""
        self.arena.g.zero_()
        self.set_step_tokens()
        self.reduce_all()


def sync_frozen(model, optimizer, reducer=None):
    """the model's frozen set (requires_grad) into the optimizer's descriptors and the reducer's ranges, before the step's
    exchange: a sharded plan and its reduce-to-owner then agree"""
    if hasattr(optimizer, "sync_frozen"):
        optimizer.sync_frozen()
    if reducer is not None:
        reducer.set_trainable(freeze_plan(model).trainable)


_LAYER_KEY = re.compile(r"^(bert_encoder\.encoder\.layer\.)(\d+)(\..+)$")


def student_state_from_teacher(sd, layers):
    """A shallower student's initial state dict from a teacher's (reference keys): student layer k = teacher layer ``layers[k]``;
    every other tensor (embeddings, pooler, STC heads) is copied as it is.  Pure: ``sd`` is not modified, the tensors are shared.
    ValueError for an empty list or an index outside the teacher's depth (the caller checks the list against the student's depth)."""
    layers = [int(i) for i in layers]
    by_layer, out = {}, {}
    for k, v in sd.items():
        m = _LAYER_KEY.match(k)
        if m:
            by_layer.setdefault(int(m.group(2)), []).append((m.group(1), m.group(3), v))
        else:
            out[k] = v
    depth = max(by_layer) + 1 if by_layer else 0
    if not layers:
        raise ValueError("student_state_from_teacher: no layers given")
    for i in layers:
        if not 0 <= i < depth:
            raise ValueError("student_state_from_teacher: teacher layer %d does not exist (the teacher has %d layers)" % (i, depth))
    for k, i in enumerate(layers):
        for pre, post, v in by_layer[i]:
            out["%s%d%s" % (pre, k, post)] = v
    return out


def teacher_scores(teacher, ids, seg, alpha, temperature=None):
    """forward_backward's ``distill`` argument from ``teacher.predict`` on the batch: enqueued on the current stream ahead of the
    student's step, no host synchronisation; the teacher is put into eval mode and nothing of it is stepped.  With a
    ``temperature`` the teacher's logits (``predict(return_logits=True)``) in the logits form dict(logits, alpha, temperature);
    without one its probabilities dict(top, bott, final, alpha)"""
    if teacher.training:
        teacher.eval()
    with torch.no_grad():
        t = teacher.predict(ids, seg_ids=seg, return_logits=temperature is not None)
    if temperature is not None:
        return dict(logits=t["logits"], alpha=float(alpha), temperature=float(temperature))
    return dict(top=t["top"], bott=t["bott"], final=t["final"], alpha=float(alpha))


def hard_loss_parts(out):
    """the loss_parts a step without a teacher would have returned: under distillation slot 3 carries the soft loss, the record
    of the [Train] line keeps the hard terms (+ the MSE of --add_l2_loss)"""
    lp = out["loss_parts"].clone()
    if out.get("mse") is not None:
        lp[3:4].copy_(out["mse"])
    else:
        lp[3:4].zero_()
    return lp


def rdrop_batch(batch):
    """the batch of an R-Drop step: every tensor of ``batch`` (ids, seg, labels, tids, tseg) repeated along dimension 0, so that rows
    b and b + P hold the same utterance (forward_backward's ``rdrop`` pairs them; the dropout hashes are keyed on the position in the
    batch, so the two copies run under independent masks).  ``tok_perm`` / ``ttok_perm`` are rebuilt for the doubled ids - token
    indices sorted stably by word id, ties in ascending token index, nbest_embed_ln_bwd's contract - by hipabi.word_perm on the
    tensors' device (a sort on the current stream, no host synchronisation).  Everything else (``word_rows``) passes through."""
    out = dict(batch)
    for k in ("ids", "seg", "labels", "tids", "tseg", "tkey"):
        if batch.get(k) is not None:
            out[k] = torch.cat([batch[k], batch[k]], dim=0)
    for k, src in (("tok_perm", "ids"), ("ttok_perm", "tids")):
        if batch.get(src) is not None:
            out[k] = hb.word_perm(out[src])
    return out


def rdrop_hard_loss_parts(out):
    """the record of an R-Drop step for the [Train] line: half the hard parts of its 2 P rows (+ the MSE of --add_l2_loss, a mean
    already), so that Loss compares with a run without the flag; slot 3's consistency term is left out, as the soft loss is"""
    lp = hard_loss_parts(out)
    lp[:3].mul_(0.5)
    return lp


def soft_term_args(teacher, distill_alpha, distill_temperature, rdrop_alpha, batch, world, add_segment_ids=True):
    """(batch, distill, rdrop) of one forward_backward call: under ``rdrop_alpha`` the doubled batch and dict(alpha); with a
    ``teacher`` its scores of the batch (teacher_scores).  One soft term per step, and neither is built under data parallelism."""
    distill = rdrop = None
    if rdrop_alpha is not None:
        if teacher is not None:
            raise ValueError("nbest_amd: rdrop_alpha together with a teacher is not built (one soft term per step)")
        if world > 1:
            raise RuntimeError("nbest_amd: rdrop under data parallelism is not built (world size %d)" % world)
        batch, rdrop = rdrop_batch(batch), dict(alpha=float(rdrop_alpha))
    if teacher is not None:
        if world > 1:
            raise RuntimeError("nbest_amd: distillation under data parallelism is not built (world size %d)" % world)
        seg = batch.get("seg") if add_segment_ids else None
        distill = teacher_scores(teacher, batch["ids"], seg, distill_alpha, distill_temperature)
    return batch, distill, rdrop


def adv_args(adv_epsilon, teacher, rdrop_alpha, world):
    """forward_backward's ``adv`` of one call under ``adv_epsilon`` (None: none).  FGM carries no soft term and is not built under
    data parallelism."""
    if adv_epsilon is None:
        return None
    if teacher is not None or rdrop_alpha is not None:
        raise ValueError("nbest_amd: adv_epsilon together with a teacher or rdrop_alpha is not built (the adversarial pass has the "
                         "hard terms only)")
    if world > 1:
        raise RuntimeError("nbest_amd: adv_epsilon under data parallelism is not built (world size %d)" % world)
    return dict(epsilon=float(adv_epsilon))


def sam_args(sam_rho, sam_adaptive, sam_eta, model, optimizer, adv_epsilon, world, n_accum=1):
    """optimizer.sam_perturb's arguments of one step under ``sam_rho`` (None: none): dict(rho, adaptive, eta).  Every combination
    that is not built is refused here, before anything is enqueued: FGM (two two-pass schemes in one step), LoRA, the fp8w mode
    (its amax histories would record twice per step and the e4m3 images would be cut from perturbed weights), a trainable head
    mask, the sharded optimizer, data parallelism and gradient accumulation (the perturbation is formed from ONE batch's
    gradient)."""
    if sam_rho is None:
        return None
    rho, eta = float(sam_rho), float(sam_eta)
    if not (rho >= 0.0 and rho != float("inf")):
        raise ValueError("nbest_amd: sam_rho must be finite and >= 0, not %r" % (sam_rho,))
    if sam_adaptive and not (eta > 0.0 and eta != float("inf")):
        raise ValueError("nbest_amd: sam_eta must be finite and > 0, not %r" % (sam_eta,))
    if adv_epsilon is not None:
        raise ValueError("nbest_amd: sam_rho together with adv_epsilon is not built (two two-pass schemes in one step)")
    if getattr(model, "lora", None) is not None:
        raise RuntimeError("nbest_amd: sam_rho on a model with LoRA enabled is not built (the perturbation would have to follow the "
                           "factors, not the merged weights)")
    if getattr(model, "fp8_forward", False):
        raise RuntimeError("nbest_amd: sam_rho on an fp8w model is not built (the amax histories would record twice per step and "
                           "the e4m3 images would be cut from perturbed weights)")
    if getattr(model, "head_mask_trainable", False):
        raise RuntimeError("nbest_amd: sam_rho under a trainable head mask is not built")
    if getattr(optimizer, "sharded", False):
        raise RuntimeError("nbest_amd: sam_rho with the sharded optimizer is not built (the fp32 master is current only on each "
                           "range's owner)")
    if world > 1:
        raise RuntimeError("nbest_amd: sam_rho under data parallelism is not built (world size %d)" % world)
    if n_accum > 1:
        raise RuntimeError("nbest_amd: sam_rho under gradient accumulation is not built (n_accum_steps %d: the perturbation is "
                           "formed from one batch's gradient)" % n_accum)
    return dict(rho=rho, adaptive=bool(sam_adaptive), eta=eta)


def transcript_keys(tids):
    """int64 [B]: for every row of the transcript ids ``tids`` [B, S] the index of the FIRST row of the batch whose ids are
    identical - the key under which the contrastive term (forward_backward's ``contrast``) leaves utterances with the same
    transcript out of each other's denominators.  An exact comparison of the rows, not a hash; on the tensor's device (CPU or
    GPU), no host synchronisation."""
    B = tids.shape[0]
    same = (tids.unsqueeze(1) == tids.unsqueeze(0)).all(dim=-1)                    # [B, B]
    idx = torch.arange(B, dtype=torch.int64, device=tids.device)
    return torch.where(same, idx.unsqueeze(0), torch.full_like(idx, B).unsqueeze(0)).min(dim=1).values


def contrast_args(contrast_weight, contrast_temperature, batch, adv_epsilon, world, check_only=False):
    """forward_backward's ``contrast`` of one call under ``contrast_weight`` (None: none), for the batch the call runs on (under
    R-Drop the doubled one: the twins share a key).  The keys are the batch's ``tkey`` or transcript_keys of its ``tids``.  The
    negatives are the rows of one process's batch: not built under data parallelism, and not with FGM.  ``check_only``: the
    refusals alone, nothing enqueued."""
    if contrast_weight is None:
        return None
    if adv_epsilon is not None:
        raise ValueError("nbest_amd: contrast_weight together with adv_epsilon is not built (the adversarial pass has the hard "
                         "terms only)")
    if world > 1:
        raise RuntimeError("nbest_amd: contrast_weight under data parallelism is not built: the negatives would have to cross "
                           "ranks (world size %d)" % world)
    if batch.get("tids") is None:
        raise ValueError("nbest_amd: contrast_weight needs the transcripts (batch['tids'])")
    if check_only:
        return None
    keys = batch.get("tkey")
    return dict(weight=float(contrast_weight), temperature=float(contrast_temperature),
                keys=keys if keys is not None else transcript_keys(batch["tids"]))


def train_step(model, optimizer, batch, add_l2_loss=False, add_segment_ids=True, reducer=None, global_batch=None, teacher=None,
               distill_alpha=0.5, distill_temperature=None, rdrop_alpha=None, adv_epsilon=None, contrast_weight=None,
               contrast_temperature=0.1, sam_rho=None, sam_adaptive=False, sam_eta=0.01):
    """One optimisation step on this rank's shard.  batch: dict(ids, seg, labels[, tids, tseg]) device tensors.
    ``global_batch`` = utterances of the whole minibatch over all ranks (default: world x this shard).
    ``teacher``: a second NBestSTCModel (knowledge distillation) - its ``predict`` scores of the batch become the soft targets of
    the step (forward_backward's ``distill``), weighted ``distill_alpha``; ``loss_parts[3]`` is then the soft loss.  With a
    ``distill_temperature`` T the teacher's logits are the targets and both models are softened by 1 / T (the logits form).
    ``rdrop_alpha``: R-Drop - the step runs on ``rdrop_batch(batch)`` (every utterance twice, 2 P rows) and adds alpha x the symmetric
    KL between the twins' outputs (forward_backward's ``rdrop``); the returned tensors have 2 P rows, ``loss_parts[3]`` is the
    consistency sum.  Not with a ``teacher``; data parallelism is not built.
    ``adv_epsilon``: FGM adversarial training on the word embeddings (forward_backward's ``adv``): the step runs the ASR pass a
    second time on embeddings moved by epsilon along the normalised gradient and the optimizer steps ONCE on the sum of both passes'
    gradients; the returned scores and ``loss_parts`` are the clean pass's, ``adv_loss_parts`` / ``adv_norm`` come on top.  Not with a
    ``teacher`` or ``rdrop_alpha``; data parallelism is not built.
    ``contrast_weight``: adds W x the in-batch contrastive loss between the ASR and the transcript CLS rows at
    ``contrast_temperature`` (forward_backward's ``contrast``; the keys are the batch's ``tkey`` or transcript_keys of its ``tids``);
    the outputs gain ``contrast``.  Under ``rdrop_alpha`` the term runs on the doubled batch with doubled keys, so the twins drop out
    of each other's denominators.  Works with ``add_l2_loss``, a ``teacher`` and ``rdrop_alpha``; not with ``adv_epsilon``; data
    parallelism is not built (negatives across ranks).
    A model under a trainable head mask (``set_head_mask(mask, trainable=True)``) steps as any other on one GPU; data parallelism is
    not built (refused before anything is enqueued).
    ``sam_rho``: sharpness-aware minimization (Foret et al., 2021; ``sam_adaptive``: ASAM, Kwon et al., 2021, with ``sam_eta``).  The
    step runs forward_backward twice under the SAME dropout bits (``advance=False`` on the first): the first pass's gradient g
    moves the trainable weights to w + e (optimizer.sam_perturb: e = rho g / ||g||, one norm over every trainable tensor), the
    second pass overwrites ``arena.g`` with the gradient there, and ``optimizer.step()`` moves the weights back to w, to the bit,
    and applies that gradient.  The soft-term arguments are computed once (one teacher ``predict``, one doubled batch, one set of
    contrast keys).  The returned dict is the FIRST pass's (scores and ``loss_parts`` at w, so the [Train] record compares with a
    run without the flag; ``asr_cls`` / ``trans_cls`` are views of the stash and show the second pass) plus ``sam_loss_parts``
    (the second pass's ``loss_parts``, at w + e) and ``sam_norm`` (fp32 [1]: ||g||, adaptive: ||T g||).  Works with the three
    optimizers, ``add_l2_loss``, a ``teacher``, ``rdrop_alpha``, ``contrast_weight``, ema_decay and frozen tensors (neither moved
    nor in the norm); sam_args lists what is refused.  About twice the step plus two streaming passes over the arenas.
    Returns the step outputs (device tensors; no host synchronisation)."""
    _, world = dist_info()
    if world > 1 and getattr(model, "head_mask_trainable", False):
        raise RuntimeError("nbest_amd: training under a head mask under data parallelism is not built (world size %d)" % world)
    b_local = batch["ids"].shape[0]
    adv = adv_args(adv_epsilon, teacher, rdrop_alpha, world)
    sam = sam_args(sam_rho, sam_adaptive, sam_eta, model, optimizer, adv_epsilon, world)
    if sam is not None and getattr(optimizer, "sam_pending", False):
        raise RuntimeError("nbest_amd: a SAM perturbation is pending on the optimizer (step or sam_restore() first)")
    if contrast_weight is not None:                              # refused before the teacher runs or the batch is doubled
        contrast_args(contrast_weight, contrast_temperature, batch, adv_epsilon, world, check_only=True)
    batch, distill, rdrop = soft_term_args(teacher, distill_alpha, distill_temperature, rdrop_alpha, batch, world, add_segment_ids)
    contrast = contrast_args(contrast_weight, contrast_temperature, batch, adv_epsilon, world)
    seg = batch.get("seg") if add_segment_ids else None          # n_best_asr_bert.py:252
    # (FGM: the second pass adds to every gradient, so nothing is ready before the call returns - one world-size-1 exchange at the end;
    # SAM: the first pass's gradient is never exchanged, the second pass's is - the same single exchange)
    overlap = reducer is not None and adv is None and sam is None
    chunks = reducer.chunks if overlap else None
    # MSE is a MEAN over B_global x H (n_best_asr_bert.py:574): the local kernel differentiates the mean over its own
    # B_local rows, so after the SUM all-reduce the term needs the weight B_local / B_global (= 1/world for equal shards)
    mse_scale = b_local / float(global_batch) if global_batch else 1.0 / world
    sync_frozen(model, optimizer, reducer)
    if reducer is not None:
        reducer.set_step_tokens(batch["ids"], batch.get("tids") if (add_l2_loss or contrast is not None) else None,
                                rows=batch.get("word_rows"))
    passes = lambda **kw: model.forward_backward(
        batch["ids"], batch["labels"], seg_ids=seg, trans_input_ids=batch.get("tids"), trans_seg_ids=batch.get("tseg"),
        add_l2_loss=add_l2_loss, mse_grad_scale=mse_scale, chunks=chunks, on_chunk_done=reducer.layers_ready if overlap else None,
        tok_perm=batch.get("tok_perm"), trans_tok_perm=batch.get("ttok_perm"), distill=distill, rdrop=rdrop, adv=adv,
        **({} if contrast is None else dict(contrast=contrast)), **kw)
    if sam is None:
        out = passes()
    else:
        out = passes(advance=False)                              # the gradient at w; step_counter stays: the same dropout bits below
        optimizer.sam_perturb(sam["rho"], adaptive=sam["adaptive"], eta=sam["eta"])
        at_e = passes(accumulate=False, advance=True)            # the gradient at w + e replaces it; optimizer.step() restores w
        out["sam_loss_parts"], out["sam_norm"] = at_e["loss_parts"], optimizer.sam_norm.clone()
    if reducer is not None and not overlap:
        reducer.reduce_all()
        optimizer.step()
    elif reducer is not None:
        reducer.wait_layers()
        optimizer.step_main()             # runs while the embedding tables' all-reduce is still in flight
        reducer.wait()
        optimizer.step_embeddings()
    else:
        optimizer.step()
    return out


# ------------------------------------------------------------------------------------------------
# data: "ASR \t<=>\t TRANSCRIPT \t<=>\t label1;label2" lines
# ------------------------------------------------------------------------------------------------
def coverage_sample(labels, coverage, seed=42):
    """Row order of the --coverage stratified subsample, /root/reference/utils/dataset/tod_asr_util.py:12-39:
    the first utterance of every distinct label set (file order), then
    rem = round(|coverage * N - n_unique|) of the remaining utterances drawn without replacement by
    pandas' DataFrame.sample(n=rem, random_state=42) = numpy RandomState(42).choice(len(rest), rem, False)."""
    seen, uniq = set(), []
    for i, l in enumerate(labels):
        t = tuple(l)
        if t not in seen:
            seen.add(t)
            uniq.append(i)
    uset = set(uniq)
    rest = [i for i in range(len(labels)) if i not in uset]
    rem = int(np.round(abs(float(coverage) * len(labels) - len(uniq))))
    pick = np.random.RandomState(seed).choice(len(rest), size=rem, replace=False)
    return uniq + [rest[int(j)] for j in pick]


def read_wcn_data(fn, coverage=None):
    """``ASR \\t<=>\\t TRANSCRIPT \\t<=>\\t label1;label2`` lines (tod_asr_util.py:43-71); coverage: see coverage_sample"""
    asr, trans, labels = [], [], []
    with open(fn) as fp:
        for line in fp:
            a, t, lbl = line.strip("\n\r").split("\t<=>\t")
            asr.append(a.strip().split(" "))
            trans.append(t.strip().split(" "))
            labels.append(lbl.strip().split(";") if lbl else [])
    if coverage:
        order = coverage_sample(labels, coverage)
        asr, trans, labels = [asr[i] for i in order], [trans[i] for i in order], [labels[i] for i in order]
    return asr, trans, labels


def read_predict_data(fn):
    """--predict input: the split format, but only the ASR field is required.  A line holds ``ASR`` alone or
    ``ASR \t<=>\t TRANSCRIPT \t<=>\t labels`` (transcript and labels are read and not used).  Returns (asr, trans, labels)
    like read_wcn_data, one entry per line in file order; a missing transcript is the ASR field, missing labels are []."""
    asr, trans, labels = [], [], []
    with open(fn) as fp:
        for n, line in enumerate(fp, 1):
            f = line.strip("\n\r").split("\t<=>\t")
            if len(f) not in (1, 3):
                raise ValueError("%s:%d: expected 1 or 3 fields separated by '\\t<=>\\t', got %d" % (fn, n, len(f)))
            a = f[0].strip().split(" ")
            asr.append(a)
            trans.append(f[1].strip().split(" ") if len(f) == 3 else list(a))
            labels.append(f[2].strip().split(";") if len(f) == 3 and f[2].strip() else [])
    return asr, trans, labels


def labels_to_multihot(label_lists, label2idx, device, unk=1):
    y = torch.zeros(len(label_lists), len(label2idx))
    for i, ls in enumerate(label_lists):
        for l in ls:
            y[i, label2idx.get(l, unk)] = 1
    return y.to(device)


def batches(data, batch_size, shuffle=False, seed=0):
    asr, trans, labels = data
    order = np.arange(len(asr))
    if shuffle:
        np.random.default_rng(seed).shuffle(order)
    for i in range(0, len(order), batch_size):
        idx = order[i:i + batch_size]
        yield [asr[j] for j in idx], [trans[j] for j in idx], [labels[j] for j in idx]


def pred_labels_from_indices(pred_row, idx2label):
    """pred_one_sample (:198-215) from the device decode: labels in top-label order"""
    return [idx2label[j] for j in pred_row if j >= 0]


def filter_informative(labels, ontology):
    """n_best_asr_bert.py:218-229: keep act-slot-value labels only when the slot is ``this`` or an informable slot
    with more than one value; labels of any other arity pass through"""
    keep = []
    for lbl in labels:
        tup = lbl.split("-")
        if len(tup) != 3 or tup[1] == "this" or (tup[1] in ontology["informable"] and len(ontology["informable"][tup[1]]) > 1):
            keep.append(lbl)
    return keep


def _count_metrics(pred, raw_labels, idx2label, counts, ontology=None):
    """pred_one_sample + update_f1 + exact-match bookkeeping (n_best_asr_bert.py:198-215,283-288) from decoded index rows"""
    TP, FP, FN, corr, tot = counts
    all_preds = []
    for row, gold in zip(pred, raw_labels):
        pc = pred_labels_from_indices(row, idx2label)
        if ontology is not None:                                          # eval only (:341-344)
            pc, gold = filter_informative(pc, ontology), filter_informative(gold, ontology)
        TP, FP, FN = update_f1(pc, gold, TP, FP, FN)
        tot += 1
        corr += int(set(pc) == set(gold))
        all_preds.append(pc)
    return (TP, FP, FN, corr, tot), all_preds


def _host_metrics(model, out, raw_labels, idx2label, counts, ontology=None):
    """synchronous form (drains the compute stream): kept for callers outside the epoch loops"""
    return _count_metrics(model.decode(out["top"], out["bott"]).cpu().tolist(), raw_labels, idx2label, counts, ontology)


class MetricsPipe:
    """The per-sample decode of the reference (n_best_asr_bert.py:283-288) WITHOUT a host synchronisation per step.  Round 3 did
    ``model.decode(...).cpu().tolist()`` after every step, which drains the compute stream - the GPU then idles while Python
    prepares the next step.  Here the decode kernel of step i writes its int32 [B, 30] rows STRAIGHT into one of two pinned host
    buffers (mapped host memory: no copy command), a one-thread kernel behind it stamps the step number into a pinned word
    (nbest_stream_stamp), and the host turns the rows into labels / F1 counts one step LATER, after polling that word - while
    step i + 1 runs.  No hipMemcpy, no event, no stream synchronisation.  (tools/real_variants.py times this form against a
    non_blocking D2H copy + event wait: once the host thread pool is capped - limit_host_threads, the actual cause of the 37 ms
    steps first measured - both keep the GPU busy, 20.4 vs 20.5 ms per step; this one issues no runtime call besides the two
    launches.)  ``finish()`` drains the last one.  Same counts, same order."""

    def __init__(self, model, idx2label, ontology=None):
        self.model, self.idx2label, self.ontology = model, idx2label, ontology
        self.counts, self.preds = (0, 0, 0, 0, 0), []
        self.cuda = model.device.type == "cuda"
        self.bufs, self.turn, self.seq = [None, None], 0, 0
        self.flags = torch.zeros(2, dtype=torch.int32).pin_memory() if self.cuda else None
        self.pending = None

    def _host_rows(self, B, n_top):
        """one of two alternating pinned buffers, grown when a larger batch comes (never reallocated per step)"""
        t = self.turn = self.turn ^ 1
        if self.bufs[t] is None or self.bufs[t].shape[0] < B or self.bufs[t].shape[1] != n_top:
            self.bufs[t] = torch.empty(B, n_top, dtype=torch.int32).pin_memory()
        return t, self.bufs[t]

    def push(self, out, raw_labels, tag=None):
        if not self.cuda:
            self._consume((self.model.decode(out["top"], out["bott"]), None, raw_labels, tag))
            return
        # (buffer t held step i-2, whose rows were counted at the previous push)
        t, rows = self._host_rows(out["top"].shape[0], out["top"].shape[1])
        pred = self.model.decode(out["top"], out["bott"], out=rows)
        self.seq += 1
        hb.stream_stamp(self.flags[t:t + 1], self.seq)
        prev, self.pending = self.pending, (pred, (t, self.seq), raw_labels, tag)
        if prev is not None:
            self._consume(prev)

    def _consume(self, item):
        host, stamp, raw_labels, tag = item
        if stamp is not None:
            t, seq = stamp
            flag, t0 = self.flags.numpy(), time.time()
            while flag[t] != seq:              # step i-1's rows: the compute stream already holds step i
                time.sleep(0.0002)
                if time.time() - t0 > 600.0:
                    raise RuntimeError("nbest_amd: the decode of a step did not arrive within 10 minutes")
        self.counts, preds = _count_metrics(host.tolist(), raw_labels, self.idx2label, self.counts, self.ontology)
        self.preds.append((tag, preds))

    def finish(self):
        if self.pending is not None:
            self._consume(self.pending)
            self.pending = None
        return self.counts, self.preds


class EncodedSplit:
    """A data split tokenised ONCE.

    The reference re-tokenises every word of every batch of every epoch in a Python loop
    (bert_xlnet_inputs.py:46-53); at the step rates of the HIP path that loop is the bottleneck of real-data runs.
    Here every utterance is converted to id / segment lists when the split is first used; a batch is then only a
    gather + right-pad into pinned host buffers (inputs.collate).  Unpacks like the raw ``(asr, trans, labels)`` tuple.
    """

    def __init__(self, data, opt, memory):
        self.asr, self.trans, self.labels = data
        tok = opt.tokenizer
        nb, msl = getattr(opt, "n_best", None), getattr(opt, "max_seq_len", None)
        as_np = lambda r: (np.asarray(r[0], dtype=np.int64), None if r[1] is None else np.asarray(r[1], dtype=np.int64))
        self.rows = [as_np(encode_utterance(s, tok, opt, nb, msl)) for s in self.asr]
        self.trows = [as_np(encode_utterance(s, tok, opt, None, msl)) for s in self.trans]
        l2i = memory["label2idx"]
        self.y = torch.zeros(len(self.labels), len(l2i))
        for i, ls in enumerate(self.labels):
            for l in ls:
                self.y[i, l2i.get(l, 1)] = 1                      # unknown label -> index 1, as labels_to_multihot
        self.pad = tok.pad_token_id

    def __iter__(self):
        return iter((self.asr, self.trans, self.labels))

    def __len__(self):
        return len(self.asr)

    def host_batch(self, idx, pin=False, stage=None):
        """``stage``: a PinnedStage whose buffers receive every tensor of the batch (no allocation per batch)"""
        take = (lambda name: (lambda which, shape: stage.take(name + str(which), shape, torch.int64))) if stage is not None else (lambda name: None)
        ids, seg, _ = collate([self.rows[j] for j in idx], self.pad, pin and stage is None, alloc=take("a"))
        tids, tseg, _ = collate([self.trows[j] for j in idx], self.pad, pin and stage is None, alloc=take("t"))
        # rows of the word-embedding table this batch touches (sparse gradient exchange under data parallelism)
        rows = np.unique(np.concatenate([ids.numpy().ravel(), tids.numpy().ravel()]))
        # tokens sorted by word id, ties in token order: what the deterministic embedding backward reduces over (nbest_embed_ln_bwd)
        perm, tperm = token_perm(ids, as_numpy=True), token_perm(tids, as_numpy=True)
        if stage is None:
            p_ = (lambda t: t.pin_memory()) if pin else (lambda t: t)
            y = p_(self.y[torch.as_tensor(idx, dtype=torch.long)])
            rows, perm, tperm = p_(torch.from_numpy(rows)), p_(torch.from_numpy(perm)), p_(torch.from_numpy(tperm))
        else:
            y = stage.take("y", (len(idx), self.y.shape[1]), self.y.dtype)
            np.take(self.y.numpy(), np.asarray(idx, dtype=np.int64), axis=0, out=y.numpy())   # (numpy: no torch CPU thread pool in the worker)
            rows, perm, tperm = stage.put("rows", rows, torch.int64), stage.put("perm", perm, torch.int32), stage.put("tperm", tperm, torch.int32)
        return dict(ids=ids, seg=seg, tids=tids, tseg=tseg, labels=y, word_rows=rows, tok_perm=perm, ttok_perm=tperm)


_ITEMSIZE = {torch.int64: 8, torch.int32: 4, torch.float32: 4, torch.uint8: 1}


def host_cpu_budget():
    """CPUs this process may really use: the smaller of its affinity mask and its cgroup quota (cpu.max / cfs_quota_us)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        if os.path.exists("/sys/fs/cgroup/cpu.max"):
            quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(quota) // int(period)))
        elif os.path.exists("/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0:
                n = min(n, max(1, quota // period))
    except (OSError, ValueError):
        pass
    return n


def limit_host_threads():
    """torch sizes its CPU thread pool by the MACHINE's cores (128 on the GPU box) while the container's quota is 16: every small
    CPU op of the loop (an index_select of the label rows: 5.6 ms instead of 0.05) wakes 128 spinning threads, the cgroup is
    throttled and the whole process - the thread that launches kernels included - is frozen for the rest of the scheduling
    period.  Measured on the box (tools/host_batch_time.py): a prefetched batch cost 6.8 ms of host time at 128 threads, 0.9 ms
    at one; inside the training loop 23-47 ms, more than a step.  The HIP path needs no CPU parallelism: cap the pool at the
    smaller of 4 and the quota.  Called by the epoch loops' Prefetcher (both of its threads), cli.py and bench.py."""
    want = max(1, min(4, host_cpu_budget()))
    if torch.get_num_threads() > want:
        torch.set_num_threads(want)


class PinnedStage:
    """Long-lived pinned host buffers for ONE batch in flight, by name, grown geometrically when a larger batch comes.
    ``take(name, shape, dtype)`` -> a tensor view to fill; ``put(name, array, dtype)`` copies a numpy array in."""

    def __init__(self, pin=True):
        self.pin, self.buf = pin, {}

    def take(self, name, shape, dtype):
        n = int(np.prod(shape)) * _ITEMSIZE[dtype]
        t = self.buf.get(name)
        if t is None or t.numel() < n:
            t = torch.empty(max(n, 2 * (0 if t is None else t.numel()), 4096), dtype=torch.uint8)
            t = self.buf[name] = t.pin_memory() if self.pin else t
        return t[:n].view(dtype).view(*shape)

    def put(self, name, array, dtype):
        t = self.take(name, array.shape, dtype)
        t.numpy()[...] = array
        return t


def token_perm(ids, as_numpy=False):
    """host: int32 [B*S] token indices sorted by word id, ties in ascending token index (numpy's stable argsort)"""
    p = np.argsort(ids.reshape(-1).numpy(), kind="stable").astype(np.int32)
    return p if as_numpy else torch.from_numpy(p)


def encoded(data, opt, memory):
    return data if isinstance(data, EncodedSplit) else EncodedSplit(data, opt, memory)


def batch_indices(n, batch_size, shuffle=False, seed=0):
    order = np.arange(n)
    if shuffle:
        np.random.default_rng(seed).shuffle(order)
    return [order[i:i + batch_size].tolist() for i in range(0, n, batch_size)]


class Prefetcher:
    """Iterates ``(batch_index, dataset indices of this rank's slice, device batch)`` one batch ahead of the consumer.

    A worker thread collates batch i+1 into pinned host memory and enqueues its H2D copies on a side stream while the
    GPU runs step i; the consumer's stream waits on the copy event only (no host synchronisation)."""

    def __init__(self, split, index_lists, device, rank=0, world=1, depth=2):
        import queue
        import threading
        self.split, self.lists, self.device, self.rank, self.world = split, index_lists, torch.device(device), rank, world
        self.cuda = self.device.type == "cuda"
        self.q = queue.Queue(maxsize=depth)
        self.stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.seconds = [0.0, 0.0, 0.0]
        limit_host_threads()
        # pinned staging: one PinnedStage per batch that can be alive at once (depth in the queue + the one the consumer holds + the one
        # being built + one spare), reused round-robin once the H2D copies that read it have completed
        self.stages = [(PinnedStage(), [None]) for _ in range(depth + 3)] if self.cuda else None
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def _work(self):
        try:
            limit_host_threads()                                     # (OpenMP's thread count is a per-thread setting)
            for bi, idx in enumerate(self.lists):
                lo, hi = shard_bounds(len(idx), self.rank, self.world)
                if hi <= lo:
                    self.q.put((bi, [], None, None))                 # nothing for this rank in this batch
                    continue
                mine = idx[lo:hi]
                t0 = time.time()
                if not self.cuda:
                    self.q.put((bi, mine, self.split.host_batch(mine), None))
                    continue
                stage, last = self.stages[bi % len(self.stages)]
                if last[0] is not None:
                    last[0].synchronize()                             # the copies out of this stage, depth + 3 batches ago
                host = self.split.host_batch(mine, stage=stage)
                t1 = time.time()
                with torch.cuda.stream(self.stream):
                    dev = {k: (None if v is None else v.to(self.device, non_blocking=True)) for k, v in host.items()}
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                last[0] = ev
                t2 = time.time()
                self.q.put((bi, mine, dev, (ev, host)))
                self.seconds[0] += t1 - t0                           # (worker-side clock: collate | H2D enqueue | queue full)
                self.seconds[1] += t2 - t1
                self.seconds[2] += time.time() - t2
            self.q.put(None)
        except BaseException as e:                                   # surface worker failures in the consumer
            self.q.put(e)

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            bi, mine, dev, sync = item
            if sync is not None:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(sync[0])
                for v in dev.values():
                    if v is not None:
                        v.record_stream(cur)
            yield bi, mine, dev


def _prep(raw_in, raw_trans, raw_labels, opt, memory, device):
    ids, seg, _ = prepare_inputs_for_roberta(raw_in, opt.tokenizer, opt, device, n_best=getattr(opt, "n_best", None),
                                             max_seq_len=getattr(opt, "max_seq_len", None))
    tids, tseg, _ = prepare_inputs_for_roberta(raw_trans, opt.tokenizer, opt, device, max_seq_len=getattr(opt, "max_seq_len", None))
    y = labels_to_multihot(raw_labels, memory["label2idx"], device)
    return dict(ids=ids, seg=seg, tids=tids, tseg=tseg, labels=y)


def train_epoch(model, data, opt, memory, epoch=0, shuffle=True):
    """n_best_asr_bert.py:232-294 -> (mean_loss, (p, r, f), acc).  ``data`` = (asr, trans, labels) lists or an
    EncodedSplit (tokenised once; pass the same object every epoch to reuse it).

    ``opt.n_accum_steps`` > 1 (n_best_asr_bert.py:522,526,266-280): the loader batch is batchSize / n_accum_steps, gradients
    of n_accum_steps consecutive micro-batches are summed and the optimizer steps after every n_accum_steps-th one; micro-
    batches left over at the end of the epoch are dropped by the next epoch's zero_grad, as there.  Under data parallelism
    only the micro-batch that closes a group exchanges gradients."""
    model.train()
    rank, world = dist_info()
    reducer = (GradReducer(model.arena, owner_ranges=getattr(opt.optimizer, "owner_ranges", None))
               if (dist.is_available() and dist.is_initialized()) else None)
    losses = []
    pipe = MetricsPipe(model, memory["idx2label"])
    split = encoded(data, opt, memory)
    n_accum = max(1, int(getattr(opt, "n_accum_steps", 1) or 1))
    lists = batch_indices(len(split), max(1, int(opt.batchSize / n_accum)), shuffle=shuffle, seed=getattr(opt, "random_seed", 999) + epoch)
    group_rows = []                                                  # word-table rows touched by the running accumulation group
    # --optim_choice adamw: the loop advances the learning-rate schedule after every optimizer step, as the reference's does
    # (n_best_asr_bert.py:273-275); BertAdam and Adam have none
    sched = getattr(opt.optimizer, "scheduler", None)
    teacher, alpha = getattr(opt, "teacher", None), getattr(opt, "distill_alpha", 0.5)      # --distill_from
    temperature = getattr(opt, "distill_temperature", None)                                 # --distill_temperature
    rdrop_alpha = getattr(opt, "rdrop_alpha", None)                                         # --rdrop_alpha
    adv_epsilon = getattr(opt, "adv_epsilon", None)                                         # --adv_epsilon
    contrast_weight = getattr(opt, "contrastive_weight", None)                              # --contrastive_weight
    contrast_temperature = getattr(opt, "contrastive_temperature", None) or 0.1
    contrast_sum = None                                              # fp32 [4] on the device: the epoch's sum of out["contrast"]
    sam = dict(sam_rho=getattr(opt, "sam_rho", None), sam_adaptive=bool(getattr(opt, "sam_adaptive", False)),   # --sam_rho
               sam_eta=getattr(opt, "sam_eta", None) or 0.01)
    sam_args(sam["sam_rho"], sam["sam_adaptive"], sam["sam_eta"], model, opt.optimizer, adv_epsilon, world, n_accum)
    sam_sum, sam_utts = None, 0                                      # fp32 [2] on the device: sum of (hard loss at w + e - at w), of sam_norm
    for bi, mine, b in Prefetcher(split, lists, model.device, rank, world):
        first, last = (bi % n_accum == 0), ((bi + 1) % n_accum == 0)
        if first:
            group_rows = []
        if not mine:
            if first:
                model.arena.g.zero_()
            if last:
                sync_frozen(model, opt.optimizer, reducer)
                if reducer is not None:
                    reducer.set_step_tokens(*group_rows)
                    reducer.reduce_all()
                opt.optimizer.step()                                 # keeps replicas and schedule positions identical
                if sched is not None:
                    sched.step()
            model.step_counter += 1
            continue
        if n_accum == 1:
            out = train_step(model, opt.optimizer, b, add_l2_loss=opt.add_l2_loss, add_segment_ids=opt.add_segment_ids, reducer=reducer,
                             global_batch=len(lists[bi]), teacher=teacher, distill_alpha=alpha,
                             distill_temperature=temperature, rdrop_alpha=rdrop_alpha, adv_epsilon=adv_epsilon,
                             **({} if sam["sam_rho"] is None else sam),
                             **({} if contrast_weight is None else dict(contrast_weight=contrast_weight,
                                                                        contrast_temperature=contrast_temperature)))
            if sched is not None:
                sched.step()
        else:
            adv = adv_args(adv_epsilon, teacher, rdrop_alpha, world)
            b, distill, rdrop = soft_term_args(teacher, alpha, temperature, rdrop_alpha, b, world, opt.add_segment_ids)
            contrast = contrast_args(contrast_weight, contrast_temperature, b, adv_epsilon, world)   # negatives: the micro-batch's
            seg = b.get("seg") if opt.add_segment_ids else None
            out = model.forward_backward(b["ids"], b["labels"], seg_ids=seg, trans_input_ids=b.get("tids"), trans_seg_ids=b.get("tseg"),
                                         add_l2_loss=opt.add_l2_loss, mse_grad_scale=len(mine) / float(len(lists[bi])),
                                         accumulate=not first, tok_perm=b.get("tok_perm"), trans_tok_perm=b.get("ttok_perm"),
                                         distill=distill, rdrop=rdrop, adv=adv, **({} if contrast is None else dict(contrast=contrast)))
            group_rows.append(b["word_rows"])
            if last:
                sync_frozen(model, opt.optimizer, reducer)
                if reducer is not None:
                    reducer.set_step_tokens(*group_rows)
                    reducer.reduce_all()
                opt.optimizer.step()
                if sched is not None:
                    sched.step()
        if contrast_weight is not None:
            contrast_sum = out["contrast"].clone() if contrast_sum is None else contrast_sum.add_(out["contrast"])
        if sam["sam_rho"] is not None:
            step = torch.cat([(out["sam_loss_parts"][:3].sum() - out["loss_parts"][:3].sum()).reshape(1), out["sam_norm"]])
            if rdrop_alpha is not None:
                step[:1].mul_(0.5)                                   # 2 P rows: per utterance, as the [Train] record
            sam_sum, sam_utts = (step if sam_sum is None else sam_sum.add_(step)), sam_utts + len(mine)
        if rdrop_alpha is not None:
            # the record: half the hard parts of the 2 P rows; the metrics: the first copy of every utterance
            losses.append((rdrop_hard_loss_parts(out), len(mine), len(lists[bi])))
            out = dict(top=out["top"][:len(mine)], bott=out["bott"][:len(mine)])
        else:
            losses.append((out["loss_parts"] if teacher is None else hard_loss_parts(out), len(mine), len(lists[bi])))
        pipe.push(out, [split.labels[j] for j in mine])
    counts, _ = pipe.finish()
    if contrast_weight is not None:                                  # read by the CLI after the [Train] line: (sum L, hits, rows, 0)
        opt.contrast_epoch = None if contrast_sum is None else contrast_sum.double().cpu().tolist()
    if sam["sam_rho"] is not None:                  # read by the CLI after the [Train] line: (sum of differences, sum of norms, utterances, steps)
        opt.sam_epoch = None if sam_sum is None else sam_sum.double().cpu().tolist() + [sam_utts, len(lists)]
    return _finish(losses, counts, model.device, len(lists))


def merge_cases(chunks):
    """[(batch_index, rank, cases)] of this rank -> all ranks' cases in dataset order (batch, then rank slice)"""
    _, world = dist_info()
    if world > 1:
        every = [None] * world
        dist.all_gather_object(every, chunks)
        chunks = sorted((c for part in every for c in part), key=lambda c: (c[0], c[1]))
    return [case for _, _, part in chunks for case in part]


@torch.no_grad()
def eval_epoch(model, data, opt, memory, fp=None, efp=None):
    """n_best_asr_bert.py:297-388 -> (mean_loss, (p, r, f), acc, cases); writes ``raw <=> pred <=> gold`` lines.

    Under data parallelism every rank evaluates its slice of each batch; the per-utterance cases are gathered and put
    back into dataset order, so ``cases`` and the lines written are the same on every rank as in a single process.
    """
    model.eval()
    rank, world = dist_info()
    onto = getattr(opt, "ontology", None)
    losses, chunks = [], []
    pipe = MetricsPipe(model, memory["idx2label"], onto)
    split = encoded(data, opt, memory)
    # the reference builds its valid / test loaders with int(batchSize / n_accum_steps) too (n_best_asr_bert.py:529-531), and the
    # record is the mean over batches of sum / batch size: the partition (and the weight of a short last batch) must be the same
    n_accum = max(1, int(getattr(opt, "n_accum_steps", 1) or 1))
    lists = batch_indices(len(split), max(1, int(opt.batchSize / n_accum)))
    for bi, mine, b in Prefetcher(split, lists, model.device, rank, world):
        if not mine:
            continue
        seg = b["seg"] if opt.add_segment_ids else None
        out = model.forward_backward(b["ids"], b["labels"], seg_ids=seg, need_grad=False)     # no MSE in eval (:331)
        losses.append((out["loss_parts"], len(mine), len(lists[bi])))
        pipe.push(out, [split.labels[j] for j in mine], tag=(bi, mine))
    counts, tagged = pipe.finish()
    for (bi, mine), preds in tagged:
        raw_labels = [split.labels[j] for j in mine]
        golds = [filter_informative(g, onto) if onto is not None else g for g in raw_labels]
        chunks.append((bi, rank, list(zip([split.asr[j] for j in mine], preds, golds))))
    cases = merge_cases(chunks)
    for raw, pc, gold in cases:
        line = "%s\t<=>\t%s\t<=>\t%s\n" % (" ".join(raw), ";".join(pc), ";".join(gold))
        if fp is not None:
            fp.write(line)
        if efp is not None and set(pc) != set(gold):
            efp.write(line)
    return _finish(losses, counts, model.device, len(lists)) + (cases,)


def attention_record(line, spans, cls_attn):
    """one --predict_attention JSON record.  ``cls_attn``: fp32 [L, heads, >= tokens], the CLS row's attention probabilities of
    one utterance (model.predict(return_attns=True)["cls_attn"][:, b]); ``spans``: inputs.utterance_segments of it.  ``mass``
    [L][segments] = per layer, the mean over heads of the probability that falls on each span, normalised over the utterance's
    own tokens (under XLM-R the reference's ids > 0 mask, quirk Q1, leaves padding keys unmasked: their share is left out)."""
    a = cls_attn.detach().double().cpu().mean(dim=1)
    m = torch.stack([a[:, lo:hi].sum(dim=1) for _, lo, hi in spans], dim=1)
    m = m / m.sum(dim=1, keepdim=True).clamp_min(1e-300)
    return {"line": line, "segments": [n for n, _, _ in spans], "tokens": [hi - lo for _, lo, hi in spans],
            "mass": [[round(x, 6) for x in row] for row in m.tolist()]}


def rollout_reference(attns, residual):
    """The arithmetic of ``model.attention_rollout`` restated with plain matrix products (Abnar & Zuidema, 2020).  ``attns``: the
    tuple of L attention maps [B, heads, S, S] (``forward(return_attns=True)``).  With A~_l = residual I + (1 - residual) mean_h A_l,
    returns fp64 [L, B, S]: row l is the CLS row (row 0) of A~_{L-1} ... A~_l - so row 0 is the rollout and row L-1 the last
    layer's head-mean CLS attention mixed with the residual."""
    rho = float(residual)
    L = len(attns)
    B, _, S, _ = attns[0].shape
    r = torch.zeros(B, 1, S, dtype=torch.float64, device=attns[0].device)
    r[:, 0, 0] = 1.0
    eye = torch.eye(S, dtype=torch.float64, device=attns[0].device)
    out = [None] * L
    for l in range(L - 1, -1, -1):
        r = r @ (rho * eye + (1.0 - rho) * attns[l].double().mean(dim=1))
        out[l] = r[:, 0]
    return torch.stack(out)


def rollout_record(line, spans, row, residual):
    """one --predict_rollout JSON record.  ``row``: fp32 [>= tokens], the CLS rollout of one utterance
    (model.attention_rollout(...)["rollout"][b]); ``spans``: inputs.utterance_segments of it.  ``token_rollout`` is the row
    normalised over the utterance's own tokens (as attention_record: under XLM-R the padding keys stay unmasked, quirk Q1, and
    their share is left out), ``mass`` its per-span sums."""
    ntok = spans[-1][2] if spans else 0
    t = row.detach().double().cpu()[:ntok]
    t = (t / sum(t[lo:hi].sum() for _, lo, hi in spans).clamp_min(1e-300)).tolist() if spans else []
    return {"line": line, "segments": [n for n, _, _ in spans], "tokens": [hi - lo for _, lo, hi in spans], "residual": float(residual),
            "mass": [round(sum(t[lo:hi]), 6) for _, lo, hi in spans], "token_rollout": [round(x, 6) for x in t]}


def token_keep_schedule(L, first, last):
    """A --token_keep schedule for an L-layer encoder: L - 1 non-increasing ints running geometrically from ``first`` (the tokens
    that leave layer 0) to ``last`` (those that reach the last layer), entry i = round(first (last / first)^(i / (L - 2))).
    L = 1 gives [], L = 2 gives [last] (the one boundary there is leads to the last layer).  ValueError unless
    L >= 1 and first >= last >= 1."""
    L, first, last = int(L), int(first), int(last)
    if L < 1:
        raise ValueError("token_keep_schedule: L must be >= 1 (got %d)" % L)
    if not first >= last >= 1:
        raise ValueError("token_keep_schedule: needs first >= last >= 1 (got %d, %d)" % (first, last))
    n = L - 1
    if n <= 1:
        return [last] * n
    out = [int(round(first * (last / float(first)) ** (i / float(n - 1)))) for i in range(n)]
    out[0], out[-1] = first, last
    for i in range(1, n):                                     # (rounding cannot raise a geometric sequence, but say so in code)
        out[i] = max(last, min(out[i], out[i - 1]))
    return out


def parse_token_keep(spec, L):
    """--token_keep SPEC -> the schedule for an L-layer encoder: ``a,b,c`` (L - 1 counts) or ``first:last``
    (token_keep_schedule).  ``L`` None: check the syntax and what can be checked without the encoder's depth, return None.
    ValueError names what is wrong."""
    try:
        if ":" in spec:
            parts = [int(x) for x in spec.split(":")]
            if len(parts) != 2:
                raise ValueError
            keep = token_keep_schedule(1 if L is None else L, parts[0], parts[1])   # (L None: its checks of first and last)
            return None if L is None else keep
        keep = [int(x) for x in spec.split(",")] if spec.strip() else []
    except ValueError as e:
        if str(e).startswith("token_keep_schedule"):
            raise
        raise ValueError("expected L - 1 comma-separated integers or FIRST:LAST")
    if any(x < 1 for x in keep):
        raise ValueError("every count must be >= 1")
    if any(y > x for x, y in zip(keep, keep[1:])):
        raise ValueError("the counts must not increase")
    if L is not None and len(keep) != L - 1:
        raise ValueError("%d counts for an encoder of %d layers (L - 1 = %d are needed)" % (len(keep), L, L - 1))
    return None if L is None else keep


def token_select_reference(score, mask, k):
    """The selection of nbest_token_select restated with numpy.  ``score`` [B, S] (any float dtype; taken as fp64), ``mask`` [B, S]
    (non-zero = a real token), 1 <= k <= S -> int64 [B, k]: position 0, then the k - 1 first of the other positions in the order
    unmasked before masked, number before NaN, higher score first, lower index first - returned ascending."""
    sc = np.asarray(score.detach().cpu().numpy() if torch.is_tensor(score) else score, dtype=np.float64)
    mk = np.asarray(mask.detach().cpu().numpy() if torch.is_tensor(mask) else mask) != 0
    B, S = sc.shape
    if not 1 <= k <= S:
        raise ValueError("token_select_reference: k=%d outside 1..S=%d" % (k, S))
    out = np.zeros((B, k), dtype=np.int64)
    for b in range(B):
        nan = np.isnan(sc[b, 1:])
        val = np.where(nan, 0.0, sc[b, 1:]) + 0.0
        # lexsort: the LAST key is the primary one; it is stable, so equal keys stay in index order
        order = np.lexsort((np.arange(S - 1), -val, nan, ~mk[b, 1:]))
        out[b] = np.sort(np.concatenate(([0], 1 + order[:k - 1])))
    return out


def token_prune_reference(attn, mask, k):
    """Score and selection of one eliminating layer of ``model.predict(token_keep=...)`` restated in fp64 (PoWER-BERT's
    significance score).  ``attn``: the layer's attention map [B, heads, S, S] (``forward(return_attns=True)[l]``), ``mask``
    [B, S] -> (score fp64 [B, S] = mean over heads of the column sums over the unmasked queries, idx int64 [B, k] =
    token_select_reference of it)."""
    a = np.asarray(attn.detach().double().cpu().numpy() if torch.is_tensor(attn) else attn, dtype=np.float64)
    mk = (np.asarray(mask.detach().cpu().numpy() if torch.is_tensor(mask) else mask) != 0).astype(np.float64)
    score = np.einsum("bi,bhij->bj", mk, a) / a.shape[1]
    return score, token_select_reference(score, mk, k)


def token_prune_record(line, spans, kept):
    """one --predict_tokens JSON record.  ``kept``: int [L - 1, >= tokens] of one utterance (model.predict(...,
    return_token_kept=True)["token_kept"][:, b]): per layer boundary the original positions still there, then -1; ``spans``:
    inputs.utterance_segments of it (as attention_record).  ``kept[l][s]`` = how many tokens of segment s leave layer l
    (kept padding positions belong to no segment)."""
    rows = kept.tolist() if hasattr(kept, "tolist") else kept
    out = []
    for row in rows:
        there = set(int(x) for x in row if x >= 0)
        out.append([sum(1 for p in range(lo, hi) if p in there) for _, lo, hi in spans])
    return {"line": line, "segments": [n for n, _, _ in spans], "tokens": [hi - lo for _, lo, hi in spans], "kept": out}


def attribution_record(line, spans, attr_row, labels, scores, baselines, steps):
    """one --predict_attribution JSON record.  ``attr_row``: per label, fp32 [>= tokens] integrated-gradients attribution of one
    utterance (model.attribute); ``spans``: inputs.utterance_segments of it (as attention_record); ``labels`` / ``scores`` /
    ``baselines``: the label strings in the .pred line's order and F at alpha = 1 / alpha = 0.  ``mass`` = per-span sums of
    ``token_attr`` (fp64), so sum(mass) ~ score - baseline_score."""
    ntok = spans[-1][2] if spans else 0
    out = []
    for a, lbl, sc, bs in zip(attr_row, labels, scores, baselines):
        t = [float(x) for x in a.detach().double().cpu()[:ntok].tolist()]
        out.append({"label": lbl, "score": round(float(sc), 6), "baseline_score": round(float(bs), 6),
                    "mass": [round(sum(t[lo:hi]), 6) for _, lo, hi in spans], "token_attr": [round(x, 6) for x in t]})
    return {"line": line, "segments": [n for n, _, _ in spans], "tokens": [hi - lo for _, lo, hi in spans], "steps": int(steps),
            "labels": out}


@torch.no_grad()
def predict_split(model, data, opt, memory, attn_fp=None, attr_fp=None, attr_steps=32, fp8=False, calib_batches=8, rollout_fp=None,
                  rollout_residual=0.5, token_keep=None, tokens_fp=None):
    """Labels of every utterance of a split through ``model.predict`` (forward only, CLS rows of the last layer):
    [(asr words, predicted labels)] in split order.  Same batches, device decode and label strings as eval_epoch (the
    ontology filter too), so the labels equal eval_epoch's pred column for the same model and data.  One GPU only.
    ``attn_fp`` (--predict_attention): a text file that receives one attention_record JSON line per utterance, in split order
    ("line": 1-based index in the split).  ``attr_fp`` (--predict_attribution): one attribution_record JSON line per utterance, in
    split order - integrated gradients (model.attribute, ``attr_steps`` path points) of every label the .pred line lists.
    ``fp8`` (--predict_fp8): ``model.fp8_calibrate`` on the first ``calib_batches`` batches of the split (from scratch), one line on
    stdout about what was recorded, then every batch through ``model.predict(fp8=True)``.
    ``rollout_fp`` (--predict_rollout): one rollout_record JSON line per utterance, in split order - the CLS attention rollout
    (model.attention_rollout with ``rollout_residual``); the labels still come from ``model.predict``.
    ``token_keep`` (--token_keep): every batch through ``model.predict(token_keep=...)``; ``tokens_fp`` (--predict_tokens): one
    token_prune_record JSON line per utterance, in split order.  Not with ``fp8`` or any of the other outputs."""
    _, world = dist_info()
    if world > 1:
        raise RuntimeError("nbest_amd: predicting a file runs on one GPU (world size %d); start it without torchrun" % world)
    onto = getattr(opt, "ontology", None)
    pipe = MetricsPipe(model, memory["idx2label"], onto)
    split = encoded(data, opt, memory)
    n_accum = max(1, int(getattr(opt, "n_accum_steps", 1) or 1))
    lists = batch_indices(len(split), max(1, int(opt.batchSize / n_accum)))
    if token_keep is None and tokens_fp is not None:
        raise RuntimeError("nbest_amd: the token record is an output of token_keep")
    if token_keep is not None and (fp8 or attn_fp is not None or attr_fp is not None or rollout_fp is not None):
        raise RuntimeError("nbest_amd: token_keep together with fp8, attention maps, attributions or the rollout is not built")
    if fp8:
        if attn_fp is not None or attr_fp is not None or rollout_fp is not None:
            raise RuntimeError("nbest_amd: the fp8 inference writes no attention maps, no attributions and no rollout")
        head = lists[:max(1, int(calib_batches))]
        for k, (bi, mine, b) in enumerate(Prefetcher(split, head, model.device)):
            model.fp8_calibrate(b["ids"], seg_ids=b["seg"] if opt.add_segment_ids else None, reset=k == 0)
        cal = model.fp8_calibration().cpu()[:-1]          # layers 0 .. L-2 run all four fp8 GEMMs (the last layer: x only)
        kinds = ["%s %.3g..%.3g" % (nm, cal[:, i].min().item(), cal[:, i].max().item()) for i, nm in enumerate(("x", "ctx", "x1", "gelu"))
                 ] if len(cal) else ["x %.3g" % model.fp8_calibration()[-1, 0].item()]
        print("fp8 calibration: %d batches, %d utterances; amax over the layers: %s"
              % (len(head), sum(len(m) for m in head), ", ".join(kinds)), flush=True)
    for bi, mine, b in Prefetcher(split, lists, model.device):
        seg = b["seg"] if opt.add_segment_ids else None
        if token_keep is None:
            out = model.predict(b["ids"], seg_ids=seg, return_attns=attn_fp is not None, fp8=fp8)
        else:
            out = model.predict(b["ids"], seg_ids=seg, token_keep=token_keep, return_token_kept=tokens_fp is not None)
        pipe.push(out, [split.labels[j] for j in mine], tag=mine)
        spans_of = {}
        for k, j in enumerate(mine if (attn_fp is not None or attr_fp is not None or rollout_fp is not None or tokens_fp is not None) else []):
            spans = utterance_segments(split.asr[j], opt.tokenizer, opt, getattr(opt, "n_best", None), getattr(opt, "max_seq_len", None))
            if spans[-1][2] != len(split.rows[j][0]):
                raise RuntimeError("nbest_amd: line %d: segment spans cover %d tokens, the encoded utterance has %d"
                                   % (j + 1, spans[-1][2], len(split.rows[j][0])))
            spans_of[j] = spans
        if tokens_fp is not None:
            tk = out["token_kept"].cpu()
            for k, j in enumerate(mine):
                tokens_fp.write(json.dumps(token_prune_record(j + 1, spans_of[j], tk[:, k])) + "\n")
        if attn_fp is not None:
            ca = out["cls_attn"].cpu()
            for k, j in enumerate(mine):
                attn_fp.write(json.dumps(attention_record(j + 1, spans_of[j], ca[:, k])) + "\n")
        if rollout_fp is not None:
            ro = model.attention_rollout(b["ids"], seg_ids=seg, residual=rollout_residual)["rollout"].cpu()
            for k, j in enumerate(mine):
                rollout_fp.write(json.dumps(rollout_record(j + 1, spans_of[j], ro[k], rollout_residual)) + "\n")
        if attr_fp is not None:
            # the labels of the .pred line: decoded rows -> label strings (ontology filter as MetricsPipe) -> their bottom ids
            rows = out["pred"].cpu().tolist()
            kept = []
            for k, row in enumerate(rows):
                names = pred_labels_from_indices(row, memory["idx2label"])
                keep = set(filter_informative(names, onto)) if onto is not None else set(names)
                kept.append([(c, memory["idx2label"][c]) for c in row if c >= 0 and memory["idx2label"][c] in keep])
            targets = [(k, c) for k, lst in enumerate(kept) for c, _ in lst]
            res = model.attribute(b["ids"], seg_ids=seg, targets=targets, steps=attr_steps)
            at, sc, bs = res["attr"].cpu(), res["score"].cpu(), res["baseline_score"].cpu()
            i = 0
            for k, j in enumerate(mine):
                n = len(kept[k])
                attr_fp.write(json.dumps(attribution_record(j + 1, spans_of[j], at[i:i + n], [nm for _, nm in kept[k]], sc[i:i + n],
                                                            bs[i:i + n], attr_steps)) + "\n")
                i += n
    _, tagged = pipe.finish()
    return [(split.asr[j], pc) for mine, preds in tagged for j, pc in zip(mine, preds)]


def read_head_mask(path, L, heads):
    """--head_mask FILE: a JSON list of L rows of ``heads`` numbers (0 prunes a head, 1 keeps it, any float gates it) -> the rows
    as floats; ValueError names what is wrong with the file"""
    try:
        with open(path) as fp:
            rows = json.load(fp)
    except (OSError, ValueError) as e:
        raise ValueError("head mask %s: %s" % (path, e))
    num = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)
    if not isinstance(rows, list) or not all(isinstance(r, list) for r in rows):
        raise ValueError("head mask %s: expected a JSON list of %d rows of %d numbers" % (path, L, heads))
    if len(rows) != L or any(len(r) != heads for r in rows):
        raise ValueError("head mask %s: shape [%d][%s] does not match the encoder's [L=%d][heads=%d]"
                         % (path, len(rows), ",".join(sorted({str(len(r)) for r in rows})), L, heads))
    if not all(num(x) and x == x and abs(x) != float("inf") for r in rows for x in r):
        raise ValueError("head mask %s: every entry must be a finite number" % path)
    return [[float(x) for x in r] for r in rows]


def head_mask_digest(rows):
    """the name a mask goes by in an experiment directory (--train_head_mask): the first 8 hex digits of the SHA-1 of its entries as
    little-endian fp32, row-major"""
    return hashlib.sha1(np.asarray(rows, dtype="<f4").tobytes()).hexdigest()[:8]


def head_mask_file_digest(path):
    """head_mask_digest of a mask file, before the encoder's shape is known (the shape is read_head_mask's to check)"""
    try:
        with open(path) as fp:
            return head_mask_digest(json.load(fp))
    except (OSError, ValueError, TypeError) as e:
        raise ValueError("head mask %s: %s" % (path, e))


def head_importance_table(grads):
    """Michel et al. (2019) from per-utterance gate gradients: ``grads`` yields fp32 [L, B_i, heads] tensors (model.head_gate_grad's
    ``grad`` per batch).  importance[l][h] = mean over all utterances of |d L_b / d xi[l, h]| (accumulated in fp64);
    normalized = importance with every layer's row divided by its l2 norm (their per-layer normalisation; a zero row stays zero)."""
    total, n = None, 0
    for g in grads:
        part = g.detach().double().abs().sum(dim=1)
        total = part if total is None else total + part
        n += g.shape[1]
    if total is None or n == 0:
        raise ValueError("head importance: no utterance")
    imp = (total / n).cpu()
    norm = imp / imp.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-300)
    return {"importance": imp.tolist(), "normalized": norm.tolist(), "utterances": n}


def prune_lowest(importance, mask, n):
    """A new mask with the ``n`` lowest-importance heads that ``mask`` still keeps (entry != 0; None = all ones) set to 0: heads in
    ascending importance, ties by (layer, head) index; a head that is the last one kept in its layer is passed over, so every layer
    keeps at least one.  ValueError when fewer than ``n`` heads can go.  Pure: neither argument is modified."""
    imp = [[float(x) for x in row] for row in (importance.tolist() if torch.is_tensor(importance) else importance)]
    new = [[1.0] * len(r) for r in imp] if mask is None else [[float(x) for x in row] for row in (mask.tolist() if torch.is_tensor(mask) else mask)]
    if [len(r) for r in new] != [len(r) for r in imp]:
        raise ValueError("prune_lowest: importance and mask differ in shape")
    if n < 0:
        raise ValueError("prune_lowest: n must be >= 0 (got %d)" % n)
    kept = [sum(1 for x in row if x != 0.0) for row in new]
    order = sorted((imp[l][h], l, h) for l in range(len(new)) for h in range(len(new[l])) if new[l][h] != 0.0)
    left = n
    for _, l, h in order:
        if left == 0:
            break
        if kept[l] > 1:
            new[l][h] = 0.0
            kept[l] -= 1
            left -= 1
    if left:
        raise ValueError("prune_lowest: only %d of %d heads can be pruned with one head kept per layer" % (n - left, n))
    return new


def head_importance(model, data, opt, memory):
    """Head importance of a split (Michel et al., 2019, "Are sixteen heads better than one?"): model.head_gate_grad over eval_epoch's
    batches, at the model's current head mask -> {"importance": [L][heads], "normalized": [L][heads], "utterances": n}
    (head_importance_table).  No dropout, no parameter gradient, no training state touched.  One GPU only."""
    _, world = dist_info()
    if world > 1:
        raise RuntimeError("nbest_amd: head importance runs on one GPU (world size %d); start it without torchrun" % world)
    split = encoded(data, opt, memory)
    n_accum = max(1, int(getattr(opt, "n_accum_steps", 1) or 1))
    lists = batch_indices(len(split), max(1, int(opt.batchSize / n_accum)))

    def grads():
        for _, mine, b in Prefetcher(split, lists, model.device):
            if mine:
                yield model.head_gate_grad(b["ids"], b["labels"], seg_ids=b["seg"] if opt.add_segment_ids else None)["grad"]
    return head_importance_table(grads())


def _finish(losses, counts, device, n_batches=None):
    """losses: [(loss_parts[4] = BCE(final), BCE(top), mean-CE, MSE of this rank's shard, B_local, B_global)] per batch.
    loss_record of a batch = sum(parts) / batch_size (n_best_asr_bert.py:168-192), mean over batches (:290).  The BCE / CE
    parts are sums over utterances, so a rank contributes its sums / B_global; the MSE part is a mean over the rank's own
    rows and enters with the weight B_local / B_global - summed over ranks this is the single-process record even when the
    shards are uneven.  ``n_batches``: batches of the epoch (the same on every rank; a rank whose shard of a batch was
    empty has no entry for it)."""
    rec = 0.0
    for lp, b_local, b_global in losses:
        lp = lp.double().cpu()
        rec += (float(lp[:3].sum()) + float(lp[3]) * b_local / b_global) / b_global
    if n_batches is None:
        n_batches = len(losses)
    stat = torch.tensor(list(counts) + [rec], dtype=torch.float64, device=device)
    _, world = dist_info()
    if world > 1:
        dist.all_reduce(stat, op=dist.ReduceOp.SUM)
    TP, FP, FN, corr, tot, lsum = stat.tolist()
    p, r, f = compute_f1(int(TP), int(FP), int(FN))
    acc = corr / tot * 100 if tot else 0
    return lsum / max(n_batches, 1), (p, r, f), acc
