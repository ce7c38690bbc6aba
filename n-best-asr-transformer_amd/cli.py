"""Command-line front end with the flag surface of the reference's training script.

    python -m nbest_amd.cli --dataset dstc2 --dataroot dstc2_data/processed_data/raw --pre_trained_model bert \\
        --deviceId 0 --random_seed 999 --dropout 0.3 --bert_dropout 0.1 --optim_choice bertadam --lr 3e-5 --bert_lr 3e-5 \\
        --warmup_proportion 0.1 --batchSize 16 --max_epoch 50 --experiment exp/ --coverage 1.0 --add_segment_ids

Flag names, defaults and meaning follow /root/reference/n_best_asr_bert.py:39-112 as driven by
/root/reference/run/train_eval_N_Best_ASR_Transformer_STC.sh:62-75 (live flags: --pre_trained_model,
--add_l2_loss, --add_segment_ids, --coverage, --without_system_act, --dropout, --bert_dropout, --lr, --bert_lr,
--warmup_proportion, --batchSize, --max_epoch, --random_seed, --testing, --experiment, --ontology_path; flags the
reference parses but never uses are accepted and only enter the experiment-directory name, as there).
Differences forced by the environment (no network, no CUDA): the encoder is built from its published shape
(nbest_amd.config.NAMED) and initialised from ``--init_checkpoint`` (a state dict with the reference's keys, e.g. a
converted HuggingFace checkpoint or a model.pt written by either implementation) or randomly; the tokenizer is a
local WordPiece vocabulary (``--vocab``; default: the words of memory.pt).  Additive flags: --dtype, --n_best,
--label_space, --synthetic.  Under torchrun the minibatch is sharded over the ranks (RCCL gradient all-reduce).
"""
import argparse
import contextlib
import json
import math
import os
import random
import sys
import time
from datetime import timedelta

import numpy as np
import torch

from . import config as ncfg, observe, synth, trainer
from .inputs import SentencePieceTokenizer, WordPieceTokenizer
from .model import NBestSTCModel
from .optim import HipAdam, HipBertAdam


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(description="N-best ASR transformer STC fine-tuning on MI355X (HIP)")
    g = ap.add_argument_group("model structure (accepted for compatibility; only used in the experiment directory name)")
    g.add_argument("--emb_size", type=int, default=256)
    g.add_argument("--hidden_size", type=int, default=512)
    g.add_argument("--max_seq_len", type=int, default=None)
    g.add_argument("--n_layers", type=int, default=6)
    g.add_argument("--n_head", type=int, default=4)
    g.add_argument("--d_k", type=int, default=64)
    g.add_argument("--d_v", type=int, default=64)
    g.add_argument("--score_util", default="pp", choices=["none", "np", "pp", "mul"])
    g.add_argument("--sent_repr", default="bin_sa_cls",
                   choices=["cls", "maxpool", "attn", "bin_lstm", "bin_sa", "bin_sa_cls", "tok_sa_cls"])
    g.add_argument("--cls_type", default="stc", choices=["nc", "tf_hd", "stc"])
    g = ap.add_argument_group("data")
    g.add_argument("--dataset", required=True)
    g.add_argument("--dataroot", required=True)
    g.add_argument("--train_file", default="train")
    g.add_argument("--valid_file", default="valid")
    g.add_argument("--test_file", default="test")
    g.add_argument("--ontology_path", default=None, help="ontology JSON: evaluation keeps informative act-slot-value labels only")
    g = ap.add_argument_group("encoder")
    g.add_argument("--bert_model_name", default="bert-base-uncased")
    g.add_argument("--fix_bert_model", action="store_true",
                   help="accepted and ignored, as by the reference (which parses it and never reads it); freeze with "
                        "--freeze_embeddings / --freeze_layers")
    g.add_argument("--freeze_embeddings", action="store_true",
                   help="train with the word, position and token-type tables and the embedding LayerNorm frozen (requires_grad False)")
    g.add_argument("--freeze_layers", type=int, default=0, metavar="K",
                   help="train with encoder layers 0..K-1 frozen (0 <= K <= the number of layers)")
    g.add_argument("--pre_trained_model", help="bert | xlm-roberta (| xlm-roberta-large).  'roberta' is refused: the reference hands "
                   "segment ids to RoBERTa's one-row token-type table and dies with an IndexError (models/model.py:56)")
    g.add_argument("--tod_pre_trained_model", help="ToD-BERT style checkpoint: keeps [SYS]/[USR] markers")
    g = ap.add_argument_group("training / testing")
    g.add_argument("--testing", action="store_true")
    g.add_argument("--predict", default=None, metavar="FILE",
                   help="label an n-best file with <exp_dir>/model.pt (loaded as --testing does): one 'ASR \\t<=>\\t labels' line per "
                        "input line, in input order.  Input lines need only the ASR field.  One GPU")
    g.add_argument("--predict_output", default=None, metavar="PATH", help="--predict output (default: <exp_dir>/<basename of FILE>.pred)")
    g.add_argument("--predict_attention", default=None, metavar="PATH",
                   help="with --predict: also write one JSON line per input line, in input order - the segments of the utterance "
                        "(cls, sys, h1, h2, ..), their token counts and, per layer, the share of the CLS row's attention (mean over "
                        "heads) that falls on each segment")
    g.add_argument("--predict_attribution", default=None, metavar="PATH",
                   help="with --predict: also write one JSON line per input line, in input order - for every label of the .pred line, "
                        "its score, the score at the all-padding baseline and the integrated-gradients attribution of the score to each "
                        "token and each segment (cls, sys, h1, h2, ..)")
    g.add_argument("--attribution_steps", type=int, default=32, metavar="M",
                   help="--predict_attribution: path points of the integrated-gradients midpoint rule (>= 1)")
    g.add_argument("--predict_rollout", default=None, metavar="PATH",
                   help="with --predict: also write one JSON line per input line, in input order - the attention rollout of the "
                        "[CLS] row (Abnar & Zuidema, 2020: the product over the layers of R I + (1 - R) mean-over-heads attention), "
                        "per token and per segment (cls, sys, h1, h2, ..).  Not with --predict_fp8, --head_mask or --compact_heads")
    g.add_argument("--rollout_residual", type=float, default=None, metavar="R",
                   help="--predict_rollout: the weight R of the residual connection in every layer, 0 <= R <= 1 (default 0.5)")
    g.add_argument("--token_keep", default=None, metavar="SPEC",
                   help="with --predict FILE: drop low-attention tokens between layers (PoWER-BERT at a fixed count per layer; "
                        "model.predict(token_keep=...)).  SPEC: L - 1 comma-separated non-increasing counts, the tokens per utterance "
                        "that leave each layer but the last, or FIRST:LAST, a geometric schedule between the two.  [CLS] is always "
                        "kept; counts >= the sequence length change nothing.  Not with --predict_fp8, --head_mask, --compact_heads, "
                        "--predict_attention, --predict_attribution, --predict_rollout, --testing or --head_importance")
    g.add_argument("--predict_tokens", default=None, metavar="PATH",
                   help="with --token_keep: also write one JSON line per input line, in input order - the segments of the utterance "
                        "(cls, sys, h1, h2, ..), their token counts and, per eliminating layer boundary, how many tokens of each "
                        "segment are still there")
    g.add_argument("--predict_fp8", action="store_true",
                   help="with --predict FILE --dtype fp8w: label the file with the fp8 inference (model.predict(fp8=True)) - the "
                        "full-width GEMMs on the fp8 MFMA with static activation scales calibrated on the first --fp8_calib_batches "
                        "batches of FILE.  A value beyond twice the calibrated amax saturates silently.  Not with --head_mask, "
                        "--compact_heads, --predict_attention or --predict_attribution")
    g.add_argument("--fp8_calib_batches", type=int, default=8, metavar="N",
                   help="--predict_fp8: batches of FILE the activation scales are calibrated on (>= 1; default 8)")
    g.add_argument("--head_mask", default=None, metavar="FILE",
                   help="gate the attention heads (HF's head_mask) for --testing, --predict and --head_importance: a JSON list of L rows "
                        "of `heads` numbers, 0 = head pruned, 1 = kept (any float scales the head's output).  Not for a training run")
    g.add_argument("--compact_heads", action="store_true",
                   help="with --predict FILE --head_mask FILE: run only the heads the mask keeps - per layer a [3 64k, H] QKV matrix, "
                        "a k-head attention and an [H, 64k] output matrix with the gate folded in, rebuilt from the weights per "
                        "batch - instead of gating full-width layers; same labels.  Not with --testing or --head_importance (they run "
                        "the stash forward), --predict_attention or --predict_attribution")
    g.add_argument("--train_head_mask", default=None, metavar="FILE",
                   help="train under a head mask (the format of --head_mask; usually the pruned_mask of --head_importance --prune_heads, "
                        "with --init_checkpoint): the fine-tune that recovers what pruning lost (Michel et al., 2019).  Every step and "
                        "every epoch's evaluation run under the mask; model.pt keeps the full tensors, the mask is not in it - evaluate "
                        "with --testing --head_mask FILE.  The experiment directory gains __hm_<digest of the mask>.  A training flag, one "
                        "GPU; not with --head_mask, --dtype fp8w or --adv_epsilon")
    g.add_argument("--head_importance", default=None, metavar="PATH",
                   help="score every attention head on the --valid_file split with <exp_dir>/model.pt (Michel et al., 2019: the mean "
                        "over utterances of |d loss / d head gate|) and write one JSON object to PATH: importance and normalized "
                        "(per-layer l2) [L][heads] tables, the head mask in force and, with --prune_heads, pruned_mask.  One GPU")
    g.add_argument("--prune_heads", type=int, default=None, metavar="N",
                   help="with --head_importance: also write pruned_mask, the mask in force with its N lowest-importance heads set to "
                        "0 (at least one head per layer stays); feed it back through --head_mask")
    g.add_argument("--deviceId", type=int, default=-1,
                   help="as the reference (n_best_asr_bert.py:116-126): 0 = pick a GPU automatically (here: the first visible one; "
                        "the reference asks gpustat / NVML for the least loaded), k > 0 = GPU k-1, -1 = CPU (refused: the path is "
                        "HIP-only).  Under torchrun every rank uses its LOCAL_RANK GPU instead")
    g.add_argument("--random_seed", type=int, default=999)
    g.add_argument("--l2", type=float, default=0)
    g.add_argument("--dropout", type=float, default=0.0)
    g.add_argument("--bert_dropout", type=float, default=0.1)
    g.add_argument("--batchSize", type=int, default=16)
    g.add_argument("--max_norm", type=float, default=5.0)
    g.add_argument("--max_epoch", type=int, default=50)
    g.add_argument("--experiment", default="exp")
    g.add_argument("--optim_choice", default="bertadam", choices=["adam", "adamw", "bertadam"],
                   help="fused HIP optimizers, as n_best_asr_bert.py:266-277,551-569: bertadam (the shipped script's choice; "
                        "each tensor clipped to norm 1, warmup-linear schedule) | adam (torch Adam: one lr for every tensor, "
                        "--bert_lr ignored, L2 decay --l2, bias correction) | adamw (HF AdamW, correct_bias=False: BertAdam's "
                        "groups, decoupled decay 0.01, linear warm-up / decay schedule; needs --restated_adamw).  adam and adamw "
                        "clip the global gradient norm to --max_norm")
    g.add_argument("--lr", type=float, default=5e-4)
    g.add_argument("--bert_lr", type=float, default=1e-5)
    g.add_argument("--warmup_proportion", type=float, default=0.1)
    g.add_argument("--init_type", default="uf", choices=["uf", "xuf", "normal"])
    g.add_argument("--init_range", type=float, default=0.2)
    g.add_argument("--with_system_act", action="store_true")
    g.add_argument("--coverage", type=float)
    g.add_argument("--add_l2_loss", action="store_true")
    g.add_argument("--without_system_act", action="store_true")
    g.add_argument("--add_segment_ids", action="store_true")
    g = ap.add_argument_group("additive flags of this build")
    g.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "fp8w"],
                   help="bf16 (default) | f32 (parity path) | fp8w: the bf16 path with every GEMM of the encoder layers (forward, input "
                        "gradient, weight gradient) on the CDNA4 block-scaled fp8 MFMA, from per-matrix-scaled e4m3 copies of the weights "
                        "and e4m3 copies of activations / gradients (BASELINE configs[4]: 'fp8 weights'); fp32 master weights, attention, "
                        "LayerNorm, heads and the optimizer are unchanged")
    g.add_argument("--n_best", type=int, default=None, help="keep only the first n hypotheses of every utterance")
    g.add_argument("--init_checkpoint", default=None, help="state dict (reference keys) to start from")
    g.add_argument("--pretrained_path", default=None,
                   help="LOCAL HF-format encoder checkpoint (directory or model.safetensors / pytorch_model.bin); its vocab.txt is "
                        "used when --vocab is not given.  Stands in for from_pretrained(name), which needs the network")
    g.add_argument("--stop_after_epoch", type=int, default=None, help="leave after this epoch (preemption drills; use with --resume)")
    g.add_argument("--resume", action="store_true", help="continue from <exp_dir>/last.pt (model + optimizer state + epoch)")
    g.add_argument("--vocab", default=None, help="WordPiece vocabulary: vocab.txt (one token per line) or a JSON list")
    g.add_argument("--label_space", default=None, help="JSON with top2bottom / idx2label instead of memory.pt")
    g.add_argument("--encoder_layers", type=int, default=None, help="override the number of encoder layers (smoke runs)")
    g.add_argument("--shard_optimizer", default="off", choices=["on", "off"],
                   help="data parallel only: the optimizer (bertadam, adam or adamw) sharded over the ranks (reduce-to-owner + owner "
                        "broadcasts, DESIGN 6) instead of replicated behind the all-reduce.  Opt-in: the path has not run over RCCL on "
                        "more than one GPU yet")
    g.add_argument("--restated_adamw", action="store_true",
                   help="run --optim_choice adamw.  The reference's AdamW (transformers.optimization.AdamW, correct_bias=False) is "
                        "not in current transformers releases, so its branch cannot run there; this build restates the update rule "
                        "(DESIGN.md, kernel K9b) and checks it against that restatement, not against the reference's own code")
    g.add_argument("--ema_decay", type=float, default=None, metavar="D",
                   help="keep an exponential moving average of the weights on the device (0 <= D < 1; decay warmed up as "
                        "min(D, (1 + t) / (10 + t)) over the optimizer steps t): every epoch's valid / test evaluation and model.pt use "
                        "the averaged weights, training goes on with the raw ones; last.pt keeps the raw weights and, in the optimizer "
                        "state, the average.  A training flag: --testing / --predict / --head_importance read model.pt, which already "
                        "holds the averaged weights.  Not with --shard_optimizer on")
    g.add_argument("--distill_from", default=None, metavar="PATH",
                   help="knowledge distillation: train this model (the student, e.g. --encoder_layers 6) on the scores of a teacher - "
                        "PATH is a state dict with the reference's keys (a model.pt of either implementation), loaded into a second "
                        "model of the same family (bf16, or f32 with --dtype f32; never fp8, dropout 0) whose predict() runs ahead of "
                        "every training step.  The gradient is that of (1 - A) * hard loss + A * soft loss, the soft loss being the "
                        "three loss terms with the teacher's scores in place of the labels; the [Train] line's Loss stays the hard "
                        "loss.  A training flag, one GPU")
    g.add_argument("--distill_teacher_layers", type=int, default=None, metavar="N",
                   help="with --distill_from: the teacher's number of encoder layers (default: the family's, whatever "
                        "--encoder_layers says)")
    g.add_argument("--distill_alpha", type=float, default=0.5, metavar="A", help="with --distill_from: weight of the soft loss, 0 <= A <= 1")
    g.add_argument("--distill_temperature", type=float, default=None, metavar="T",
                   help="with --distill_from: distil from the teacher's LOGITS at temperature T (finite, > 0): both models' logits are "
                        "divided by T inside the heads kernel and the soft loss is T^2 x the three terms on the tempered scores "
                        "(Hinton et al., 2015).  Given, even as 1.0, the logits path runs (nbest_stc_heads_kd_t) and exp_dir gains "
                        "__kdT_<T>; not given, the teacher's probabilities are the targets, as without the flag")
    g.add_argument("--distill_init_layers", default=None, metavar="i0,i1,...",
                   help="with --distill_from: initialise student layer k from teacher layer i_k and copy the teacher's embeddings "
                        "and heads (one index per student layer, each below the teacher's depth); replaces --init_checkpoint")
    g.add_argument("--rdrop_alpha", type=float, default=None, metavar="A",
                   help="R-Drop (Liang et al., 2021): every training step runs each utterance twice in one batch of 2 x batchSize rows "
                        "(the dropout hashes are keyed on the position in the batch, so the two copies get independent masks) and adds "
                        "A x the symmetric KL between the two copies' outputs to the hard loss of both (nbest_stc_heads_rdrop); A finite "
                        "and > 0.  The [Train] line's Loss is half the hard loss of the 2 x batchSize rows and its F1 that of the first "
                        "copies; exp_dir gains __rdrop_<A>.  A training flag, one GPU; needs --dropout or --bert_dropout > 0; not with "
                        "--distill_from")
    g.add_argument("--adv_epsilon", type=float, default=None, metavar="E",
                   help="FGM adversarial training on the word embeddings (Miyato et al., 2017): every training step runs the ASR pass a "
                        "second time with each utterance's word embeddings moved by E (L2 norm) along the gradient of the step's loss "
                        "(nbest_embed_adv_delta, nbest_encoder_desc.emb_delta), under the same dropout bits, and the optimizer steps once on "
                        "the sum of both passes' gradients; E finite and > 0.  The [Train] line's Loss and F1 are the clean pass's; exp_dir "
                        "gains __fgm_<E>.  A training flag, one GPU; not with --distill_from, --rdrop_alpha, --dtype fp8w, "
                        "--freeze_embeddings or --freeze_layers K > 0")
    g.add_argument("--sam_rho", type=float, default=None, metavar="R",
                   help="sharpness-aware minimization (Foret et al., 2021): every training step takes the gradient at w + e, e = R g / "
                        "||g|| (one norm over every trainable tensor, nbest_sam_perturb), under the same dropout bits as the pass that "
                        "produced g, and applies it at w (nbest_sam_restore); R finite and > 0.  About twice the step.  The [Train] "
                        "line's Loss and F1 are the first pass's (at w); one more line per epoch carries the mean loss rise at w + e and "
                        "the mean gradient norm; exp_dir gains __sam_<R>.  A training flag, one GPU; works with the three optimizers, "
                        "--add_l2_loss, --rdrop_alpha, --distill_from, --contrastive_weight, --ema_decay, --freeze_* and --resume; not "
                        "with --adv_epsilon, --lora_rank, --dtype fp8w, --train_head_mask, --shard_optimizer on or --n_layers 12 "
                        "(gradient accumulation)")
    g.add_argument("--sam_adaptive", action="store_true",
                   help="with --sam_rho: ASAM (Kwon et al., 2021), the scale-invariant variant: e = R T^2 g / ||T g||, T = |w| + "
                        "--sam_eta element by element (nbest_sam_norms); exp_dir gains __asam_<R>_<eta> instead")
    g.add_argument("--sam_eta", type=float, default=None, metavar="ETA",
                   help="with --sam_rho --sam_adaptive: the floor added to |w|; finite and > 0 (default 0.01).  Plain SAM does not read "
                        "it: given without --sam_adaptive it is refused")
    g.add_argument("--contrastive_weight", type=float, default=None, metavar="W",
                   help="in-batch contrastive alignment of the n-best list with its transcript (Chang & Chen, 2022; the loss of SimCSE / "
                        "CLIP): every step runs the transcript pass and adds W x the symmetric InfoNCE between the ASR and the "
                        "transcript CLS rows to the loss (nbest_cls_contrast) - each utterance's ASR row must pick its own transcript "
                        "out of the batch's and the other way round; utterances with identical transcripts stay out of each other's "
                        "denominators.  W finite and > 0, a weight per utterance next to the summed BCE terms.  The [Train] line's Loss "
                        "stays the hard loss (+ MSE); one more line per epoch carries the term and its alignment-hit rate; exp_dir gains "
                        "__cl_<W>_<T>.  Under gradient accumulation the negatives are those of the micro-batch.  A training flag, one "
                        "GPU; not with --adv_epsilon, --dtype fp8w or --train_head_mask")
    g.add_argument("--contrastive_temperature", type=float, default=None, metavar="T",
                   help="with --contrastive_weight: the temperature the cosines are divided by; finite and > 0 (default 0.1)")
    g.add_argument("--lora_rank", type=int, default=None, metavar="R",
                   help="LoRA (Hu et al., 2022): freeze the encoder and train a rank-R update W0 + (A / R) B A on the --lora_targets "
                        "matrices of every layer, plus the STC heads; 1 <= R <= 64.  The arenas keep the merged weights (the encoder "
                        "kernels are untouched: nbest_lora_grad projects the dense weight gradient onto the factors, nbest_lora_merge "
                        "rewrites the adapted blocks after the update), so model.pt holds merged weights in the reference's keys and "
                        "every scoring flag works on it; lora.pt (factors + heads + base digest, a few MB) is written next to it; "
                        "exp_dir gains __lora_r<R>_a<A>_<targets joined by '+'>.  A training flag, one GPU, --optim_choice bertadam; "
                        "not with --dtype fp8w, --shard_optimizer on, --ema_decay, --freeze_embeddings / --freeze_layers, "
                        "--train_head_mask or --adv_epsilon.  Adapter dropout is not built (it cannot act on merged weights)")
    g.add_argument("--lora_alpha", type=float, default=None, metavar="A", help="with --lora_rank: the update is scaled by A / R (default 2 R)")
    g.add_argument("--lora_targets", default=None, metavar="t0,t1,...",
                   help="with --lora_rank: the adapted matrices, from query, key, value, attn_out, ffn_up, ffn_down (default query,value)")
    g.add_argument("--lora_lr", type=float, default=None, metavar="LR", help="with --lora_rank: learning rate of the factors (default --lr)")
    g.add_argument("--lora_adapter", default=None, metavar="FILE",
                   help="with --testing, --predict or --head_importance: after <exp_dir>/model.pt (the BASE weights) is loaded, apply "
                        "the lora.pt of a --lora_rank run (factors and heads) and merge.  The file carries a digest of the base blocks "
                        "it was trained on: a model.pt that differs there (an already merged one, say) exits naming both digests")
    opt = ap.parse_args(argv)
    scoring = (("--testing", opt.testing), ("--predict", opt.predict is not None), ("--head_importance", opt.head_importance is not None))
    if opt.lora_rank is None:
        for flag, v in (("--lora_alpha", opt.lora_alpha), ("--lora_targets", opt.lora_targets), ("--lora_lr", opt.lora_lr)):
            if v is not None:
                ap.error("%s is a setting of --lora_rank: pass --lora_rank R too" % flag)
    else:
        from . import lora as _lora
        for flag, on in scoring:
            if on:
                ap.error("--lora_rank is a training flag: %s reads model.pt from the directory named without it (apply an adapter "
                         "file to a base model with --lora_adapter FILE)" % flag)
        if opt.lora_alpha is None:
            opt.lora_alpha = 2.0 * opt.lora_rank
        try:
            opt.lora_rank, opt.lora_alpha, _ = _lora.check_config(opt.lora_rank, opt.lora_alpha, 1)
            opt.lora_targets = ",".join(_lora.parse_targets("query,value" if opt.lora_targets is None else opt.lora_targets))
        except ValueError as e:
            ap.error("--lora_rank / --lora_alpha / --lora_targets: %s" % e)
        if opt.lora_lr is None:
            opt.lora_lr = opt.lr
        if not (opt.lora_lr > 0.0 and math.isfinite(opt.lora_lr)):
            ap.error("--lora_lr %s: must be a finite number > 0" % opt.lora_lr)
        if opt.dtype == "fp8w":
            ap.error("--lora_rank together with --dtype fp8w is not built (the e4m3 weight copies are quantised from the full master "
                     "after every step; LoRA under fp8 has not been measured)")
        if opt.optim_choice != "bertadam":
            ap.error("--lora_rank together with --optim_choice %s is not built (its global-norm clip would have to span the main and "
                     "the adapter arena); use --optim_choice bertadam" % opt.optim_choice)
        if opt.shard_optimizer == "on":
            ap.error("--lora_rank together with --shard_optimizer on is not built (the adapter arena is not sharded)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--lora_rank runs on one GPU: LoRA under data parallelism is not built (world size %s)" % os.environ["WORLD_SIZE"])
        if opt.ema_decay is not None:
            ap.error("--lora_rank together with --ema_decay is not built (the average would have to follow the factors, not the "
                     "merged weights)")
        if opt.freeze_embeddings or opt.freeze_layers > 0:
            ap.error("--lora_rank freezes the whole encoder itself: not with --freeze_embeddings or --freeze_layers (adapting only "
                     "some layers from the command line is not built)")
        if opt.train_head_mask is not None:
            ap.error("--lora_rank together with --train_head_mask is not built (LoRA under a head mask)")
        if opt.adv_epsilon is not None:
            ap.error("--lora_rank together with --adv_epsilon is not built (FGM needs trainable embeddings, LoRA freezes them)")
    if opt.lora_adapter is not None:
        if not any(on for _, on in scoring):
            ap.error("--lora_adapter applies to --testing, --predict and --head_importance: a training run writes lora.pt itself "
                     "(--lora_rank)")
        if opt.dtype == "fp8w":
            ap.error("--lora_adapter together with --dtype fp8w is not built (LoRA on an fp8w model)")
        if not os.path.isfile(opt.lora_adapter):
            ap.error("--lora_adapter %s: no such file" % opt.lora_adapter)
    if opt.contrastive_weight is None:
        if opt.contrastive_temperature is not None:
            ap.error("--contrastive_temperature applies to --contrastive_weight only")
    else:
        if not (opt.contrastive_weight > 0.0 and math.isfinite(opt.contrastive_weight)):
            ap.error("--contrastive_weight %s: must be a finite number > 0" % opt.contrastive_weight)
        if opt.contrastive_temperature is None:
            opt.contrastive_temperature = 0.1
        if not (opt.contrastive_temperature > 0.0 and math.isfinite(opt.contrastive_temperature)):
            ap.error("--contrastive_temperature %s: must be a finite number > 0" % opt.contrastive_temperature)
        for flag, on in (("--testing", opt.testing), ("--predict", opt.predict is not None), ("--head_importance", opt.head_importance is not None)):
            if on:
                ap.error("--contrastive_weight is a training flag: %s reads model.pt from the directory named without it" % flag)
        if opt.adv_epsilon is not None:
            ap.error("--contrastive_weight together with --adv_epsilon is not built (the adversarial pass has the hard terms only)")
        if opt.dtype == "fp8w":
            ap.error("--contrastive_weight together with --dtype fp8w is not built (e4m3 noise on the CLS rows is of the size of the "
                     "cosine differences the term resolves)")
        if opt.train_head_mask is not None:
            ap.error("--contrastive_weight together with --train_head_mask is not built (the contrastive term under a head mask)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--contrastive_weight runs on one GPU: negatives across ranks are not built (world size %s)" % os.environ["WORLD_SIZE"])
    if opt.adv_epsilon is not None:
        if not (opt.adv_epsilon > 0.0 and math.isfinite(opt.adv_epsilon)):
            ap.error("--adv_epsilon %s: must be a finite number > 0" % opt.adv_epsilon)
        for flag, on in (("--testing", opt.testing), ("--predict", opt.predict is not None), ("--head_importance", opt.head_importance is not None)):
            if on:
                ap.error("--adv_epsilon is a training flag: %s reads model.pt from the directory named without it" % flag)
        if opt.distill_from is not None:
            ap.error("--adv_epsilon together with --distill_from is not built (the adversarial pass has the hard terms only)")
        if opt.rdrop_alpha is not None:
            ap.error("--adv_epsilon together with --rdrop_alpha is not built (the adversarial pass has the hard terms only)")
        if opt.dtype == "fp8w":
            ap.error("--adv_epsilon together with --dtype fp8w is not built (the fp8 forward has no perturbed embedding)")
        if opt.freeze_embeddings or opt.freeze_layers > 0:
            ap.error("--adv_epsilon needs trainable embeddings: not with --freeze_embeddings or --freeze_layers K > 0 (the perturbation "
                     "is formed from the gradient w.r.t. the word embeddings)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--adv_epsilon runs on one GPU: FGM under data parallelism is not built (world size %s)" % os.environ["WORLD_SIZE"])
    if opt.rdrop_alpha is not None:
        if not (opt.rdrop_alpha > 0.0 and math.isfinite(opt.rdrop_alpha)):
            ap.error("--rdrop_alpha %s: must be a finite number > 0" % opt.rdrop_alpha)
        for flag, on in (("--testing", opt.testing), ("--predict", opt.predict is not None), ("--head_importance", opt.head_importance is not None)):
            if on:
                ap.error("--rdrop_alpha is a training flag: %s reads model.pt from the directory named without it" % flag)
        if opt.distill_from is not None:
            ap.error("--rdrop_alpha together with --distill_from is not built (one soft term per step)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--rdrop_alpha runs on one GPU: R-Drop under data parallelism is not built (world size %s)" % os.environ["WORLD_SIZE"])
        if opt.dropout == 0 and opt.bert_dropout == 0:
            ap.error("--rdrop_alpha needs dropout: with --dropout 0 and --bert_dropout 0 the two copies of an utterance are identical "
                     "and the consistency term is zero")
    if opt.distill_from is None:
        if opt.distill_teacher_layers is not None or opt.distill_init_layers is not None:
            ap.error("--distill_teacher_layers / --distill_init_layers describe the teacher of --distill_from: pass --distill_from PATH too")
        if opt.distill_temperature is not None:
            ap.error("--distill_temperature softens the teacher of --distill_from: pass --distill_from PATH too")
    else:
        if opt.distill_temperature is not None and not (opt.distill_temperature > 0.0 and math.isfinite(opt.distill_temperature)):
            ap.error("--distill_temperature %s: must be a finite number > 0" % opt.distill_temperature)
        if not 0.0 <= opt.distill_alpha <= 1.0:
            ap.error("--distill_alpha %s: must be in [0, 1]" % opt.distill_alpha)
        for flag, on in (("--testing", opt.testing), ("--predict", opt.predict is not None), ("--head_importance", opt.head_importance is not None)):
            if on:
                ap.error("--distill_from is a training flag: %s reads the student's model.pt and needs no teacher" % flag)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--distill_from runs on one GPU: a data-parallel teacher is not built (world size %s)" % os.environ["WORLD_SIZE"])
        if opt.distill_teacher_layers is not None and opt.distill_teacher_layers < 1:
            ap.error("--distill_teacher_layers %d: must be >= 1" % opt.distill_teacher_layers)
        if opt.distill_init_layers is not None:
            if opt.init_checkpoint:
                ap.error("--distill_init_layers replaces --init_checkpoint (the student starts from the teacher's layers): pass one of them")
            try:
                opt.distill_init_layers = [int(x) for x in opt.distill_init_layers.split(",")]
            except ValueError:
                ap.error("--distill_init_layers %s: expected comma-separated layer indices, e.g. 1,3,5,7,9,11" % opt.distill_init_layers)
            if any(i < 0 for i in opt.distill_init_layers):
                ap.error("--distill_init_layers: layer indices must be >= 0")
    if opt.ema_decay is not None:
        if not 0.0 <= opt.ema_decay < 1.0:
            ap.error("--ema_decay %s: must be in [0, 1)" % opt.ema_decay)
        if opt.shard_optimizer == "on":
            ap.error("--ema_decay is not built for --shard_optimizer on (the fp32 master is current only on each range's owner)")
        if opt.testing or opt.predict is not None or opt.head_importance is not None:
            ap.error("--ema_decay is a training flag: --testing, --predict and --head_importance read model.pt, which already holds "
                     "the averaged weights of a run that used it")
    if opt.optim_choice == "adamw" and not opt.restated_adamw:
        ap.error("--optim_choice adamw: the reference's AdamW is not in current transformers releases, so the reference cannot run "
                 "it; this build's restatement of its update rule runs when --restated_adamw is passed too")
    if opt.deviceId < 0:
        ap.error("--deviceId -1 (CPU) is not available: the path is HIP-only")
    if opt.freeze_layers < 0:
        ap.error("--freeze_layers %d: must be >= 0" % opt.freeze_layers)
    if opt.pre_trained_model == "roberta":
        ap.error("--pre_trained_model roberta: the reference passes segment ids (1 after the first separator) to RoBERTa's "
                 "one-row token-type table in both encoder passes (models/model.py:45,56; n_best_asr_bert.py:255) and fails "
                 "with an IndexError; use bert or xlm-roberta")
    if opt.pre_trained_model and opt.pre_trained_model not in ncfg.NAMED:
        ap.error("--pre_trained_model %s: known shapes are %s" % (opt.pre_trained_model, ", ".join(sorted(ncfg.NAMED))))
    if opt.predict_attention is not None and opt.predict is None:
        ap.error("--predict_attention is an output of --predict: pass --predict FILE too")
    if opt.predict_attribution is not None and opt.predict is None:
        ap.error("--predict_attribution is an output of --predict: pass --predict FILE too")
    if opt.predict_rollout is not None:
        if opt.predict is None:
            ap.error("--predict_rollout is an output of --predict: pass --predict FILE too")
        if opt.predict_fp8:
            ap.error("--predict_rollout together with --predict_fp8 is not built (the rollout runs the stash forward)")
        if opt.head_mask is not None or opt.compact_heads:
            ap.error("--predict_rollout together with %s is not built (the mean over heads under a head mask is not defined here)"
                     % ("--compact_heads" if opt.compact_heads else "--head_mask"))
    if opt.predict_tokens is not None and opt.token_keep is None:
        ap.error("--predict_tokens is an output of --token_keep: pass --predict FILE --token_keep SPEC too")
    if opt.token_keep is not None:
        if opt.predict is None:
            ap.error("--token_keep is an inference flag: pass it with --predict FILE (%s)"
                     % ("--testing runs the stash forward, where dropping tokens is not built" if opt.testing else
                        "--head_importance runs the stash forward, where dropping tokens is not built" if opt.head_importance is not None
                        else "training under token elimination is not built"))
        for flag, on in (("--predict_fp8", opt.predict_fp8), ("--head_mask", opt.head_mask is not None), ("--compact_heads", opt.compact_heads),
                         ("--predict_attention", opt.predict_attention is not None),
                         ("--predict_attribution", opt.predict_attribution is not None),
                         ("--predict_rollout", opt.predict_rollout is not None), ("--testing", opt.testing),
                         ("--head_importance", opt.head_importance is not None)):
            if on:
                ap.error("--token_keep together with %s is not built" % flag)
        try:
            trainer.parse_token_keep(opt.token_keep, None)
        except ValueError as e:
            ap.error("--token_keep %s: %s" % (opt.token_keep, e))
    if opt.rollout_residual is not None:
        if opt.predict_rollout is None:
            ap.error("--rollout_residual is a setting of --predict_rollout: pass --predict_rollout PATH too")
        if not (0.0 <= opt.rollout_residual <= 1.0):
            ap.error("--rollout_residual must be in [0, 1] (got %g)" % opt.rollout_residual)
    else:
        opt.rollout_residual = 0.5
    if opt.attribution_steps < 1:
        ap.error("--attribution_steps must be >= 1 (got %d)" % opt.attribution_steps)
    if opt.fp8_calib_batches < 1:
        ap.error("--fp8_calib_batches must be >= 1 (got %d)" % opt.fp8_calib_batches)
    if opt.predict_fp8:
        if opt.predict is None:
            ap.error("--predict_fp8 is a mode of --predict: pass --predict FILE too")
        if opt.dtype != "fp8w":
            ap.error("--predict_fp8 needs a model with the fp8 forward: pass --dtype fp8w (got --dtype %s)" % opt.dtype)
        if opt.compact_heads:
            ap.error("--predict_fp8 together with --compact_heads is not built (compact heads in fp8)")
        if opt.head_mask is not None:
            ap.error("--predict_fp8 together with --head_mask is not built (the fp8 forward has no gated context)")
        if opt.predict_attention is not None:
            ap.error("--predict_fp8 together with --predict_attention is not built (the CLS attention maps in fp8)")
        if opt.predict_attribution is not None:
            ap.error("--predict_fp8 together with --predict_attribution is not built (the attribution runs the stash forward)")
    if opt.predict is not None:
        if not os.path.isfile(opt.predict):
            ap.error("--predict %s: no such file" % opt.predict)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--predict runs on one GPU: start it without torchrun (world size %s)" % os.environ["WORLD_SIZE"])
    if opt.prune_heads is not None and opt.head_importance is None:
        ap.error("--prune_heads prunes by the scores of --head_importance: pass --head_importance PATH too")
    if opt.prune_heads is not None and opt.prune_heads < 0:
        ap.error("--prune_heads must be >= 0 (got %d)" % opt.prune_heads)
    if opt.head_importance is not None:
        if opt.testing or opt.predict is not None:
            ap.error("--head_importance is a run of its own: pass it without --testing / --predict")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--head_importance runs on one GPU: start it without torchrun (world size %s)" % os.environ["WORLD_SIZE"])
    if opt.head_mask is not None:
        if not (opt.testing or opt.predict is not None or opt.head_importance is not None):
            ap.error("--head_mask applies to --testing, --predict and --head_importance; training under a head mask is not built")
        if not os.path.isfile(opt.head_mask):
            ap.error("--head_mask %s: no such file" % opt.head_mask)
    if opt.compact_heads:
        if opt.testing or opt.head_importance is not None:
            ap.error("--compact_heads applies to --predict only: %s runs the stash forward, and compacting the heads there is not "
                     "built" % ("--testing" if opt.testing else "--head_importance"))
        if opt.predict is None:
            ap.error("--compact_heads is an inference flag: pass it with --predict FILE --head_mask FILE (training with compacted "
                     "heads is not built)")
        if opt.head_mask is None:
            ap.error("--compact_heads compacts the heads a mask prunes: pass --head_mask FILE too")
        if opt.predict_attention is not None:
            ap.error("--compact_heads together with --predict_attention is not built (the CLS attention maps are indexed by "
                     "original head)")
        if opt.predict_attribution is not None:
            ap.error("--compact_heads together with --predict_attribution is not built (the attribution runs the gated stash "
                     "forward; drop --compact_heads)")
    if opt.train_head_mask is not None:
        for flag, on in (("--testing", opt.testing), ("--predict", opt.predict is not None), ("--head_importance", opt.head_importance is not None)):
            if on:
                ap.error("--train_head_mask is a training flag: %s runs under --head_mask FILE, on the directory named without it" % flag)
        if opt.head_mask is not None:
            ap.error("--train_head_mask together with --head_mask: a training run takes its mask from --train_head_mask alone")
        if opt.dtype == "fp8w":
            ap.error("--train_head_mask together with --dtype fp8w is not built (the fp8 forward has no gated context)")
        if opt.adv_epsilon is not None:
            ap.error("--train_head_mask together with --adv_epsilon is not built (FGM under a head mask)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--train_head_mask runs on one GPU: training under a head mask under data parallelism is not built (world size %s)"
                     % os.environ["WORLD_SIZE"])
        if not os.path.isfile(opt.train_head_mask):
            ap.error("--train_head_mask %s: no such file" % opt.train_head_mask)
        try:
            trainer.head_mask_file_digest(opt.train_head_mask)
        except ValueError as e:
            ap.error("--train_head_mask: %s" % e)
    if opt.sam_rho is None:
        if opt.sam_adaptive or opt.sam_eta is not None:
            ap.error("--sam_adaptive / --sam_eta are settings of --sam_rho: pass --sam_rho R too")
    else:
        if not (opt.sam_rho > 0.0 and math.isfinite(opt.sam_rho)):
            ap.error("--sam_rho %s: must be a finite number > 0" % opt.sam_rho)
        if opt.sam_eta is not None and not opt.sam_adaptive:
            ap.error("--sam_eta is a setting of --sam_adaptive: pass --sam_adaptive too")
        if opt.sam_eta is None:
            opt.sam_eta = 0.01
        if not (opt.sam_eta > 0.0 and math.isfinite(opt.sam_eta)):
            ap.error("--sam_eta %s: must be a finite number > 0" % opt.sam_eta)
        for flag, on in scoring:
            if on:
                ap.error("--sam_rho is a training flag: %s reads model.pt from the directory named without it" % flag)
        if opt.adv_epsilon is not None:
            ap.error("--sam_rho together with --adv_epsilon is not built (two two-pass schemes in one step)")
        if opt.lora_rank is not None:
            ap.error("--sam_rho together with --lora_rank is not built (the perturbation would have to follow the factors, not the "
                     "merged weights)")
        if opt.dtype == "fp8w":
            ap.error("--sam_rho together with --dtype fp8w is not built (the amax histories would record twice per step and the e4m3 "
                     "images would be cut from perturbed weights)")
        if opt.train_head_mask is not None:
            ap.error("--sam_rho together with --train_head_mask is not built (SAM under a head mask)")
        if opt.shard_optimizer == "on":
            ap.error("--sam_rho together with --shard_optimizer on is not built (the fp32 master is current only on each range's owner)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--sam_rho runs on one GPU: SAM under data parallelism is not built (world size %s)" % os.environ["WORLD_SIZE"])
        if opt.n_layers == 12:
            ap.error("--sam_rho together with --n_layers 12 is not built (that flag turns gradient accumulation on; the perturbation "
                     "is formed from one batch's gradient)")
    opt.gpu_index = 0 if opt.deviceId == 0 else opt.deviceId - 1            # n_best_asr_bert.py:116-126 (0: auto -> first GPU)
    # gradient accumulation exactly as the reference derives it (n_best_asr_bert.py:522): 4 micro-batches of batchSize / 4
    # per optimizer step when --n_layers 12 is passed (the shipped script never passes it -> 1)
    opt.n_accum_steps = 4 if opt.n_layers == 12 else 1
    opt.ontology = None if opt.ontology_path is None else json.load(open(opt.ontology_path))       # n_best_asr_bert.py:138-140
    return opt


def exp_dir(opt):
    """experiment directory name, the scheme of /root/reference/utils/util.py:20-55"""
    parts = ["nl_%s" % opt.n_layers, "nh_%s" % opt.n_head, "dk_%s" % opt.d_k, "dv_%s" % opt.d_v, "bs_%s" % opt.batchSize,
             "dp_%s_%s" % (opt.dropout, opt.bert_dropout),
             "opt_%s_%s_%s_%s" % (opt.optim_choice, opt.warmup_proportion, opt.lr, opt.bert_lr), "mn_%s" % opt.max_norm,
             "me_%s" % opt.max_epoch, "seed_%s" % opt.random_seed, "score_%s" % opt.score_util, "repr_%s" % opt.sent_repr,
             "cls_%s" % opt.cls_type]
    if getattr(opt, "freeze_embeddings", False) or getattr(opt, "freeze_layers", 0):     # only then: existing names stay as they are
        parts.append("fz_%s_%s" % ("emb" if opt.freeze_embeddings else "none", opt.freeze_layers))
    if getattr(opt, "ema_decay", None) is not None:                                      # the same rule
        parts.append("ema_%s" % opt.ema_decay)
    if getattr(opt, "distill_from", None) is not None:
        parts.append("kd_%s" % opt.distill_alpha)
        if getattr(opt, "distill_temperature", None) is not None:
            parts.append("kdT_%s" % opt.distill_temperature)
    if getattr(opt, "rdrop_alpha", None) is not None:
        parts.append("rdrop_%s" % opt.rdrop_alpha)
    if getattr(opt, "adv_epsilon", None) is not None:
        parts.append("fgm_%s" % opt.adv_epsilon)
    if getattr(opt, "contrastive_weight", None) is not None:
        parts.append("cl_%s_%s" % (opt.contrastive_weight, opt.contrastive_temperature))
    if getattr(opt, "sam_rho", None) is not None:
        parts.append("asam_%s_%s" % (opt.sam_rho, opt.sam_eta) if getattr(opt, "sam_adaptive", False) else "sam_%s" % opt.sam_rho)
    if getattr(opt, "lora_rank", None) is not None:
        from . import lora as _lora
        parts.append(_lora.exp_dir_part(opt.lora_rank, opt.lora_alpha, opt.lora_targets))
    if getattr(opt, "train_head_mask", None) is not None:                                # last: the mask's digest, not the file's name
        parts.append("hm_%s" % trainer.head_mask_file_digest(opt.train_head_mask))
    return os.path.join(opt.experiment, "data_%s" % opt.dataset, "__".join(parts))


def freeze_parameters(model, embeddings=False, layers=0):
    """--freeze_embeddings / --freeze_layers K: requires_grad_(False) on the embedding tensors and on those of encoder layers
    0..K-1, before the optimizer is built (everything else follows the parameters' flags, as for a user's own freezing code).
    Returns the names frozen."""
    L = model.cfg.num_hidden_layers
    if not 0 <= layers <= L:
        raise SystemExit("--freeze_layers %d: the encoder has %d layers" % (layers, L))
    pre = ["bert_encoder.embeddings."] if embeddings else []
    pre += ["bert_encoder.encoder.layer.%d." % l for l in range(layers)]
    frozen = set()
    for n, p in model.named_parameters():
        if n.startswith(tuple(pre)):
            p.requires_grad_(False)
            frozen.add(n)
    return frozen


def load_teacher(opt, family, cfg, labels, dev):
    """--distill_from: (the teacher, its state dict).  A second model of the student's family and vocabulary, --distill_teacher_layers
    deep (default: the family's depth), bf16 or - with --dtype f32 - f32, never fp8; no dropout, eval mode, no optimizer."""
    tcfg = ncfg.NAMED[family](hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    if opt.distill_teacher_layers:
        tcfg.num_hidden_layers = opt.distill_teacher_layers
    tcfg.vocab_size = cfg.vocab_size
    if not os.path.isfile(opt.distill_from):
        raise SystemExit("--distill_from %s: no such file" % opt.distill_from)
    sd = torch.load(opt.distill_from, map_location="cpu", weights_only=True)
    teacher = NBestSTCModel(tcfg, labels, device=dev, compute_dtype=torch.float32 if opt.dtype == "f32" else torch.bfloat16,
                            dropout=0.0, seed=opt.random_seed)
    try:
        teacher.load_reference_state(sd)
    except (KeyError, RuntimeError, ValueError) as e:
        raise SystemExit("--distill_from %s does not fit a %d-layer %s teacher (--distill_teacher_layers): %s"
                         % (opt.distill_from, tcfg.num_hidden_layers, family, e))
    teacher.eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    return teacher, sd


def _lora_checkpoint(model):
    from . import lora as _lora
    return _lora.checkpoint_entry(model)


def apply_lora_adapter(model, path):
    """--lora_adapter: the adapter file on top of the base weights the model holds; the model is left plain (merged weights, LoRA
    off), so everything that scores a model.pt runs as on a merged one"""
    from . import lora as _lora
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        _lora.load(model, sd, keep=False)
    except (ValueError, KeyError, RuntimeError) as e:
        raise SystemExit("--lora_adapter %s: %s" % (path, e))


def predict_output_path(opt):
    """where --predict writes: --predict_output, or <exp_dir>/<basename of FILE>.pred"""
    return opt.predict_output or os.path.join(exp_dir(opt), os.path.basename(opt.predict) + ".pred")


def load_memory(opt):
    if opt.label_space:
        d = json.load(open(opt.label_space))
        idx2label = d["idx2label"]
        return dict(top2bottom_dict={int(k): v for k, v in d["top2bottom"].items()}, idx2label=idx2label,
                    label2idx={l: i for i, l in enumerate(idx2label)}, word2idx=d.get("word2idx", {}))
    # memory.pt is a plain dict of dicts / lists: the safe loader reads it
    m = torch.load(os.path.join(opt.dataroot, "memory.pt"), weights_only=True)
    m["idx2label"] = [m["idx2label"][i] for i in range(len(m["idx2label"]))]
    return m


def load_tokenizer(opt, memory):
    for fn in ("vocab.txt", "sentencepiece.bpe.model"):
        if not opt.vocab and opt.pretrained_path and os.path.exists(os.path.join(opt.pretrained_path, fn)):
            opt.vocab = os.path.join(opt.pretrained_path, fn)
    if opt.vocab and opt.vocab.endswith(".model"):              # sentencepiece model (XLM-R family)
        return SentencePieceTokenizer(opt.vocab)
    if opt.vocab:
        if opt.vocab.endswith(".json"):
            vocab = json.load(open(opt.vocab))
        else:
            vocab = [l.rstrip("\n") for l in open(opt.vocab, encoding="utf-8")]
    else:
        words = sorted({w.lower() for w in memory.get("word2idx", {}) if isinstance(w, str)})
        vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [w for w in words if w and not w.startswith("[")]
        vocab = list(dict.fromkeys(vocab))
    return WordPieceTokenizer(vocab)


class _Log:
    def __init__(self, path, rank, append=False):
        self.fp = open(path, "a" if append else "w") if rank == 0 else None

    def info(self, msg):
        if self.fp:
            self.fp.write(msg + "\n")
            self.fp.flush()
            print(msg, flush=True)


def main(argv=None):
    opt = parse_arguments(argv)
    trainer.limit_host_threads()
    rank, world, local = trainer.init_distributed()
    dev = torch.device("cuda", local if world > 1 else opt.gpu_index)
    torch.cuda.set_device(dev)
    random.seed(opt.random_seed)
    np.random.seed(opt.random_seed)
    torch.manual_seed(opt.random_seed)

    memory = load_memory(opt)
    labels = ncfg.LabelSpace(memory["top2bottom_dict"], memory["idx2label"])
    opt.tokenizer = load_tokenizer(opt, memory)
    family = opt.pre_trained_model or "bert"
    cfg = ncfg.NAMED[family](hidden_dropout_prob=opt.bert_dropout, attention_probs_dropout_prob=opt.bert_dropout)
    if opt.encoder_layers:
        cfg.num_hidden_layers = opt.encoder_layers
    if (family == "bert" and not (opt.init_checkpoint or opt.pretrained_path or opt.distill_init_layers)) or opt.vocab:
        cfg.vocab_size = max(opt.tokenizer.vocab_size, 8)          # embedding table sized for the local vocabulary
    model = NBestSTCModel(cfg, labels, device=dev, compute_dtype=torch.float32 if opt.dtype == "f32" else torch.bfloat16,
                          dropout=opt.dropout, seed=opt.random_seed, fp8_forward=(opt.dtype == "fp8w"))
    teacher = None
    if opt.distill_from is not None:
        teacher, tsd = load_teacher(opt, family, cfg, labels, dev)
        opt.teacher = teacher
    if opt.distill_from is not None and opt.distill_init_layers is not None:
        if len(opt.distill_init_layers) != cfg.num_hidden_layers:
            raise SystemExit("--distill_init_layers: %d indices for a student of %d layers" % (len(opt.distill_init_layers), cfg.num_hidden_layers))
        try:
            model.load_reference_state(trainer.student_state_from_teacher(tsd, opt.distill_init_layers))
        except ValueError as e:
            raise SystemExit("--distill_init_layers: %s" % e)
    elif opt.init_checkpoint:
        model.load_model(opt.init_checkpoint)
    else:
        model.load_reference_state(synth.model_state(cfg, labels, seed=opt.random_seed))
        if opt.pretrained_path:
            model.load_pretrained_encoder(opt.pretrained_path)
    trainer.broadcast_parameters(model)
    frozen = freeze_parameters(model, opt.freeze_embeddings, opt.freeze_layers)
    n_params = sum(s.numel for s in model.arena.slots if s.name not in frozen)
    n_bert = sum(s.numel for s in model.arena.slots if "bert_encoder" in s.name and s.name not in frozen)
    lora_cfg = None
    if opt.lora_rank is not None:                          # after the weights are in place: they become the base
        lora_cfg = dict(rank=opt.lora_rank, alpha=opt.lora_alpha, targets=opt.lora_targets.split(","), seed=opt.random_seed)
        st = model.enable_lora(**lora_cfg)
        n_bert = st.n_trainable
        n_params = n_bert + sum(s.numel for s in model.arena.slots if s.name.startswith("clf."))
    # (the weights are in place: --init_checkpoint is the usual companion; a mask of the wrong shape exits before a directory is made)
    train_mask = None
    if opt.train_head_mask is not None:                    # after the weights are in place (--init_checkpoint is the usual companion)
        try:
            train_mask = trainer.read_head_mask(opt.train_head_mask, cfg.num_hidden_layers, cfg.num_attention_heads)
        except ValueError as e:
            raise SystemExit("--train_head_mask: %s" % e)
        model.set_head_mask(train_mask, trainable=True)    # every step and every epoch's evaluation below run under it
    opt.exp_dir = exp_dir(opt)
    if rank == 0:
        os.makedirs(opt.exp_dir, exist_ok=True)
        print("word vocab size:", opt.tokenizer.vocab_size)
        print("#labels:", labels.n_bottom)
        print("#top-labels:", labels.n_top)
        print("num params: {}".format(n_params))
        print("num bert params: {}, {}%".format(n_bert, 100 * n_bert / n_params))

    def load(split, coverage=None):
        fn = os.path.join(opt.dataroot, split)
        if not os.path.exists(fn):
            return None
        return trainer.EncodedSplit(trainer.read_wcn_data(fn, coverage), opt, memory)       # tokenised once per run

    if opt.head_mask is not None:
        try:
            model.set_head_mask(trainer.read_head_mask(opt.head_mask, cfg.num_hidden_layers, cfg.num_attention_heads),
                                compact=opt.compact_heads)
        except ValueError as e:
            raise SystemExit("--head_mask: %s" % e)

    if opt.head_importance is not None:
        model.load_model(os.path.join(opt.exp_dir, "model.pt"))
        if opt.lora_adapter is not None:
            apply_lora_adapter(model, opt.lora_adapter)
        data = load(opt.valid_file)
        if data is None:
            raise SystemExit("--head_importance: no split at %s" % os.path.join(opt.dataroot, opt.valid_file))
        t0 = time.time()
        model.eval()
        res = trainer.head_importance(model, data, opt, memory)
        mask = model.head_mask
        res["head_mask"] = [[1.0] * cfg.num_attention_heads for _ in range(cfg.num_hidden_layers)] if mask is None else mask.cpu().tolist()
        if opt.prune_heads is not None:
            try:
                res["pruned_mask"] = trainer.prune_lowest(res["importance"], res["head_mask"], opt.prune_heads)
            except ValueError as e:
                raise SystemExit("--prune_heads: %s" % e)
        with open(opt.head_importance, "w") as fp:
            json.dump(res, fp)
            fp.write("\n")
        print("head importance of %d utterances in %.2f s -> %s" % (res["utterances"], time.time() - t0, opt.head_importance), flush=True)
        return 0

    if opt.predict is not None:
        model.load_model(os.path.join(opt.exp_dir, "model.pt"))
        if opt.lora_adapter is not None:
            apply_lora_adapter(model, opt.lora_adapter)
        out_path = predict_output_path(opt)
        t0 = time.time()
        attn_fp = open(opt.predict_attention, "w") if opt.predict_attention else None
        attr_fp = open(opt.predict_attribution, "w") if opt.predict_attribution else None
        roll_fp = open(opt.predict_rollout, "w") if opt.predict_rollout else None
        token_keep = None
        if opt.token_keep is not None:
            try:
                token_keep = trainer.parse_token_keep(opt.token_keep, cfg.num_hidden_layers)
            except ValueError as e:
                raise SystemExit("--token_keep %s: %s" % (opt.token_keep, e))
        tok_fp = open(opt.predict_tokens, "w") if opt.predict_tokens else None
        try:
            cases = trainer.predict_split(model, trainer.read_predict_data(opt.predict), opt, memory, attn_fp=attn_fp, attr_fp=attr_fp,
                                          attr_steps=opt.attribution_steps, fp8=opt.predict_fp8, calib_batches=opt.fp8_calib_batches,
                                          rollout_fp=roll_fp, rollout_residual=opt.rollout_residual,
                                          **({} if token_keep is None else dict(token_keep=token_keep, tokens_fp=tok_fp)))
        finally:
            for fp in (attn_fp, attr_fp, roll_fp, tok_fp):
                if fp is not None:
                    fp.close()
        with open(out_path, "w") as fp:
            for raw, pc in cases:
                fp.write("%s\t<=>\t%s\n" % (" ".join(raw), ";".join(pc)))
        print("predicted %d utterances in %.2f s -> %s" % (len(cases), time.time() - t0, out_path), flush=True)
        return 0

    valid, test = load(opt.valid_file), load(opt.test_file)
    if opt.testing:
        model.load_model(os.path.join(opt.exp_dir, "model.pt"))
        if opt.lora_adapter is not None:
            apply_lora_adapter(model, opt.lora_adapter)
        log = _Log(os.path.join(opt.exp_dir, "log.test"), rank)
        for name, data in (("Train", load(opt.train_file)), ("Valid", valid), ("Test", test)):
            if data is None:
                continue
            with open(os.path.join(opt.exp_dir, "%s.eval" % name.lower()), "w") as fp, \
                    open(os.path.join(opt.exp_dir, "%s.eval.err" % name.lower()), "w") as efp:
                t0 = time.time()
                loss, (p, r, f), acc, _ = trainer.eval_epoch(model, data, opt, memory, fp, efp)
                log.info("[%s]\tTime: %.2f\tLoss: %.2f\t(p/r/f): (%.2f/%.2f/%.2f)\tAcc: %.2f" % (name, time.time() - t0, loss, p, r, f, acc))
        return 0

    train = load(opt.train_file, opt.coverage)
    if train is None:
        raise SystemExit("no training split at %s" % os.path.join(opt.dataroot, opt.train_file))
    t_total = (len(train) // opt.batchSize + 1) * opt.max_epoch            # n_best_asr_bert.py:556
    if opt.optim_choice == "bertadam":
        opt.optimizer = HipBertAdam(model, lr=opt.lr, bert_lr=opt.bert_lr, warmup=opt.warmup_proportion, t_total=t_total,
                                    shard=opt.shard_optimizer == "on", ema_decay=opt.ema_decay, lora_lr=opt.lora_lr)
    else:                                                                   # n_best_asr_bert.py:551-569
        opt.optimizer = HipAdam(model, kind=opt.optim_choice, lr=opt.lr, bert_lr=opt.bert_lr, l2=opt.l2, warmup=opt.warmup_proportion,
                                t_total=t_total, max_grad_norm=opt.max_norm, shard=opt.shard_optimizer == "on", ema_decay=opt.ema_decay)
    opt.scheduler = getattr(opt.optimizer, "scheduler", None)
    log = _Log(os.path.join(opt.exp_dir, "log.train"), rank, append=opt.resume and os.path.exists(os.path.join(opt.exp_dir, "last.pt")))
    t_start = time.time()
    log.info("Training starts at %s" % time.asctime(time.localtime(t_start)))
    if teacher is not None:
        log.info("Distillation: teacher %s (%d layers), alpha %s%s; gradient of (1 - alpha) * hard + alpha * soft, Loss below is the hard loss"
                 % (opt.distill_from, teacher.cfg.num_hidden_layers, opt.distill_alpha,
                    "" if opt.distill_temperature is None else ", temperature %s (teacher logits, soft = T^2 x the tempered terms)"
                    % opt.distill_temperature))
    if opt.rdrop_alpha is not None:
        log.info("R-Drop: alpha %s; every utterance twice per step under independent dropout bits, gradient of the hard loss of both "
                 "copies + alpha * their symmetric KL, Loss below is half the hard loss of the doubled batch" % opt.rdrop_alpha)
    if opt.adv_epsilon is not None:
        log.info("FGM: epsilon %s; every step runs the ASR pass again on word embeddings moved by epsilon (L2 norm per utterance) along "
                 "the loss gradient, same dropout bits, one optimizer step on the sum of both gradients, Loss and F1 below are the clean "
                 "pass's" % opt.adv_epsilon)
    if opt.contrastive_weight is not None:
        log.info("Contrastive: weight %s, temperature %s; every step runs the transcript pass and adds weight x the in-batch symmetric "
                 "InfoNCE between the ASR and the transcript CLS rows (identical transcripts are no negatives), Loss below stays the hard "
                 "loss (+ MSE)" % (opt.contrastive_weight, opt.contrastive_temperature))
    if opt.sam_rho is not None:
        log.info("%s: rho %s%s; every step takes the gradient at w + e (e along the first pass's gradient, same dropout bits) and "
                 "applies it at w, Loss and F1 below are the first pass's"
                 % ("ASAM" if opt.sam_adaptive else "SAM", opt.sam_rho, ", eta %s" % opt.sam_eta if opt.sam_adaptive else ""))
    if train_mask is not None:
        log.info("Head mask: %s (digest %s), heads kept per layer %s of %d; every step and every evaluation run under it, a pruned "
                 "head's weights get a zero gradient, model.pt keeps the full tensors (evaluate with --testing --head_mask)"
                 % (opt.train_head_mask, trainer.head_mask_digest(train_mask), [sum(1 for x in r if x != 0.0) for r in train_mask],
                    cfg.num_attention_heads))
    if lora_cfg is not None:
        log.info("LoRA: rank %d, alpha %g, targets %s, lr %s; %d trainable parameters (%d in the factors of %d blocks + the STC heads), "
                 "the encoder's own tensors are frozen; model.pt holds the merged weights, lora.pt the factors and heads"
                 % (opt.lora_rank, opt.lora_alpha, opt.lora_targets, opt.lora_lr, n_params, model.lora.n_trainable, len(model.lora.blocks)))
    if opt.ema_decay is not None:
        log.info("Weight EMA: decay %s (warm-up min(D, (1 + t) / (10 + t))); evaluation and model.pt use the averaged weights" % opt.ema_decay)
    best = dict(epoch=0, vf=0.0, tef=0.0, v_acc=0.0, te_acc=0.0)
    first_epoch, last = 0, os.path.join(opt.exp_dir, "last.pt")
    if opt.resume and os.path.exists(last):
        ck = torch.load(last, map_location="cpu", weights_only=True)           # written by this program: tensors + numbers
        if ck.get("head_mask") != train_mask:
            said = lambda m: "without a head mask" if m is None else "under the head mask %s" % trainer.head_mask_digest(m)
            raise SystemExit("--resume from %s: the checkpoint was trained %s, this run trains %s; resume with the --train_head_mask "
                             "it was started with" % (last, said(ck.get("head_mask")), said(train_mask)))
        from . import lora as _lora
        have = ck.get("lora")
        want = None if lora_cfg is None else model.lora.config()
        if (None if have is None else have["config"]) != want:
            said = lambda c: "without LoRA" if c is None else "with LoRA %s" % (c,)
            raise SystemExit("--resume from %s: the checkpoint was trained %s, this run trains %s; resume with the --lora_* flags it "
                             "was started with" % (last, said(None if have is None else have["config"]), said(want)))
        if lora_cfg is not None:
            model.disable_lora()
        model.load_reference_state(ck["model"])
        if lora_cfg is not None:                                               # the merged weights are in: put base and factors back
            model.enable_lora(**lora_cfg)
            _lora.restore_checkpoint(model, have)
        try:
            opt.optimizer.load_state_dict(ck["optimizer"])
        except ValueError as e:
            raise SystemExit("--resume from %s: %s" % (last, e))
        best, first_epoch = ck["best"], ck["epoch"] + 1
        model.step_counter = int(ck["dropout_step"])                           # dropout streams continue where they stopped
        log.info("Resumed after epoch %02d (optimizer step %d)" % (ck["epoch"], opt.optimizer.step_count))
    for ep in range(first_epoch, opt.max_epoch):
        t0 = time.time()
        loss, (p, r, f), acc = trainer.train_epoch(model, train, opt, memory, epoch=ep)
        log.info("[Train]\tEpoch: %02d\tTime: %.2f\tLoss: %.2f\t(p/r/f): (%.2f/%.2f/%.2f)\tAcc: %.2f" % (ep, time.time() - t0, loss, p, r, f, acc))
        if opt.contrastive_weight is not None and getattr(opt, "contrast_epoch", None):
            csum, chits, crows = opt.contrast_epoch[:3]
            log.info("[Contrast]\tEpoch: %02d\tLoss: %.4f\tAlign: %.2f" % (ep, csum / max(crows, 1.0), 100.0 * chits / max(crows, 1.0)))
        if opt.sam_rho is not None and getattr(opt, "sam_epoch", None):
            ssum, snorm, sutts, ssteps = opt.sam_epoch[:4]
            log.info("[SAM]\tEpoch: %02d\tSharpness: %.4f\tGradNorm: %.4f" % (ep, ssum / max(sutts, 1.0), snorm / max(ssteps, 1.0)))
        # --ema_decay: the evaluations and the model.pt write run on the averaged weights; the raw ones are back afterwards
        with (opt.optimizer.ema_weights() if opt.ema_decay is not None else contextlib.nullcontext()):
            res = {}
            for name, data in (("valid", valid), ("test", test)):
                if data is None:
                    continue
                fn = os.path.join(opt.exp_dir, "%s.iter%d" % (name, ep))
                with (open(fn, "w") if rank == 0 else open(os.devnull, "w")) as fp, \
                        (open(fn + ".err", "w") if rank == 0 else open(os.devnull, "w")) as efp:
                    t0 = time.time()
                    loss, (p, r, f), acc, cases = trainer.eval_epoch(model, data, opt, memory, fp, efp)
                log.info("[%s]\tEpoch: %02d\tTime: %.2f\tLoss: %.2f\t(p/r/f): (%.2f/%.2f/%.2f)\tAcc: %.2f" % (
                    name.capitalize(), ep, time.time() - t0, loss, p, r, f, acc))
                if rank == 0:                                                           # n_best_asr_bert.py:416,426
                    observe.observability_lens(observe.EpochInfoCollector.from_cases(cases, loss, (p, r, f), acc), ep, name,
                                               opt.exp_dir, "tod_asr_bert_stc")
                res[name] = (f, acc)
            vf, v_acc = res.get("valid", (0.0, 0.0))
            tef, te_acc = res.get("test", (0.0, 0.0))
            if vf > best["vf"]:
                best.update(epoch=ep, vf=vf, tef=tef, v_acc=v_acc, te_acc=te_acc)
                # sharded optimizer: the fp32 master is current only on each range's owner.  gather_master is a sequence of
                # collectives: EVERY rank runs it (vf is the all-reduced F1, so every rank takes this branch together); only
                # the file write is rank 0's
                opt.optimizer.gather_master(moments=False)
                if rank == 0:
                    model.save_model(os.path.join(opt.exp_dir, "model.pt"))
                    if model.lora is not None:
                        torch.save(model.lora_state_dict(), os.path.join(opt.exp_dir, "lora.pt"))
                log.info("NEW BEST:\tEpoch: %02d\tvalid F1/Acc: %.2f/%.2f\ttest F1/Acc: %.2f/%.2f" % (ep, vf, v_acc, tef, te_acc))
        if opt.resume:
            opt.optimizer.gather_master()           # all ranks (collectives); master and moments are whole everywhere afterwards
            if rank == 0:                           # ... so the state dicts are built AFTER the gather, on rank 0 only
                torch.save(dict(model={k: v.detach().cpu() for k, v in model.state_dict().items()},
                                optimizer=opt.optimizer.state_dict(gather=False), best=best, epoch=ep, dropout_step=model.step_counter,
                                **({} if train_mask is None else dict(head_mask=train_mask)),
                                **({} if model.lora is None else dict(lora=_lora_checkpoint(model)))),
                           last + ".tmp")
                os.replace(last + ".tmp", last)
        if opt.stop_after_epoch is not None and ep >= opt.stop_after_epoch:
            log.info("Stopping after epoch %02d as requested" % ep)
            return 0
    log.info("Done training. Elapsed time: %s" % timedelta(seconds=time.time() - t_start))
    log.info("BEST RESULT:\tEpoch: %02d\tBest valid F1/Acc: %.2f/%.2f\ttest F1/Acc: %.2f/%.2f" % (
        best["epoch"], best["vf"], best["v_acc"], best["tef"], best["te_acc"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
