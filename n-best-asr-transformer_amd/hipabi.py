"""ctypes binding of the C-ABI library ``csrc/libnbest_hip.so`` (declared in include/nbest_hip.h).

PyTorch is used only for device memory and streams: every wrapper passes ``tensor.data_ptr()`` and
the current HIP stream handle.  There is NO fallback: if the library is missing or an entry point
fails, a RuntimeError is raised (the product path must never silently run on the CPU).
"""
import collections
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NBEST_LIB") or os.path.join(_HERE, "csrc", "libnbest_hip.so")   # NBEST_LIB: another build of the library - how one GPU run times the parent commit's library against this one, alternating

F32, BF16 = 0, 1
ADAM_L2, ADAMW = 0, 1          # include/nbest_hip.h NBEST_ADAM_L2 / NBEST_ADAMW
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RES, EPI_DGELU, EPI_RES, EPI_F32_SPLITK = range(7)
EPI_BIAS_GELU_Q8 = 7           # nbest_gemm_fp8 only: the e4m3 copy of gelu(u) and nothing else (the FFN-up of the fp8 inference)

EXPORTS = [
    "nbest_version", "nbest_last_error", "nbest_embed_ln_fwd", "nbest_embed_ln_bwd", "nbest_embed_bwd_ws_bytes", "nbest_rows_gather", "nbest_rows_zero", "nbest_rows_add",
    "nbest_gemm_ws_bytes", "nbest_gemm", "nbest_gemm_plan", "nbest_wgrad_pair_ws_bytes", "nbest_wgrad_pair", "nbest_wgrad_group", "nbest_wgrad_window", "nbest_pack_bn", "nbest_pack_weights", "nbest_pack_bn_fp8", "nbest_pack_weights_fp8", "nbest_attention_fwd", "nbest_attention_bwd", "nbest_attention_bwd_ws_bytes", "nbest_attention_keep_bytes", "nbest_attention_fwd_keep", "nbest_attention_bwd_keep", "nbest_layernorm_fwd",
    "nbest_layernorm_bwd", "nbest_rowred_ws_bytes", "nbest_colsum", "nbest_heads_ws_bytes", "nbest_stc_heads", "nbest_stc_heads_kd", "nbest_stc_heads_kd_t", "nbest_stc_heads_logits", "nbest_stc_heads_rdrop",
    "nbest_stc_heads_vjp", "nbest_cls_mse", "nbest_cls_contrast_ws_bytes", "nbest_cls_contrast", "nbest_cls_grad_scatter", "nbest_stc_decode", "nbest_stream_stamp", "nbest_fp8_amax_fold", "nbest_bertadam_chunk", "nbest_bertadam_step", "nbest_bertadam_norms", "nbest_bertadam_update",
    "nbest_adam_clip_coef", "nbest_adam_update", "nbest_adam_step", "nbest_ema_update", "nbest_ema_exchange", "nbest_sam_norms", "nbest_sam_perturb", "nbest_sam_restore",
    "nbest_cast_f32_to_bf16", "nbest_transpose_weights", "nbest_encoder_act_bytes", "nbest_encoder_ws_bytes", "nbest_encoder_wgrad_launches_per_layer", "nbest_encoder_wgrad_plan", "nbest_encoder_forward",
    "nbest_encoder_backward", "nbest_gemm_fp8", "nbest_gemm_fp8_ws_bytes", "nbest_wgrad_fp8", "nbest_wgrad_fp8_ws_bytes", "nbest_wgrad_fp8_pair", "nbest_wgrad_fp8_pair_ws_bytes", "nbest_cast_bf16_to_fp8", "nbest_quantize_weights_fp8",
    "nbest_attention_cls_fwd", "nbest_encoder_infer_ws_bytes", "nbest_encoder_infer",
    "nbest_attention_probs", "nbest_attention_cls_probs", "nbest_encoder_act_view", "nbest_encoder_infer_attn",
    "nbest_embed_ln_fwd_interp", "nbest_embed_attrib",
    "nbest_head_gate_fwd", "nbest_head_gate_bwd",
    "nbest_head_prune_plan", "nbest_head_prune_pack", "nbest_encoder_infer_pruned",
    "nbest_embed_ln_fwd_adv", "nbest_embed_ln_bwd_adv", "nbest_embed_adv_ws_bytes", "nbest_embed_adv_delta",
    "nbest_layernorm_fwd_fp8", "nbest_layernorm_bwd_fp8", "nbest_attention_fwd_fp8", "nbest_attention_bwd_fp8", "nbest_cast_bf16_to_fp8_scaled", "nbest_amax_bf16",
    "nbest_gemm_fp8_plan", "nbest_wgrad_fp8_plan",
    "nbest_fp8_amax_fold_max", "nbest_encoder_infer_fp8_ws_bytes", "nbest_encoder_infer_fp8",
    "nbest_attention_rollout_step",
    "nbest_token_select", "nbest_rows_compact", "nbest_encoder_infer_tokens_ws_bytes", "nbest_encoder_infer_tokens",
    "nbest_lora_plan", "nbest_lora_grad_ws_bytes", "nbest_lora_merge", "nbest_lora_grad",
]


class GemmArgs(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p),
                ("U", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
                ("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64), ("ldr", C.c_int64), ("ldu", C.c_int64),
                ("trans_a", C.c_int32), ("trans_b", C.c_int32), ("epilogue", C.c_int32), ("dtype", C.c_int32),
                ("accumulate", C.c_int32), ("drop_p", C.c_float), ("drop_stream", C.c_uint32), ("seed", C.c_uint64),
                ("colsum_out", C.c_void_p), ("colsum_accumulate", C.c_int32), ("flags", C.c_int32),
                ("B_packed", C.c_void_p), ("b_pack_bn", C.c_int32), ("pad_", C.c_int32)]


class GemmPlanInfo(C.Structure):
    _fields_ = [("generation", C.c_int32), ("bm", C.c_int32), ("bn", C.c_int32), ("bk", C.c_int32),
                ("wave_rows", C.c_int32), ("wave_cols", C.c_int32), ("stages", C.c_int32), ("form", C.c_int32),
                ("reg_epilogue", C.c_int32), ("splits", C.c_int32), ("k_per_split", C.c_int64),
                ("b_packed", C.c_int32), ("kernel_epilogue", C.c_int32)]


class GemmFp8Args(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p), ("U", C.c_void_p),
                ("C8", C.c_void_p), ("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64), ("ldr", C.c_int64), ("ldu", C.c_int64), ("ldc8", C.c_int64),
                ("epilogue", C.c_int32), ("out_scale", C.c_float), ("drop_p", C.c_float), ("drop_stream", C.c_uint32), ("seed", C.c_uint64),
                ("out_scale_dev", C.c_void_p), ("a_amax", C.c_void_p), ("c8_amax_prev", C.c_void_p), ("c8_amax_new", C.c_void_p),
                ("colsum_out", C.c_void_p), ("colsum_accumulate", C.c_int32), ("pad", C.c_int32), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
                ("B_packed", C.c_void_p), ("b_pack_bn", C.c_int32), ("pad3", C.c_int32)]


class GemmFp8PlanInfo(C.Structure):
    _fields_ = [("bn", C.c_int32), ("stages", C.c_int32), ("tiles_m", C.c_int32), ("tiles_n", C.c_int32), ("group_cols", C.c_int32),
                ("packed_taken", C.c_int32)]


class LabelSpaceC(C.Structure):
    _fields_ = [("n_top", C.c_int32), ("n_bottom", C.c_int32), ("n_rows", C.c_int32),
                ("bottom_off", C.c_void_p), ("bottom_ids", C.c_void_p), ("head_row", C.c_void_p)]


class TensorDesc(C.Structure):
    _fields_ = [("offset", C.c_int64), ("numel", C.c_int64), ("lr", C.c_float), ("wd", C.c_float),
                ("active", C.c_int32), ("block_start", C.c_int32)]


class MatrixDesc(C.Structure):
    _fields_ = [("offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("tile_start", C.c_int32), ("pad", C.c_int32)]


LORA_MAX_RANK = 64             # include/nbest_hip.h NBEST_LORA_MAX_RANK


class LoraDesc(C.Structure):
    """nbest_lora_desc: one adapted block (a contiguous row range of one arena matrix); tile_start / ws_off are nbest_lora_plan's"""
    _fields_ = [("p_off", C.c_int64), ("base_off", C.c_int64), ("a_off", C.c_int64), ("b_off", C.c_int64), ("ws_off", C.c_int64),
                ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32), ("rank", C.c_int32),
                ("scale", C.c_float), ("tile_start", C.c_int32)]


HEAD_PRUNE_MAX_HEADS = 32      # include/nbest_hip.h NBEST_HEAD_PRUNE_MAX_HEADS


class HeadPruneLayer(C.Structure):
    """nbest_head_prune_layer: a layer's row of the compact-heads table (element offsets in the arenas / in the images, k, idx)"""
    _fields_ = [("src_wqkv", C.c_int64), ("src_bqkv", C.c_int64), ("src_wo", C.c_int64),
                ("dst_wqkv", C.c_int64), ("dst_bqkv", C.c_int64), ("dst_wo", C.c_int64),
                ("k", C.c_int32), ("pad", C.c_int32), ("idx", C.c_int32 * HEAD_PRUNE_MAX_HEADS)]


class HeadPruneImages(C.Structure):
    _fields_ = [("w", C.c_void_p), ("w_packed", C.c_void_p), ("bqkv", C.c_void_p), ("layers_host", C.POINTER(HeadPruneLayer))]


class LayerOffsets(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("wqkv", "bqkv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2", "ln2_g", "ln2_b")]


class EncoderDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("L", C.c_int32),
                ("heads", C.c_int32), ("F", C.c_int32), ("vocab", C.c_int32), ("max_pos", C.c_int32), ("n_types", C.c_int32),
                ("ln_eps", C.c_float), ("hidden_drop", C.c_float), ("attn_drop", C.c_float),
                ("word_pad_id", C.c_int64), ("pos_pad_id", C.c_int64),
                ("off_word", C.c_int64), ("off_pos", C.c_int64), ("off_type", C.c_int64),
                ("off_emb_ln_g", C.c_int64), ("off_emb_ln_b", C.c_int64),
                ("layers_host", C.POINTER(LayerOffsets)), ("seed", C.c_uint64), ("drop_stream_base", C.c_uint32),
                ("wgrad_events_n", C.c_int32), ("wgrad_events", C.POINTER(C.c_void_p)),
                ("w8", C.c_void_p), ("w8_inv_scale", C.c_void_p), ("w8t", C.c_void_p), ("gamax_prev", C.c_void_p),
                ("gamax_new", C.c_void_p), ("fp8_bwd", C.c_int32), ("head_gate_stash", C.c_int32),
                ("wpk", C.c_void_p), ("wpkt", C.c_void_p), ("w8p", C.c_void_p), ("w8tp", C.c_void_p),
                ("word_perm", C.c_void_p), ("aamax_prev", C.c_void_p), ("aamax_new", C.c_void_p), ("fp8_act", C.c_int32), ("cls_top", C.c_int32),
                ("first_trainable", C.c_int32), ("no_input_grad", C.c_int32), ("emb_delta", C.c_void_p), ("wgrad_skip_host", C.c_void_p),
                ("head_gate", C.c_void_p), ("head_gate_grad", C.c_void_p),
                ("base_ids", C.c_void_p), ("alpha", C.c_void_p), ("no_param_grad", C.c_int32), ("pad5", C.c_int32)]
    # nbest_encoder_desc.wgrad_group (WGRAD_GROUP_*): the descriptor's last field, in the slot that was padding
    wgrad_group = property(lambda self: self.pad5, lambda self, v: setattr(self, "pad5", int(v)))


_lib = None


def lib():
    """Load the library once; fail loudly when it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("nbest_amd: %s is missing - build it with `make -C %s` (hipcc, gfx950). "
                               "There is no CPU fallback for the product path." % (LIB_PATH, os.path.dirname(LIB_PATH)))
        L = C.CDLL(LIB_PATH)
        for name in EXPORTS:
            if not hasattr(L, name):
                raise RuntimeError("nbest_amd: %s does not export %s" % (LIB_PATH, name))
        for name in ("nbest_embed_bwd_ws_bytes", "nbest_gemm_ws_bytes", "nbest_wgrad_pair_ws_bytes", "nbest_rowred_ws_bytes", "nbest_heads_ws_bytes",
                     "nbest_attention_bwd_ws_bytes", "nbest_attention_keep_bytes", "nbest_embed_adv_ws_bytes", "nbest_cls_contrast_ws_bytes",
                     "nbest_encoder_act_bytes", "nbest_encoder_ws_bytes", "nbest_encoder_infer_ws_bytes", "nbest_encoder_infer_fp8_ws_bytes",
                     "nbest_encoder_infer_tokens_ws_bytes"):
            getattr(L, name).restype = C.c_size_t
        L.nbest_embed_bwd_ws_bytes.argtypes = [C.c_int64, C.c_int64]
        L.nbest_rows_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.nbest_rows_zero.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.nbest_rows_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.nbest_rowred_ws_bytes.argtypes = [C.c_int64, C.c_int64]
        L.nbest_heads_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.nbest_gemm_ws_bytes.argtypes = [C.POINTER(GemmArgs)]
        L.nbest_gemm.argtypes = [C.POINTER(GemmArgs), C.c_void_p]
        L.nbest_gemm_plan.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmPlanInfo)]
        L.nbest_wgrad_pair_ws_bytes.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmArgs)]
        L.nbest_wgrad_pair.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmArgs), C.c_void_p]
        L.nbest_wgrad_group.argtypes = [C.POINTER(GemmArgs), C.c_int32, C.c_void_p]
        L.nbest_wgrad_window.argtypes = [C.POINTER(GemmArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p]
        L.nbest_encoder_act_bytes.argtypes = [C.POINTER(EncoderDesc)]
        L.nbest_encoder_ws_bytes.argtypes = [C.POINTER(EncoderDesc)]
        L.nbest_encoder_wgrad_launches_per_layer.argtypes = [C.POINTER(EncoderDesc)]
        L.nbest_encoder_wgrad_plan.argtypes = [C.POINTER(EncoderDesc), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        vp, i64, i32, f32, u64, u32, sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_uint64, C.c_uint32, C.c_size_t
        L.nbest_embed_ln_fwd.argtypes = [vp] * 10 + [i64, i32, f32, i32, f32, u64, u32, vp]
        L.nbest_embed_ln_bwd.argtypes = [vp] * 15 + [i32, i32, i32, i32, i32, i64, i64, i32, i32, f32, u64, u32, vp, sz, vp]
        L.nbest_embed_ln_fwd_interp.argtypes = [vp] * 12 + [i32, i32, i32, f32, i32, f32, u64, u32, vp]
        L.nbest_embed_attrib.argtypes = [vp] * 11 + [i32, i32, i32, i32, f32, i32, vp]
        L.nbest_embed_ln_fwd_adv.argtypes = [vp] * 11 + [i64, i32, f32, i32, f32, u64, u32, vp]
        L.nbest_embed_ln_bwd_adv.argtypes = [vp] * 16 + [i32, i32, i32, i32, i32, i64, i64, i32, i32, f32, u64, u32, vp, sz, vp]
        L.nbest_embed_adv_ws_bytes.argtypes = [i32, i32]
        L.nbest_embed_adv_delta.argtypes = [vp] * 11 + [i32, i32, i32, f32, i32, f32, u64, u32, f32, vp, sz, vp]
        L.nbest_head_gate_fwd.argtypes = [vp, i64, vp, i64, vp, i64, i32, i32, i32, vp]
        L.nbest_head_gate_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
        L.nbest_attention_fwd.argtypes = [vp] * 4 + [i32] * 5 + [f32, u64, u32, vp]
        L.nbest_attention_bwd.argtypes = [vp] * 7 + [i32, vp, sz] + [i32] * 5 + [f32, u64, u32, vp]
        L.nbest_attention_bwd_ws_bytes.argtypes = [i32, i32, i32]
        L.nbest_attention_keep_bytes.argtypes = [i32, i32, i32]
        L.nbest_attention_fwd_keep.argtypes = [vp] * 4 + [i32] * 5 + [f32, u64, u32, vp, vp]
        L.nbest_attention_bwd_keep.argtypes = [vp] * 7 + [i32, vp, sz] + [i32] * 5 + [f32, u64, u32, vp, vp]
        L.nbest_attention_fwd_fp8.argtypes = [vp] * 5 + [i32] * 5 + [f32, u64, u32, vp, vp, vp, vp]
        L.nbest_attention_bwd_fp8.argtypes = [vp] * 7 + [i32, vp, sz] + [i32] * 5 + [f32, u64, u32, vp, vp, vp, vp, vp]
        L.nbest_layernorm_fwd_fp8.argtypes = [vp] * 6 + [i64, i32, f32, i32, vp, vp, vp]
        L.nbest_layernorm_bwd_fp8.argtypes = [vp] * 9 + [i64, i32, i32, i32, f32, u64, u32, vp, sz, vp, vp, vp, vp]
        L.nbest_cast_bf16_to_fp8_scaled.argtypes = [vp, vp, i64, vp, vp, vp]
        L.nbest_amax_bf16.argtypes = [vp, i64, vp, vp]
        L.nbest_layernorm_fwd.argtypes = [vp] * 5 + [i64, i32, f32, i32, vp]
        L.nbest_layernorm_bwd.argtypes = [vp] * 9 + [i64, i32, i32, i32, f32, u64, u32, vp, sz, vp]
        L.nbest_colsum.argtypes = [vp, vp, i64, i64, i64, i32, i32, vp, sz, vp]
        L.nbest_stc_heads.argtypes = [vp, i64, vp, vp, C.POINTER(LabelSpaceC)] + [vp] * 8 + [i32] * 5 + [f32, u64, u32, vp, sz, vp]
        L.nbest_stc_heads_kd.argtypes = [vp, i64, vp, vp, C.POINTER(LabelSpaceC)] + [vp] * 4 + [f32] + [vp] * 7 + [i32] * 5 + [f32, u64, u32, vp, sz, vp]
        L.nbest_stc_heads_kd_t.argtypes = [vp, i64, vp, vp, C.POINTER(LabelSpaceC)] + [vp] * 2 + [f32, f32] + [vp] * 7 + [i32] * 5 + [f32, u64, u32, vp, sz, vp]
        L.nbest_stc_heads_rdrop.argtypes = [vp, i64, vp, vp, C.POINTER(LabelSpaceC), vp, f32] + [vp] * 7 + [i32] * 5 + [f32, u64, u32, vp, sz, vp]
        L.nbest_stc_heads_logits.argtypes = [vp, i64, vp, vp, C.POINTER(LabelSpaceC), vp, i32, i32, i32, vp]
        L.nbest_stc_heads_vjp.argtypes = [vp, C.POINTER(LabelSpaceC)] + [vp] * 8 + [i32, i32, i32, f32, u64, u32, vp, sz, vp]
        L.nbest_cls_mse.argtypes = [vp, i64, vp, i64, vp, vp, vp, i32, i32, i32, f32, vp]
        L.nbest_cls_contrast_ws_bytes.argtypes = [i32, i32]
        L.nbest_cls_contrast.argtypes = [vp, i64, vp, i64, vp, f32, f32, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]
        L.nbest_cls_grad_scatter.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        L.nbest_stc_decode.argtypes = [vp, vp, C.POINTER(LabelSpaceC), vp, vp, i32, vp]
        L.nbest_stream_stamp.argtypes = [vp, i32, vp]
        L.nbest_fp8_amax_fold.argtypes = [vp, vp, i32, vp]
        L.nbest_fp8_amax_fold_max.argtypes = [vp, vp, i32, vp]
        f64 = C.c_double                  # b1, b2 of every optimizer: the library forms (float)b and (float)(1 - b) itself
        L.nbest_bertadam_step.argtypes = [vp] * 6 + [i32, i32, f32, f64, f64, f32, f32, vp, sz, vp]
        L.nbest_bertadam_norms.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
        L.nbest_bertadam_update.argtypes = [vp] * 6 + [i32, i32, i32, i32, vp, vp, f32, f64, f64, f32, f32, vp]
        L.nbest_adam_clip_coef.argtypes = [vp, i32, f32, vp, vp]
        L.nbest_adam_update.argtypes = [i32] + [vp] * 6 + [i32, i32, i32, i32, vp, f32, f32, f32, f64, f64, f32, vp]
        L.nbest_adam_step.argtypes = [i32] + [vp] * 6 + [i32, i32, f32, f32, f32, f64, f64, f32, f32, vp, sz, vp]
        L.nbest_ema_update.argtypes = [vp, vp, vp, i32, i32, f32, vp]
        L.nbest_ema_exchange.argtypes = [vp, vp, vp, vp, i32, i32, vp]
        L.nbest_sam_norms.argtypes = [vp, vp, vp, i32, i32, f32, vp, vp]
        L.nbest_sam_perturb.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, f32, f32, vp]
        L.nbest_sam_restore.argtypes = [vp, vp, vp, vp, i32, i32, vp]
        L.nbest_cast_f32_to_bf16.argtypes = [vp, vp, i64, vp]
        L.nbest_encoder_forward.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 7 + [sz, vp, sz, C.POINTER(C.c_void_p), vp]
        L.nbest_encoder_infer_ws_bytes.argtypes = [C.POINTER(EncoderDesc)]
        L.nbest_encoder_infer.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 7 + [sz, vp, vp]
        L.nbest_encoder_infer_fp8_ws_bytes.argtypes = [C.POINTER(EncoderDesc)]
        L.nbest_encoder_infer_fp8.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 7 + [sz, vp, vp]
        L.nbest_attention_cls_fwd.argtypes = [vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp]
        L.nbest_encoder_infer_attn.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 7 + [sz, vp, vp, vp]
        L.nbest_head_prune_plan.argtypes = [C.POINTER(C.c_int32), i32, i32, i32, C.POINTER(HeadPruneLayer)] + [C.POINTER(C.c_size_t)] * 3
        L.nbest_head_prune_pack.argtypes = [vp, vp, vp, C.POINTER(HeadPruneLayer), vp, i32, i32, i32, vp, sz, vp, sz, vp]
        L.nbest_encoder_infer_pruned.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 7 + [sz, vp, C.POINTER(HeadPruneImages), vp]
        L.nbest_encoder_act_view.argtypes = [C.POINTER(EncoderDesc), vp, i32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.nbest_attention_probs.argtypes = [vp] * 4 + [i32] * 5 + [vp]
        L.nbest_attention_cls_probs.argtypes = [vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp]
        L.nbest_attention_rollout_step.argtypes = [vp] * 5 + [f32] + [i32] * 5 + [vp]
        L.nbest_token_select.argtypes = [vp] * 3 + [i32] + [vp] * 4 + [i32, i32, vp]
        L.nbest_rows_compact.argtypes = [vp] * 3 + [i32] * 5 + [vp]
        L.nbest_encoder_infer_tokens_ws_bytes.argtypes = [C.POINTER(EncoderDesc)]
        L.nbest_encoder_infer_tokens.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 7 + [sz, vp, C.POINTER(C.c_int32), i32, vp, vp]
        L.nbest_encoder_backward.argtypes = [C.POINTER(EncoderDesc)] + [vp] * 9 + [sz, vp, vp, sz, i32, i32, i32, i32, vp]
        L.nbest_transpose_weights.argtypes = [vp, vp, vp, i32, i32, vp]
        L.nbest_pack_bn.argtypes = [i64]
        L.nbest_pack_weights.argtypes = [vp, vp, vp, i32, i32, vp]
        L.nbest_pack_bn_fp8.argtypes = [i64, i64]
        L.nbest_pack_weights_fp8.argtypes = [vp, vp, vp, i32, i32, vp]
        L.nbest_gemm_fp8.argtypes = [C.POINTER(GemmFp8Args), vp]
        L.nbest_gemm_fp8_plan.argtypes = [C.POINTER(GemmFp8Args), C.POINTER(GemmFp8PlanInfo)]
        L.nbest_wgrad_fp8_plan.argtypes = [i64, i64, i64, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
        L.nbest_cast_bf16_to_fp8.argtypes = [vp, vp, i64, vp]
        L.nbest_wgrad_fp8_ws_bytes.restype = C.c_size_t
        L.nbest_wgrad_fp8_ws_bytes.argtypes = [i64, i64, i64]
        L.nbest_wgrad_fp8.argtypes = [vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, i32, vp, sz, vp]
        L.nbest_wgrad_fp8_pair_ws_bytes.restype = C.c_size_t
        L.nbest_wgrad_fp8_pair_ws_bytes.argtypes = [i64, i64, i64, i64]
        L.nbest_wgrad_fp8_pair.argtypes = [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, i64, i64, i32, vp, sz, vp]
        L.nbest_quantize_weights_fp8.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]
        L.nbest_gemm_fp8_ws_bytes.restype = C.c_size_t
        L.nbest_gemm_fp8_ws_bytes.argtypes = [C.POINTER(GemmFp8Args)]
        L.nbest_lora_plan.argtypes = [C.POINTER(LoraDesc), i32, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        L.nbest_lora_grad_ws_bytes.restype = C.c_size_t
        L.nbest_lora_grad_ws_bytes.argtypes = [C.POINTER(LoraDesc), i32]
        L.nbest_lora_merge.argtypes = [vp, vp, vp, vp, C.POINTER(LoraDesc), vp, i32, vp]
        L.nbest_lora_grad.argtypes = [vp, vp, vp, C.POINTER(LoraDesc), vp, i32, vp, sz, vp]
        L.nbest_last_error.argtypes = [C.c_char_p, sz]
        _lib = L
    return _lib


def last_error():
    buf = C.create_string_buffer(512)
    lib().nbest_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc, what):
    if rc != 0:
        raise RuntimeError("nbest_hip %s failed (%d): %s" % (what, rc, last_error()))


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(t):
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise RuntimeError("nbest_amd: unsupported activation dtype %s" % t)


def ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------
# thin per-op wrappers (used by the kernel parity tests; training goes through encoder_forward/backward)
# ------------------------------------------------------------------------------------------------
def gemm_prepared(A, B, M, N, K, out, trans_a=False, trans_b=False, epilogue=EPI_NONE, defer_reduce=False):
    """build the argument block + workspace ONCE and return a zero-overhead launcher (benchmark loops)"""
    g = GemmArgs()
    g.A, g.B, g.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = A.stride(0), B.stride(0), out.stride(0)
    g.trans_a, g.trans_b, g.epilogue, g.dtype = int(trans_a), int(trans_b), epilogue, dtype_code(A.dtype)
    g.flags = 1 if defer_reduce else 0
    ws = _ws(lib().nbest_gemm_ws_bytes(C.byref(g)), A.device)
    g.ws, g.ws_bytes = ws.data_ptr(), ws.numel()
    fn, ref, st = lib().nbest_gemm, C.byref(g), stream_ptr()

    def launch():
        rc = fn(ref, st)
        if rc:
            check(rc, "gemm")
    launch.keepalive = (g, ws, A, B, out)
    return launch


def pack_weight(W):
    """W [N, K] bf16 (k-contiguous) -> (packed copy, tile width) for nbest_gemm_args::B_packed, or (None, 0) when the shape has no packed form"""
    N, K = W.shape
    bn = lib().nbest_pack_bn(N)
    if bn == 0 or K % 32 or N % bn:
        return None, 0
    d = (MatrixDesc * 1)()
    d[0].offset, d[0].rows, d[0].cols, d[0].tile_start, d[0].pad = 0, N, K, 0, bn
    dd = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(W.device)
    out = torch.empty_like(W)
    check(lib().nbest_pack_weights(ptr(W), ptr(out), ptr(dd), 1, (N // bn) * (K // 32), stream_ptr()), "pack_weights")
    return out, bn


def pack_weight_fp8(W8):
    """W8 [N, K] e4m3 bytes -> (packed copy, tile width) for nbest_gemm_fp8_args::B_packed"""
    N, K = W8.shape
    bn = lib().nbest_pack_bn_fp8(N, K)
    if bn == 0 or K % 64 or N % bn:
        return None, 0
    d = (MatrixDesc * 1)()
    d[0].offset, d[0].rows, d[0].cols, d[0].tile_start, d[0].pad = 0, N, K, 0, bn
    dd = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(W8.device)
    out = torch.empty_like(W8)
    check(lib().nbest_pack_weights_fp8(ptr(W8), ptr(out), ptr(dd), 1, (N // bn) * (K // 64), stream_ptr()), "pack_weights_fp8")
    return out, bn


def _gemm_args(A, B, M, N, K, trans_a, trans_b, epilogue, bias, R, U, out, accumulate, drop_p, seed, drop_stream, colsum_out,
               defer_reduce, B_packed, b_pack_bn, want_u):
    """the argument block of gemm / gemm_plan with its workspace: (GemmArgs, out, U, workspace)"""
    dt = dtype_code(A.dtype)
    dev = A.device
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if epilogue == EPI_F32_SPLITK else A.dtype, device=dev)
    if epilogue == EPI_BIAS_GELU and U is None and want_u:        # gelu'(u): float in the fp32 path, 8-bit fixed point in the bf16 path
        U = torch.empty(M, N, dtype=torch.float32 if A.dtype == torch.float32 else torch.uint8, device=dev)
    g = GemmArgs()
    g.A, g.B, g.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    g.bias = bias.data_ptr() if bias is not None else None
    g.R = R.data_ptr() if R is not None else None
    g.U = U.data_ptr() if U is not None else None
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = A.stride(0), B.stride(0), out.stride(0)
    g.ldr = R.stride(0) if R is not None else 0
    g.ldu = U.stride(0) if U is not None else 0
    g.trans_a, g.trans_b, g.epilogue, g.dtype = int(trans_a), int(trans_b), epilogue, dt
    g.accumulate, g.drop_p, g.drop_stream, g.seed = int(accumulate), drop_p, drop_stream, seed
    g.colsum_out = colsum_out.data_ptr() if colsum_out is not None else None
    g.flags = 1 if defer_reduce else 0
    if B_packed is not None:
        g.B_packed, g.b_pack_bn = B_packed.data_ptr(), b_pack_bn
    nb = lib().nbest_gemm_ws_bytes(C.byref(g))
    ws = _ws(nb, dev)
    g.ws, g.ws_bytes = ws.data_ptr(), ws.numel()
    return g, out, U, ws


def gemm(A, B, M, N, K, trans_a=False, trans_b=False, epilogue=EPI_NONE, bias=None, R=None, U=None, out=None,
         accumulate=False, drop_p=0.0, seed=0, drop_stream=0, colsum_out=None, defer_reduce=False, B_packed=None, b_pack_bn=0,
         want_u=True):
    """C[M,N] = epi(op(A) . op(B)); returns C (and U for EPI_BIAS_GELU; ``want_u=False``: C only, no GELU' rows written)."""
    g, out, U, ws = _gemm_args(A, B, M, N, K, trans_a, trans_b, epilogue, bias, R, U, out, accumulate, drop_p, seed, drop_stream,
                               colsum_out, defer_reduce, B_packed, b_pack_bn, want_u)
    check(lib().nbest_gemm(C.byref(g), stream_ptr()), "gemm")
    return (out, U) if epilogue == EPI_BIAS_GELU and want_u else out


FORM_NN, FORM_NT, FORM_TT, FORM_TN = range(4)                    # include/nbest_hip.h NBEST_GEMM_FORM_*
EPI_BIAS_GELU_NO_U = 0x102                                       # kernel_epilogue of EPI_BIAS_GELU with U = NULL


def gemm_plan_args(g):
    """nbest_gemm_plan on a filled GemmArgs: what nbest_gemm would launch (host only, nothing enqueued), as a dict of the
    nbest_gemm_plan_info fields; an argument block nbest_gemm refuses raises with the same code"""
    info = GemmPlanInfo()
    check(lib().nbest_gemm_plan(C.byref(g), C.byref(info)), "gemm_plan")
    return {name: int(getattr(info, name)) for name, _ in GemmPlanInfo._fields_}


def gemm_plan(A, B, M, N, K, trans_a=False, trans_b=False, epilogue=EPI_NONE, bias=None, R=None, U=None, out=None,
              accumulate=False, drop_p=0.0, seed=0, drop_stream=0, colsum_out=None, defer_reduce=False, B_packed=None, b_pack_bn=0,
              want_u=True):
    """the kernel ``gemm`` would launch for the same arguments (nbest_gemm_plan), as a dict; launches nothing"""
    g, out, U, ws = _gemm_args(A, B, M, N, K, trans_a, trans_b, epilogue, bias, R, U, out, accumulate, drop_p, seed, drop_stream,
                               colsum_out, defer_reduce, B_packed, b_pack_bn, want_u)
    return gemm_plan_args(g)


def gemm_plan_shape(M, N, K, trans_a=False, trans_b=False, epilogue=EPI_NONE, dtype=BF16, lda=None, ldb=None, ldc=None, ldr=None,
                    ldu=None, with_u=True, colsum=False, packed_bn=0, accumulate=False):
    """gemm_plan from a shape alone: the operands are stand-in addresses (the plan dereferences none), packed rows unless a leading
    dimension is given, every operand the epilogue reads present, the workspace as large as nbest_gemm_ws_bytes asks"""
    g = GemmArgs()
    fake = 1 << 20
    g.A, g.B, g.C = fake, fake, fake
    g.M, g.N, g.K = M, N, K
    g.lda = lda if lda is not None else (M if trans_a else K)
    g.ldb = ldb if ldb is not None else (N if trans_b else K)
    g.ldc = ldc if ldc is not None else N
    g.trans_a, g.trans_b, g.epilogue, g.dtype, g.accumulate = int(trans_a), int(trans_b), epilogue, dtype, int(accumulate)
    if epilogue in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RES):
        g.bias = fake
    if epilogue in (EPI_BIAS_DROP_RES, EPI_RES):
        g.R, g.ldr = fake, (ldr if ldr is not None else N)
    if epilogue == EPI_DGELU or (epilogue == EPI_BIAS_GELU and with_u):
        g.U, g.ldu = fake, (ldu if ldu is not None else N)
    if colsum:
        g.colsum_out = fake
    if packed_bn:
        g.B_packed, g.b_pack_bn = fake, packed_bn
    g.ws, g.ws_bytes = fake, max(int(lib().nbest_gemm_ws_bytes(C.byref(g))), 16)
    return gemm_plan_args(g)


def wgrad_pair(dY1, X1, dY2, X2, out1=None, out2=None, accumulate=False):
    """(dY1^T . X1, dY2^T . X2) in fp32 by ONE launch (nbest_wgrad_pair): dY_i [K, M_i], X_i [K, N] bf16, token-major"""
    K, N = X1.shape
    outs, gs = [], []
    for dY, X, out in ((dY1, X1, out1), (dY2, X2, out2)):
        M = dY.shape[1]
        if out is None:
            out = torch.empty(M, N, dtype=torch.float32, device=X.device)
        g = GemmArgs()
        g.A, g.B, g.C = dY.data_ptr(), X.data_ptr(), out.data_ptr()
        g.M, g.N, g.K = M, N, K
        g.lda, g.ldb, g.ldc = dY.stride(0), X.stride(0), out.stride(0)
        g.trans_a = g.trans_b = 1
        g.epilogue, g.dtype, g.accumulate = EPI_F32_SPLITK, dtype_code(X.dtype), int(accumulate)
        outs.append(out)
        gs.append(g)
    nb = lib().nbest_wgrad_pair_ws_bytes(C.byref(gs[0]), C.byref(gs[1]))
    ws = _ws(nb, X1.device)
    gs[0].ws, gs[0].ws_bytes = ws.data_ptr(), ws.numel()
    check(lib().nbest_wgrad_pair(C.byref(gs[0]), C.byref(gs[1]), stream_ptr()), "wgrad_pair")
    return outs


WGRAD_GROUP_PLAN, WGRAD_GROUP_NEVER, WGRAD_GROUP_ALWAYS, WGRAD_GROUP_WINDOW = 0, 1, 2, 3     # EncoderDesc.wgrad_group


def wgrad_group(problems, outs=None, accumulate=False):
    """[dY_i^T . X_i] in fp32 by ONE launch without K-splits (nbest_wgrad_group): problems = [(dY_i [K, M_i], X_i [K, N_i]), ...] bf16,
    token-major, 1 .. 8 of them with the same K; outs[i] [M_i, N_i] fp32 (accumulate: added to)"""
    n = len(problems)
    gs = (GemmArgs * max(n, 1))()
    res = []
    for i, (dY, X) in enumerate(problems):
        M, N = dY.shape[1], X.shape[1]
        out = outs[i] if outs is not None else torch.empty(M, N, dtype=torch.float32, device=X.device)
        g = gs[i]
        g.A, g.B, g.C = dY.data_ptr(), X.data_ptr(), out.data_ptr()
        g.M, g.N, g.K = M, N, X.shape[0]
        g.lda, g.ldb, g.ldc = dY.stride(0), X.stride(0), out.stride(0)
        g.trans_a = g.trans_b = 1
        g.epilogue, g.dtype, g.accumulate = EPI_F32_SPLITK, dtype_code(X.dtype), int(accumulate)
        res.append(out)
    check(lib().nbest_wgrad_group(gs, n, stream_ptr()), "wgrad_group")
    return res


def wgrad_window(entries, outs=None, accumulate=False):
    """one window of weight-gradient tiles (nbest_wgrad_window): entries = [(dY_i [K, M_i], X_i [K, N_i], tile_first, tile_count), ...],
    1 .. 16 of them, at most 256 tiles in all; outs[i] [M_i, N_i] fp32 - only the tiles of the ranges are written (accumulate: added to)"""
    n = len(entries)
    gs = (GemmArgs * max(n, 1))()
    first, count = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    res = []
    for i, (dY, X, f, c) in enumerate(entries):
        M, N = dY.shape[1], X.shape[1]
        out = outs[i] if outs is not None else torch.empty(M, N, dtype=torch.float32, device=X.device)
        g = gs[i]
        g.A, g.B, g.C = dY.data_ptr(), X.data_ptr(), out.data_ptr()
        g.M, g.N, g.K = M, N, X.shape[0]
        g.lda, g.ldb, g.ldc = dY.stride(0), X.stride(0), out.stride(0)
        g.trans_a = g.trans_b = 1
        g.epilogue, g.dtype, g.accumulate = EPI_F32_SPLITK, dtype_code(X.dtype), int(accumulate)
        first[i], count[i] = int(f), int(c)
        res.append(out)
    check(lib().nbest_wgrad_window(gs, first, count, n, stream_ptr()), "wgrad_window")
    return res


def encoder_wgrad_plan(desc, layer_begin, layer_end):
    """the weight-gradient schedule of a backward call (nbest_encoder_wgrad_plan; host only): dict(mode, sets, peel_layer,
    launches=[dict(after_layer, tiles, entries=[(layer, matrix, tile_first, tile_count), ...]), ...])"""
    n = lib().nbest_encoder_wgrad_plan(C.byref(desc), layer_begin, layer_end, None, 0)
    check(min(n, 0), "encoder_wgrad_plan")
    buf = (C.c_int32 * n)()
    check(min(lib().nbest_encoder_wgrad_plan(C.byref(desc), layer_begin, layer_end, buf, n), 0), "encoder_wgrad_plan")
    v = list(buf)
    plan = {"mode": v[0], "sets": v[1], "peel_layer": v[2], "launches": []}
    at = 4
    for _ in range(v[3]):
        after, tiles, ne = v[at:at + 3]
        at += 3
        plan["launches"].append({"after_layer": after, "tiles": tiles, "entries": [tuple(v[at + 4 * i:at + 4 * i + 4]) for i in range(ne)]})
        at += 4 * ne
    return plan


def rows_gather(table, rows, cap):
    """(ids [cap] int64 with -1 padding, vals [cap, H] fp32 with zero padding) <- rows of the fp32 table (nbest_rows_gather)"""
    H = table.shape[1]
    ids = torch.empty(cap, dtype=torch.long, device=table.device)
    vals = torch.empty(cap, H, dtype=torch.float32, device=table.device)
    check(lib().nbest_rows_gather(ptr(table), ptr(rows), rows.numel(), cap, ptr(ids), ptr(vals), H, stream_ptr()), "rows_gather")
    return ids, vals


def rows_zero(table, ids):
    check(lib().nbest_rows_zero(ptr(table), ptr(ids), ids.numel(), table.shape[1], stream_ptr()), "rows_zero")


def rows_add(table, ids, vals):
    """table[ids[i]] += vals[i]; ids unique within the call, negative ids are padding"""
    check(lib().nbest_rows_add(ptr(table), ptr(ids), ptr(vals), ids.numel(), table.shape[1], stream_ptr()), "rows_add")


def gelu_d_decode(U):
    """gelu'(u) as float from what BIAS_GELU stored (bf16 path: q = round(200 g') + 26 in one byte)"""
    return U if U.dtype == torch.float32 else (U.float() - 26.0) / 200.0


def gelu_d_encode(g):
    return torch.clamp(torch.round(g.float() * 200.0 + 26.0), 0, 255).to(torch.uint8)      # round half to even, as the kernels


def cast_fp8(x):
    """bf16 -> e4m3 bytes (unit scale, saturating): the A operand of an fp8 forward GEMM"""
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().nbest_cast_bf16_to_fp8(ptr(x), ptr(out), x.numel(), stream_ptr()), "cast_bf16_to_fp8")
    return out


def _gemm_fp8_args(A8, W8, M, N, K, bias, out_scale, epilogue, R, drop_p, seed, drop_stream, out, B_packed, b_pack_bn, U, C8, colsum_out,
                   colsum_accumulate, a_amax, c8_amax_prev, c8_amax_slots, out_scale_dev, want_c):
    """the argument block of gemm_fp8 / gemm_fp8_plan: (GemmFp8Args, out, U, C8, workspace); every leading dimension is the tensor's
    row stride"""
    dev = A8.device
    if want_c and out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    if not want_c:
        out = None
    if epilogue == EPI_BIAS_GELU:                                   # outputs; DGELU: U is the input, C8 an optional output of the caller's
        if U is None:
            U = torch.empty(M, N, dtype=torch.uint8, device=dev)
        if C8 is None:
            C8 = torch.empty(M, N, dtype=torch.uint8, device=dev)
    if epilogue == EPI_BIAS_GELU_Q8 and C8 is None:                 # its one output (call with want_c=False: a C is refused)
        C8 = torch.empty(M, N, dtype=torch.uint8, device=dev)
    g = GemmFp8Args()
    g.A, g.B = A8.data_ptr(), W8.data_ptr()
    g.C = out.data_ptr() if out is not None else None
    g.bias = bias.data_ptr() if bias is not None else None
    g.M, g.N, g.K, g.lda, g.ldb = M, N, K, A8.stride(0), W8.stride(0)
    g.ldc = out.stride(0) if out is not None else N
    g.epilogue, g.out_scale, g.drop_p, g.drop_stream, g.seed = epilogue, out_scale, drop_p, drop_stream, seed
    if U is not None:
        g.U, g.ldu = U.data_ptr(), U.stride(0)
    if C8 is not None:
        g.C8, g.ldc8 = C8.data_ptr(), C8.stride(0)
    if R is not None:
        g.R, g.ldr = R.data_ptr(), R.stride(0)
    if B_packed is not None:
        g.B_packed, g.b_pack_bn = B_packed.data_ptr(), b_pack_bn
    if out_scale_dev is not None:
        g.out_scale_dev = out_scale_dev.data_ptr()
    if a_amax is not None:
        g.a_amax = _amax_args(a_amax, None)[0]
    g.c8_amax_prev, g.c8_amax_new = _amax_args(c8_amax_prev, c8_amax_slots)
    ws = None
    if colsum_out is not None:
        g.colsum_out, g.colsum_accumulate = colsum_out.data_ptr(), int(colsum_accumulate)
        ws = _ws(lib().nbest_gemm_fp8_ws_bytes(C.byref(g)), dev)
        g.ws, g.ws_bytes = ws.data_ptr(), ws.numel()
    return g, out, U, C8, ws


def gemm_fp8(A8, W8, M, N, K, bias=None, out_scale=1.0, epilogue=EPI_BIAS, R=None, drop_p=0.0, seed=0, drop_stream=0, out=None, B_packed=None,
             b_pack_bn=0, U=None, C8=None, colsum_out=None, colsum_accumulate=False, a_amax=None, c8_amax_prev=None, c8_amax_slots=None,
             out_scale_dev=None, want_c=True):
    """C[M,N] (bf16) = epi((A8 . W8^T) * out_scale + bias), A8 / W8 e4m3 bytes; BIAS_GELU also returns (U 8-bit gelu', C8 fp8 copy).
    The whole of nbest_gemm_fp8_args: ``bias=None`` for NONE / RES / DGELU; ``U``: the GELU' rows DGELU reads (BIAS_GELU: where it writes
    them); ``C8``: the e4m3 copy (DGELU: optional); ``colsum_out`` [N] fp32 (+)= the column sums of DGELU; ``a_amax`` / ``c8_amax_prev``:
    1-element int32 tensors (float bits), ``c8_amax_slots``: a slot block, as _amax_args; ``out_scale_dev``: a device float that overrides
    ``out_scale``; ``want_c=False``: C = NULL (None is returned in its place).  BIAS_GELU_Q8 (``want_c=False``, no ``U``, no slots) returns C8."""
    g, out, U, C8, ws = _gemm_fp8_args(A8, W8, M, N, K, bias, out_scale, epilogue, R, drop_p, seed, drop_stream, out, B_packed, b_pack_bn, U, C8,
                                       colsum_out, colsum_accumulate, a_amax, c8_amax_prev, c8_amax_slots, out_scale_dev, want_c)
    check(lib().nbest_gemm_fp8(C.byref(g), stream_ptr()), "gemm_fp8")
    if epilogue == EPI_BIAS_GELU_Q8:
        return C8
    return (out, U, C8) if epilogue == EPI_BIAS_GELU else out


def gemm_fp8_plan_args(g):
    """nbest_gemm_fp8_plan on a filled GemmFp8Args, as a dict of the nbest_gemm_fp8_plan_info fields (host only, nothing enqueued); an
    argument block nbest_gemm_fp8 refuses raises with the same code"""
    info = GemmFp8PlanInfo()
    check(lib().nbest_gemm_fp8_plan(C.byref(g), C.byref(info)), "gemm_fp8_plan")
    return {name: int(getattr(info, name)) for name, _ in GemmFp8PlanInfo._fields_}


def gemm_fp8_plan(A8, W8, M, N, K, bias=None, out_scale=1.0, epilogue=EPI_BIAS, R=None, drop_p=0.0, seed=0, drop_stream=0, out=None,
                  B_packed=None, b_pack_bn=0, U=None, C8=None, colsum_out=None, colsum_accumulate=False, a_amax=None, c8_amax_prev=None,
                  c8_amax_slots=None, out_scale_dev=None, want_c=True):
    """the kernel ``gemm_fp8`` would launch for the same arguments (nbest_gemm_fp8_plan), as a dict; launches nothing"""
    g = _gemm_fp8_args(A8, W8, M, N, K, bias, out_scale, epilogue, R, drop_p, seed, drop_stream, out, B_packed, b_pack_bn, U, C8, colsum_out,
                       colsum_accumulate, a_amax, c8_amax_prev, c8_amax_slots, out_scale_dev, want_c)[0]
    return gemm_fp8_plan_args(g)


def gemm_fp8_plan_shape(M, N, K, epilogue=EPI_BIAS, lda=None, ldb=None, ldc=None, packed_bn=0, drop_p=0.0):
    """gemm_fp8_plan from a shape alone (no torch, no GPU): stand-in addresses, every operand the epilogue reads present"""
    g = GemmFp8Args()
    fake = 1 << 20
    g.A = g.B = g.C = fake
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = (lda or K), (ldb or K), (ldc or N)
    g.ldr = g.ldu = g.ldc8 = N
    g.epilogue, g.out_scale, g.drop_p = epilogue, 1.0, drop_p
    if epilogue in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RES, EPI_BIAS_GELU_Q8):
        g.bias = fake
    if epilogue in (EPI_BIAS_DROP_RES, EPI_RES):
        g.R = fake
    if epilogue in (EPI_BIAS_GELU, EPI_DGELU):
        g.U = fake
    if epilogue in (EPI_BIAS_GELU, EPI_BIAS_GELU_Q8):
        g.C8 = fake
    if epilogue == EPI_BIAS_GELU_Q8:
        g.C = None                                                  # it writes the e4m3 copy only
    if packed_bn:
        g.B_packed, g.b_pack_bn = fake, packed_bn
    return gemm_fp8_plan_args(g)


def wgrad_fp8_plan(M, N, K):
    """nbest_wgrad_fp8_plan -> (splits, k_per_split) of the fp8 weight gradient with M x N outputs (a pair: M = Ma + Mb) over K tokens"""
    sp, kps = C.c_int(0), C.c_int64(0)
    check(lib().nbest_wgrad_fp8_plan(M, N, K, C.byref(sp), C.byref(kps)), "wgrad_fp8_plan")
    return int(sp.value), int(kps.value)


def wgrad_fp8(dY8, X8, M, N, K, a_amax=None, out=None, accumulate=False, x_amax=None):
    """dW[M,N] (fp32) = dY8^T . X8 over K token rows, both operands token-major e4m3 bytes; a_amax / x_amax: the amax words the
    delayed scales of dY8 / X8 were derived from (None = unit scale)"""
    if out is None:
        out = torch.zeros(M, N, dtype=torch.float32, device=dY8.device)
    ws = _ws(lib().nbest_wgrad_fp8_ws_bytes(M, N, K), dY8.device)
    check(lib().nbest_wgrad_fp8(ptr(dY8), ptr(X8), ptr(out), M, N, K, dY8.stride(0), X8.stride(0), out.stride(0), ptr(a_amax), ptr(x_amax),
                                int(accumulate), ptr(ws), ws.numel(), stream_ptr()), "wgrad_fp8")
    return out


def wgrad_fp8_pair(dY8a, X8a, dY8b, X8b, amax_a=None, amax_b=None, outs=None, accumulate=False, xamax_a=None, xamax_b=None):
    """(dY8a^T . X8a / s_a, dY8b^T . X8b / s_b) in fp32 by ONE launch; dY8_i [K, M_i], X8_i [K, N] token-major e4m3 bytes"""
    K, N = X8a.shape
    Ma, Mb = dY8a.shape[1], dY8b.shape[1]
    oa, ob = outs if outs is not None else (torch.zeros(Ma, N, dtype=torch.float32, device=X8a.device),
                                            torch.zeros(Mb, N, dtype=torch.float32, device=X8a.device))
    ws = _ws(lib().nbest_wgrad_fp8_pair_ws_bytes(Ma, Mb, N, K), X8a.device)
    check(lib().nbest_wgrad_fp8_pair(ptr(dY8a), ptr(X8a), ptr(oa), Ma, dY8a.stride(0), X8a.stride(0), oa.stride(0), ptr(amax_a), ptr(xamax_a),
                                     ptr(dY8b), ptr(X8b), ptr(ob), Mb, dY8b.stride(0), X8b.stride(0), ob.stride(0), ptr(amax_b), ptr(xamax_b),
                                     N, K, int(accumulate), ptr(ws), ws.numel(), stream_ptr()), "wgrad_fp8_pair")
    return oa, ob


def layernorm_fwd(x, gamma, beta, eps):
    M, H = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
    check(lib().nbest_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(stats), M, H, eps, dtype_code(x.dtype),
                                    stream_ptr()), "layernorm_fwd")
    return y, stats


def layernorm_bwd(dy, x, stats, gamma, want_dbias=True, drop_p=0.0, seed=0, drop_stream=0, want_params=True):
    """``want_params=False``: dx / dx_drop only (dgamma = dbeta = dbias = NULL, no workspace - the call of a no_param_grad backward);
    the three sums come back as None"""
    M, H = x.shape
    dx = torch.empty_like(x)
    dxd = torch.empty_like(x) if drop_p > 0 else None
    dg = torch.zeros(H, dtype=torch.float32, device=x.device) if want_params else None
    db = torch.zeros_like(dg) if want_params else None
    dbias = torch.zeros_like(dg) if want_params and want_dbias else None
    ws = _ws(lib().nbest_rowred_ws_bytes(M, H), x.device) if want_params else None
    check(lib().nbest_layernorm_bwd(ptr(dy), ptr(x), ptr(stats), ptr(gamma), ptr(dx), ptr(dxd), ptr(dg), ptr(db), ptr(dbias),
                                    M, H, dtype_code(x.dtype), 0, drop_p, seed, drop_stream, ptr(ws), ws.numel() if ws is not None else 0,
                                    stream_ptr()), "layernorm_bwd")
    return dx, dxd, dg, db, dbias


def colsum(X, accumulate=False, out=None):
    M, N = X.shape
    if out is None:
        out = torch.zeros(N, dtype=torch.float32, device=X.device)
    ws = _ws(lib().nbest_rowred_ws_bytes(M, N), X.device)
    check(lib().nbest_colsum(ptr(X), ptr(out), M, N, X.stride(0), dtype_code(X.dtype), int(accumulate), ptr(ws), ws.numel(),
                             stream_ptr()), "colsum")
    return out


def attention_fwd(qkv, key_mask, B, S, heads, drop_p=0.0, seed=0, drop_stream=0, want_keep=False):
    """``want_keep``: also return the dropout keep words for attention_bwd(keep=...) (None where the shape has no such path)"""
    H = heads * 64
    ctx = torch.empty(B * S, H, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, heads, S, dtype=torch.float32, device=qkv.device)
    if want_keep:
        nb = lib().nbest_attention_keep_bytes(B, S, heads) if qkv.dtype == torch.bfloat16 else 0
        keep = torch.zeros(nb // 4, dtype=torch.int32, device=qkv.device) if nb else None
        check(lib().nbest_attention_fwd_keep(ptr(qkv), ptr(key_mask), ptr(ctx), ptr(lse), B, S, heads, 64, dtype_code(qkv.dtype),
                                             drop_p, seed, drop_stream, ptr(keep), stream_ptr()), "attention_fwd_keep")
        return ctx, lse, keep
    check(lib().nbest_attention_fwd(ptr(qkv), ptr(key_mask), ptr(ctx), ptr(lse), B, S, heads, 64, dtype_code(qkv.dtype),
                                    drop_p, seed, drop_stream, stream_ptr()), "attention_fwd")
    return ctx, lse


def attention_cls_fwd(q, ldq, kv, ldkv, key_mask, B, S, heads, out=None):
    """nbest_attention_cls_fwd: one query row per (utterance, head) -> ctx [B, heads * 64] (q, kv: element strides ldq / ldkv)"""
    H = heads * 64
    ctx = torch.empty(B, H, dtype=kv.dtype, device=kv.device) if out is None else out
    check(lib().nbest_attention_cls_fwd(ptr(q), ldq, ptr(kv), ldkv, ptr(key_mask), ptr(ctx), ctx.stride(0), B, S, heads, 64,
                                        dtype_code(kv.dtype), stream_ptr()), "attention_cls_fwd")
    return ctx


def attention_probs(qkv, key_mask, lse, B, S, heads, out=None):
    """nbest_attention_probs: the softmax probabilities of the forward that stashed ``qkv`` and ``lse`` -> fp32 [B, heads, S, S]
    (masked keys 0, no dropout)"""
    probs = torch.empty(B, heads, S, S, dtype=torch.float32, device=qkv.device) if out is None else out
    check(lib().nbest_attention_probs(ptr(qkv), ptr(key_mask), ptr(lse), ptr(probs), B, S, heads, 64, dtype_code(qkv.dtype),
                                      stream_ptr()), "attention_probs")
    return probs


def attention_rollout_step(qkv, key_mask, lse, r_in, residual, B, S, heads, out=None):
    """nbest_attention_rollout_step: fp32 [B, S] ``r_in`` through residual I + (1 - residual) mean_h P_h, P the probabilities
    attention_probs gives for the same ``qkv`` / ``key_mask`` / ``lse`` (never written) -> fp32 [B, S] (``out``: another buffer)"""
    r_out = torch.empty(B, S, dtype=torch.float32, device=qkv.device) if out is None else out
    check(lib().nbest_attention_rollout_step(ptr(qkv), ptr(key_mask), ptr(lse), ptr(r_in), ptr(r_out), float(residual), B, S, heads, 64,
                                             dtype_code(qkv.dtype), stream_ptr()), "attention_rollout_step")
    return r_out


def attention_cls_probs(q, ldq, kv, ldkv, key_mask, B, S, heads, out=None):
    """nbest_attention_cls_probs: the probabilities of one query row per (utterance, head) -> fp32 [B, heads, S]
    (arguments of attention_cls_fwd; ``out``: rows of stride out.stride(1))"""
    probs = torch.empty(B, heads, S, dtype=torch.float32, device=kv.device) if out is None else out
    check(lib().nbest_attention_cls_probs(ptr(q), ldq, ptr(kv), ldkv, ptr(key_mask), ptr(probs), probs.stride(1), B, S, heads, 64,
                                          dtype_code(kv.dtype), stream_ptr()), "attention_cls_probs")
    return probs


def head_gate_fwd(ctx, gate, heads, out=None):
    """nbest_head_gate_fwd: ctx [M, >= heads * 64] (rows of stride ctx.stride(0)), gate fp32 [heads] -> gate[h] * ctx per head slice.
    ``out``: where the result goes (rows of stride out.stride(0); ``out is ctx``: in place); None = a fresh [M, heads * 64] tensor"""
    M = ctx.shape[0]
    if out is None:
        out = torch.empty(M, heads * 64, dtype=ctx.dtype, device=ctx.device)
    check(lib().nbest_head_gate_fwd(ptr(ctx), ctx.stride(0), ptr(out), out.stride(0), ptr(gate), M, heads, 64, dtype_code(ctx.dtype),
                                    stream_ptr()), "head_gate_fwd")
    return out


def head_gate_bwd(ctx, dctx, gate, B, S, heads, want_dgate=True):
    """nbest_head_gate_bwd: ctx (the un-gated context) and dctx (the gradient w.r.t. the gated one) [B * S, heads * 64], gate fp32
    [heads] -> dgate fp32 [B, heads] (None without ``want_dgate``); dctx is scaled by the gate IN PLACE (left alone where gate == 1)"""
    dgate = torch.empty(B, heads, dtype=torch.float32, device=dctx.device) if want_dgate else None
    check(lib().nbest_head_gate_bwd(ptr(ctx), ptr(dctx), ptr(gate), ptr(dgate), B, S, heads, 64, dtype_code(dctx.dtype), stream_ptr()),
          "head_gate_bwd")
    return dgate


def encoder_act_view(desc, act, layer):
    """nbest_encoder_act_view: (qkv, lse) device addresses of ``layer`` inside the stash ``act`` (a uint8 tensor) that
    nbest_encoder_forward wrote with ``desc``; raises for a frozen (unstashed) layer"""
    q, l = C.c_void_p(), C.c_void_p()
    check(lib().nbest_encoder_act_view(C.byref(desc), ptr(act), layer, C.byref(q), C.byref(l)), "encoder_act_view")
    return q.value, l.value


def head_prune_plan(kept, heads, dtype, layer_offsets=None):
    """nbest_head_prune_plan for the kept head indices ``kept`` (one ascending list per layer): the table (HeadPruneLayer array with
    k, idx and the image offsets; the arena offsets too when ``layer_offsets`` - the arena's LayerOffsets - is given) and the byte
    sizes (Wqkv' section, Wo' section, bias image).  Host arithmetic: no GPU needed."""
    L = len(kept)
    tab = (HeadPruneLayer * L)()
    ks = (C.c_int32 * L)(*[len(ix) for ix in kept])
    sizes = [C.c_size_t() for _ in range(3)]
    check(lib().nbest_head_prune_plan(ks, L, heads, dtype_code(dtype), tab, *[C.byref(x) for x in sizes]), "head_prune_plan")
    for l, ix in enumerate(kept):
        for i, h in enumerate(ix):
            tab[l].idx[i] = int(h)
        if layer_offsets is not None:
            o = layer_offsets[l]
            tab[l].src_wqkv, tab[l].src_bqkv, tab[l].src_wo = o.wqkv, o.bqkv, o.wo
    return tab, tuple(x.value for x in sizes)


def head_prune_pack(wts, prm, gate, tab, heads, w_out, b_out, tab_dev=None):
    """nbest_head_prune_pack: gather the compact images of table ``tab`` (head_prune_plan, arena offsets filled) out of ``wts`` /
    ``prm`` under ``gate`` fp32 [L, heads] into ``w_out`` (the dtype of wts) and ``b_out`` (fp32), one launch.  ``tab_dev``: the
    device copy of the table (uploaded here when None); returned."""
    if tab_dev is None:
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(wts.device)
    check(lib().nbest_head_prune_pack(ptr(wts), ptr(prm), ptr(gate), tab, ptr(tab_dev), len(tab), heads, dtype_code(wts.dtype),
                                      ptr(w_out), w_out.numel() * w_out.element_size(), ptr(b_out),
                                      b_out.numel() * b_out.element_size(), stream_ptr()), "head_prune_pack")
    return tab_dev


def encoder_infer_pruned(desc, wts, prm, ids, seg, pos, key_mask, ws, cls_out, tab, w, w_packed, bqkv):
    """nbest_encoder_infer_pruned -> cls_out [B, H] on the compact images ``w`` / ``w_packed`` (or None) / ``bqkv`` of table ``tab``"""
    im = HeadPruneImages(w.data_ptr(), None if w_packed is None else w_packed.data_ptr(), bqkv.data_ptr(), tab)
    check(lib().nbest_encoder_infer_pruned(C.byref(desc), ptr(wts), ptr(prm), ptr(ids), ptr(seg), ptr(pos), ptr(key_mask), ptr(ws),
                                           ws.numel(), ptr(cls_out), C.byref(im), stream_ptr()), "encoder_infer_pruned")


def encoder_infer_fp8(desc, wts, prm, ids, seg, pos, key_mask, ws, cls_out):
    """nbest_encoder_infer_fp8 -> cls_out [B, H]: the calibration pass or the fp8 pass, as the descriptor's fp8 fields say"""
    check(lib().nbest_encoder_infer_fp8(C.byref(desc), ptr(wts), ptr(prm), ptr(ids), ptr(seg), ptr(pos), ptr(key_mask), ptr(ws),
                                        ws.numel(), ptr(cls_out), stream_ptr()), "encoder_infer_fp8")


def token_select(score, key_mask, k, origin=None, want_origin=True):
    """nbest_token_select: per utterance the ``k`` positions to keep of fp32 [B, S] ``score`` under u8 [B, S] ``key_mask`` (position 0,
    then unmasked before masked, numbers before NaN, higher score, lower index) -> (idx int32 [B, k] ascending, mask u8 [B, k],
    maskf fp32 [B, k], origin int32 [B, k] or None); ``origin`` int32 [B, S]: what idx is translated through (None: the identity)"""
    B, S = score.shape
    dev = score.device
    idx = torch.empty(B, k, dtype=torch.int32, device=dev)
    mask = torch.empty(B, k, dtype=torch.uint8, device=dev)
    maskf = torch.empty(B, k, dtype=torch.float32, device=dev)
    org = torch.empty(B, k, dtype=torch.int32, device=dev) if want_origin else None
    check(lib().nbest_token_select(ptr(score), ptr(key_mask), ptr(origin), k, ptr(idx), ptr(mask), ptr(maskf), ptr(org), B, S, stream_ptr()),
          "token_select")
    return idx, mask, maskf, org


def rows_compact(src, idx, out=None):
    """nbest_rows_compact: ``src`` [B, S, H] (bf16 / fp32, contiguous) gathered by int32 [B, k] ``idx`` -> [B, k, H]"""
    B, S, H = src.shape
    k = idx.shape[1]
    dst = torch.empty(B, k, H, dtype=src.dtype, device=src.device) if out is None else out
    check(lib().nbest_rows_compact(ptr(src), ptr(idx), ptr(dst), B, S, k, H, dtype_code(src.dtype), stream_ptr()), "rows_compact")
    return dst


def encoder_infer_tokens(desc, wts, prm, ids, seg, pos, key_mask, ws, cls_out, keep, token_kept=None):
    """nbest_encoder_infer_tokens -> cls_out [B, H]: nbest_encoder_infer that keeps ``keep[l]`` tokens per utterance after layer l
    (L - 1 host ints); ``token_kept`` (int32 [L - 1, B, S] or None) receives the original positions that leave every layer"""
    n = len(keep)
    arr = (C.c_int32 * max(n, 1))(*[int(x) for x in keep])
    check(lib().nbest_encoder_infer_tokens(C.byref(desc), ptr(wts), ptr(prm), ptr(ids), ptr(seg), ptr(pos), ptr(key_mask), ptr(ws),
                                           ws.numel(), ptr(cls_out), arr, n, ptr(token_kept), stream_ptr()), "encoder_infer_tokens")
    return cls_out


def encoder_infer(desc, wts, prm, ids, seg, pos, key_mask, ws, cls_out, cls_attn=None):
    """nbest_encoder_infer -> cls_out [B, H]; with ``cls_attn`` (fp32 [L, B, heads, S]) nbest_encoder_infer_attn, which also
    writes the CLS row's attention probabilities of every layer"""
    if cls_attn is None:
        check(lib().nbest_encoder_infer(C.byref(desc), ptr(wts), ptr(prm), ptr(ids), ptr(seg), ptr(pos), ptr(key_mask), ptr(ws),
                                        ws.numel(), ptr(cls_out), stream_ptr()), "encoder_infer")
    else:
        check(lib().nbest_encoder_infer_attn(C.byref(desc), ptr(wts), ptr(prm), ptr(ids), ptr(seg), ptr(pos), ptr(key_mask), ptr(ws),
                                             ws.numel(), ptr(cls_out), ptr(cls_attn), stream_ptr()), "encoder_infer_attn")
    return cls_out


def attention_bwd(qkv, key_mask, ctx, dctx, lse, B, S, heads, drop_p=0.0, seed=0, drop_stream=0, dbias=None, keep=None,
                  accumulate=False):
    """``dbias`` (fp32 [3H]): receives the column sums of dqkv - overwritten, or added to with ``accumulate``"""
    dqkv = torch.empty_like(qkv)
    ws = _ws(lib().nbest_attention_bwd_ws_bytes(B, S, heads), qkv.device) if dbias is not None else None
    if keep is not None:
        check(lib().nbest_attention_bwd_keep(ptr(qkv), ptr(key_mask), ptr(ctx), ptr(dctx), ptr(lse), ptr(dqkv), ptr(dbias), int(accumulate),
                                             ptr(ws), ws.numel() if ws is not None else 0, B, S, heads, 64, dtype_code(qkv.dtype), drop_p,
                                             seed, drop_stream, ptr(keep), stream_ptr()), "attention_bwd_keep")
        return dqkv
    check(lib().nbest_attention_bwd(ptr(qkv), ptr(key_mask), ptr(ctx), ptr(dctx), ptr(lse), ptr(dqkv), ptr(dbias), int(accumulate), ptr(ws),
                                    ws.numel() if ws is not None else 0, B, S, heads, 64, dtype_code(qkv.dtype), drop_p, seed,
                                    drop_stream, stream_ptr()), "attention_bwd")
    return dqkv


# ---- the fp8 producers on their own (include/nbest_hip.h, "The fp8 PRODUCERS on their own"; used by the kernel tests) ----
# amax_prev: a 1-element int32 tensor holding the float bits of last pass's amax, or None (unit scale); amax_slots: an int32 tensor of
# AMAX_TENSOR_WORDS words the kernel raises its slot words in, or None (nothing recorded).  The e4m3 copies come back as uint8
# tensors pre-filled with 0x7F, an e4m3 NaN code no producer writes: a byte the kernel skipped shows.
def _amax_args(amax_prev, amax_slots):
    if amax_prev is not None and (amax_prev.dtype != torch.int32 or amax_prev.numel() != 1):
        raise ValueError("nbest_amd: amax_prev must be a 1-element int32 tensor (float bits)")
    if amax_slots is not None and (amax_slots.dtype != torch.int32 or amax_slots.numel() != AMAX_TENSOR_WORDS or not amax_slots.is_contiguous()):
        raise ValueError("nbest_amd: amax_slots must be a contiguous int32 tensor of %d words" % AMAX_TENSOR_WORDS)
    return ptr(amax_prev), ptr(amax_slots)


def _e4m3_buffer(shape, device):
    return torch.full(shape, 0x7F, dtype=torch.uint8, device=device)


def layernorm_fwd_fp8(x, gamma, beta, eps, amax_prev=None, amax_slots=None, want8=True):
    """nbest_layernorm_fwd_fp8 -> (y, stats, y8); ``want8=False``: no copy (y8 None)"""
    M, H = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
    y8 = _e4m3_buffer((M, H), x.device) if want8 else None
    ap, an = _amax_args(amax_prev, amax_slots)
    check(lib().nbest_layernorm_fwd_fp8(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(y8), ptr(stats), M, H, eps, dtype_code(x.dtype), ap, an,
                                        stream_ptr()), "layernorm_fwd_fp8")
    return y, stats, y8


def layernorm_bwd_fp8(dy, x, stats, gamma, want_dbias=True, drop_p=0.0, seed=0, drop_stream=0, want_params=True, amax_prev=None,
                      amax_slots=None, want8=True, want_dx_drop=True):
    """nbest_layernorm_bwd_fp8 -> layernorm_bwd's five results + out8 (the copy of dx_drop under dropout, else of dx);
    ``want8=False``: record only; ``want_dx_drop=False`` (dropout with ``want8``): dx_drop = NULL, only its copy is written"""
    M, H = x.shape
    dx = torch.empty_like(x)
    dxd = torch.empty_like(x) if drop_p > 0 and want_dx_drop else None
    dg = torch.zeros(H, dtype=torch.float32, device=x.device) if want_params else None
    db = torch.zeros_like(dg) if want_params else None
    dbias = torch.zeros_like(dg) if want_params and want_dbias else None
    ws = _ws(lib().nbest_rowred_ws_bytes(M, H), x.device) if want_params else None
    out8 = _e4m3_buffer((M, H), x.device) if want8 else None
    ap, an = _amax_args(amax_prev, amax_slots)
    check(lib().nbest_layernorm_bwd_fp8(ptr(dy), ptr(x), ptr(stats), ptr(gamma), ptr(dx), ptr(dxd), ptr(dg), ptr(db), ptr(dbias),
                                        M, H, dtype_code(x.dtype), 0, drop_p, seed, drop_stream, ptr(ws), ws.numel() if ws is not None else 0,
                                        ptr(out8), ap, an, stream_ptr()), "layernorm_bwd_fp8")
    return dx, dxd, dg, db, dbias, out8


def attention_fwd_fp8(qkv, key_mask, B, S, heads, drop_p=0.0, seed=0, drop_stream=0, want_keep=False, amax_prev=None, amax_slots=None,
                      want8=True):
    """nbest_attention_fwd_fp8 -> (ctx, lse, keep, ctx8); keep as attention_fwd(want_keep=...), None without it"""
    H = heads * 64
    ctx = torch.empty(B * S, H, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, heads, S, dtype=torch.float32, device=qkv.device)
    nb = lib().nbest_attention_keep_bytes(B, S, heads) if want_keep and qkv.dtype == torch.bfloat16 else 0
    keep = torch.zeros(nb // 4, dtype=torch.int32, device=qkv.device) if nb else None
    ctx8 = _e4m3_buffer((B * S, H), qkv.device) if want8 else None
    ap, an = _amax_args(amax_prev, amax_slots)
    check(lib().nbest_attention_fwd_fp8(ptr(qkv), ptr(key_mask), ptr(ctx), ptr(ctx8), ptr(lse), B, S, heads, 64, dtype_code(qkv.dtype),
                                        drop_p, seed, drop_stream, ptr(keep), ap, an, stream_ptr()), "attention_fwd_fp8")
    return ctx, lse, keep, ctx8


def attention_bwd_fp8(qkv, key_mask, ctx, dctx, lse, B, S, heads, drop_p=0.0, seed=0, drop_stream=0, dbias=None, keep=None,
                      accumulate=False, amax_prev=None, amax_slots=None, want8=True, want_dqkv=True):
    """nbest_attention_bwd_fp8 -> (dqkv, out8); ``want_dqkv=False`` (with ``want8``): dqkv = NULL, only the copy is written"""
    dqkv = torch.empty_like(qkv) if want_dqkv else None
    ws = _ws(lib().nbest_attention_bwd_ws_bytes(B, S, heads), qkv.device) if dbias is not None else None
    out8 = _e4m3_buffer(tuple(qkv.shape), qkv.device) if want8 else None
    ap, an = _amax_args(amax_prev, amax_slots)
    check(lib().nbest_attention_bwd_fp8(ptr(qkv), ptr(key_mask), ptr(ctx), ptr(dctx), ptr(lse), ptr(dqkv), ptr(dbias), int(accumulate), ptr(ws),
                                        ws.numel() if ws is not None else 0, B, S, heads, 64, dtype_code(qkv.dtype), drop_p, seed,
                                        drop_stream, ptr(keep), ptr(out8), ap, an, stream_ptr()), "attention_bwd_fp8")
    return dqkv, out8


def cast_fp8_scaled(x, amax_prev=None, amax_slots=None):
    """nbest_cast_bf16_to_fp8_scaled: bf16 -> e4m3 bytes under the delayed scale of ``amax_prev``; max |x| recorded into ``amax_slots``"""
    out = _e4m3_buffer(tuple(x.shape), x.device)
    ap, an = _amax_args(amax_prev, amax_slots)
    check(lib().nbest_cast_bf16_to_fp8_scaled(ptr(x), ptr(out), x.numel(), ap, an, stream_ptr()), "cast_bf16_to_fp8_scaled")
    return out


def amax_bf16(x, amax_slots):
    """nbest_amax_bf16: raise the slot words of ``amax_slots`` by max |x| of a bf16 tensor"""
    _, an = _amax_args(None, amax_slots)
    check(lib().nbest_amax_bf16(ptr(x), x.numel(), an, stream_ptr()), "amax_bf16")


def embed_ln_fwd(ids, seg, pos, word, type_tab, ptab, gamma, beta, eps, drop_p=0.0, seed=0, drop_stream=0, delta=None):
    """``delta`` (fp32 [B*S, H]): nbest_embed_ln_fwd_adv, the word rows moved by it"""
    M, H = ids.numel(), word.shape[1]
    out = torch.empty(M, H, dtype=word.dtype, device=word.device)
    stats = torch.empty(M, 2, dtype=torch.float32, device=word.device)
    if delta is not None:
        _check_delta(delta, M, H)
        check(lib().nbest_embed_ln_fwd_adv(ptr(ids), ptr(seg), ptr(pos), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma), ptr(beta),
                                           ptr(delta), ptr(out), ptr(stats), M, H, eps, dtype_code(word.dtype), drop_p, seed, drop_stream,
                                           stream_ptr()), "embed_ln_fwd_adv")
        return out, stats
    check(lib().nbest_embed_ln_fwd(ptr(ids), ptr(seg), ptr(pos), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma), ptr(beta),
                                   ptr(out), ptr(stats), M, H, eps, dtype_code(word.dtype), drop_p, seed, drop_stream,
                                   stream_ptr()), "embed_ln_fwd")
    return out, stats


def embed_ln_fwd_interp(ids, base_ids, alpha, seg, pos, word, type_tab, ptab, gamma, beta, eps, drop_p=0.0, seed=0, drop_stream=0):
    """nbest_embed_ln_fwd_interp: ids / base_ids [B, S] int64, alpha fp32 [B] -> (out [B*S, H], stats [B*S, 2]); the word row of
    sequence b moves from word[base_ids] (alpha 0) to word[ids] (alpha 1)"""
    B, S = ids.shape
    H = word.shape[1]
    out = torch.empty(B * S, H, dtype=word.dtype, device=word.device)
    stats = torch.empty(B * S, 2, dtype=torch.float32, device=word.device)
    check(lib().nbest_embed_ln_fwd_interp(ptr(ids), ptr(base_ids), ptr(alpha), ptr(seg), ptr(pos), ptr(word), ptr(type_tab), ptr(ptab),
                                          ptr(gamma), ptr(beta), ptr(out), ptr(stats), B, S, H, eps, dtype_code(word.dtype), drop_p, seed,
                                          drop_stream, stream_ptr()), "embed_ln_fwd_interp")
    return out, stats


def embed_attrib(ids, base_ids, alpha, seg, pos, word, type_tab, ptab, gamma, dhidden, pairs, m, S, eps, out=None):
    """nbest_embed_attrib -> fp32 [pairs, S]: integrated-gradients attribution of every token of each pair, from the interpolated
    call's inputs (pair p = sequences p m .. p m + m - 1) and ``dhidden``, the gradient w.r.t. its embedding LayerNorm output"""
    H = word.shape[1]
    attr = torch.empty(pairs, S, dtype=torch.float32, device=word.device) if out is None else out
    check(lib().nbest_embed_attrib(ptr(ids), ptr(base_ids), ptr(alpha), ptr(seg), ptr(pos), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma),
                                   ptr(dhidden), ptr(attr), pairs, m, S, H, eps, dtype_code(word.dtype), stream_ptr()), "embed_attrib")
    return attr


def _check_delta(delta, M, H):
    if delta.dtype != torch.float32 or not delta.is_contiguous() or delta.numel() != M * H:
        raise ValueError("nbest_amd: delta must be a contiguous fp32 tensor of [%d, %d] elements" % (M, H))


def embed_adv_delta(ids, seg, pos, key_mask, word, type_tab, ptab, gamma, dout, B, S, eps, epsilon, drop_p=0.0, seed=0, drop_stream=0,
                    out=None, norm=None, ws=None):
    """nbest_embed_adv_delta -> (delta fp32 [B*S, H], norm fp32 [B]): the FGM perturbation of the word rows from ``dout``, the gradient
    w.r.t. the embedding LayerNorm output of the clean pass (its drop_p / seed / drop_stream): the per-token LayerNorm backward scaled
    per utterance to an L2 norm of ``epsilon``; norm[b] is the gradient's norm before scaling.  ``out`` / ``norm`` / ``ws``: buffers to
    write into (None: allocated)."""
    H = word.shape[1]
    delta = torch.empty(B * S, H, dtype=torch.float32, device=word.device) if out is None else out
    _check_delta(delta, B * S, H)
    norm = torch.empty(B, dtype=torch.float32, device=word.device) if norm is None else norm
    if ws is None:
        ws = _ws(lib().nbest_embed_adv_ws_bytes(B, S), word.device)
    check(lib().nbest_embed_adv_delta(ptr(ids), ptr(seg), ptr(pos), ptr(key_mask), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma), ptr(dout),
                                      ptr(delta), ptr(norm), B, S, H, eps, dtype_code(word.dtype), drop_p, seed, drop_stream, float(epsilon),
                                      ptr(ws), ws.numel(), stream_ptr()), "embed_adv_delta")
    return delta, norm


def word_perm(ids):
    """token indices sorted by word id, ties in token order (int32 [B*S]): the index the deterministic embedding backward
    reduces over.  The data loaders build it on the host next to ids (trainer.EncodedSplit.host_batch, bench.py); this is the
    device-side stand-in for callers that hand over bare id tensors (a stable sort on the current stream, no host sync)."""
    return torch.sort(ids.reshape(-1), stable=True)[1].to(torch.int32)


def embed_ln_bwd(ids, seg, pos, word, type_tab, ptab, gamma, stats, dout, B, S, word_pad_id=-1, pos_pad_id=-1, drop_p=0.0,
                 seed=0, drop_stream=0, perm=None, accumulate_into=None, delta=None):
    """accumulate_into = (dword, dtype_tab, dptab, dgamma, dbeta): add to these (tables_accumulate = accumulate = 1)
    ``delta`` (fp32 [B*S, H]): nbest_embed_ln_bwd_adv, for a forward that ran with it (``stats`` are that forward's)"""
    H = word.shape[1]
    if perm is None:
        perm = word_perm(ids)
    if delta is not None:
        _check_delta(delta, B * S, H)
        dev, acc = word.device, accumulate_into is not None
        if acc:
            dword, dtype_tab, dptab, dg, db = accumulate_into
        else:
            dword = torch.zeros(word.shape, dtype=torch.float32, device=dev)
            dtype_tab = torch.zeros(type_tab.shape, dtype=torch.float32, device=dev)
            dptab = torch.zeros(ptab.shape, dtype=torch.float32, device=dev)
            dg = torch.zeros(H, dtype=torch.float32, device=dev)
            db = torch.zeros_like(dg)
        ws = _ws(lib().nbest_embed_bwd_ws_bytes(B * S, H), dev)
        check(lib().nbest_embed_ln_bwd_adv(ptr(ids), ptr(seg), ptr(pos), ptr(perm), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma), ptr(stats),
                                           ptr(delta), ptr(dout), ptr(dword), ptr(dtype_tab), ptr(dptab), ptr(dg), ptr(db), B, S, H,
                                           type_tab.shape[0], dtype_code(word.dtype), word_pad_id, pos_pad_id, int(acc), int(acc), drop_p, seed,
                                           drop_stream, ptr(ws), ws.numel(), stream_ptr()), "embed_ln_bwd_adv")
        return dword, dtype_tab, dptab, dg, db
    if accumulate_into is not None:
        dword, dtype_tab, dptab, dg, db = accumulate_into
        ws = _ws(lib().nbest_embed_bwd_ws_bytes(B * S, H), word.device)
        check(lib().nbest_embed_ln_bwd(ptr(ids), ptr(seg), ptr(pos), ptr(perm), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma), ptr(stats),
                                       ptr(dout), ptr(dword), ptr(dtype_tab), ptr(dptab), ptr(dg), ptr(db), B, S, H,
                                       type_tab.shape[0], dtype_code(word.dtype), word_pad_id, pos_pad_id, 1, 1, drop_p, seed,
                                       drop_stream, ptr(ws), ws.numel(), stream_ptr()), "embed_ln_bwd")
        return dword, dtype_tab, dptab, dg, db
    dev = word.device
    dword = torch.zeros(word.shape, dtype=torch.float32, device=dev)
    dtype_tab = torch.zeros(type_tab.shape, dtype=torch.float32, device=dev)
    dptab = torch.zeros(ptab.shape, dtype=torch.float32, device=dev)
    dg = torch.zeros(H, dtype=torch.float32, device=dev)
    db = torch.zeros_like(dg)
    ws = _ws(lib().nbest_embed_bwd_ws_bytes(B * S, H), dev)
    check(lib().nbest_embed_ln_bwd(ptr(ids), ptr(seg), ptr(pos), ptr(perm), ptr(word), ptr(type_tab), ptr(ptab), ptr(gamma), ptr(stats),
                                   ptr(dout), ptr(dword), ptr(dtype_tab), ptr(dptab), ptr(dg), ptr(db), B, S, H,
                                   type_tab.shape[0], dtype_code(word.dtype), word_pad_id, pos_pad_id, 0, 0, drop_p, seed,
                                   drop_stream, ptr(ws), ws.numel(), stream_ptr()), "embed_ln_bwd")
    return dword, dtype_tab, dptab, dg, db


class DeviceLabelSpace:
    """Device copy of the STC label hierarchy in the layout nbest_label_space expects."""

    def __init__(self, labels, device):
        off, ids, head_row = [0], [], []
        row = labels.n_top
        for t in range(labels.n_top):
            bs = labels.top2bottom[t]
            ids += bs
            off.append(len(ids))
            if len(bs) >= 2:
                head_row.append(row)
                row += len(bs)
            else:
                head_row.append(-1)
        self.n_rows = row
        assert row == labels.n_head_rows
        self.labels = labels
        i32 = dict(dtype=torch.int32, device=device)
        self.bottom_off = torch.tensor(off, **i32)
        self.bottom_ids = torch.tensor(ids, **i32)
        self.head_row = torch.tensor(head_row, **i32)
        self.head_row_host = head_row
        self.none_flag = torch.tensor([1 if l.endswith("NONE") else 0 for l in labels.idx2label], dtype=torch.uint8, device=device)
        self.c = LabelSpaceC(labels.n_top, labels.n_bottom, row, self.bottom_off.data_ptr(), self.bottom_ids.data_ptr(),
                             self.head_row.data_ptr())


def heads_ws(B, R, H, device):
    """a PRIVATE workspace for stc_heads (the default is a shared scratch buffer): the autograd bridge keeps it until stc_heads_vjp"""
    return torch.empty(lib().nbest_heads_ws_bytes(B, R, H), dtype=torch.uint8, device=device)


def stc_heads_vjp(Wh, dls, top, bott, dtop, dbott, dfin, B, H, dWh, dbh, ws, accumulate=True, drop_p=0.0, seed=0, drop_stream=0):
    """d(CLS) [B, H] (and dWh / dbh, accumulated) for arbitrary upstream gradients of top / bottoms / final; ``ws``: the workspace of
    the stc_heads call that produced top / bott"""
    dcls = torch.empty(B, H, dtype=torch.float32, device=Wh.device)
    check(lib().nbest_stc_heads_vjp(ptr(Wh), C.byref(dls.c), ptr(top), ptr(bott), ptr(dtop), ptr(dbott), ptr(dfin), ptr(dcls), ptr(dWh),
                                    ptr(dbh), B, H, int(accumulate), drop_p, seed, drop_stream, ptr(ws), ws.numel(), stream_ptr()),
          "stc_heads_vjp")
    return dcls


# the soft term of a heads call: kind "kd" (tensors: t_top, t_bott, t_final), "kd_t" (tensors: t_logits; a temperature) or "rdrop"
SoftTerm = collections.namedtuple("SoftTerm", "kind alpha temperature tensors", defaults=(None, ()))


def _stc_heads_call(hidden, cls_stride, Wh, bh, dls, labels_f, B, H, need_grad, accumulate, drop_p, seed, drop_stream, dWh, dbh, ws,
                    soft=None):
    """the outputs, gradient buffers and workspace of one heads call, then nbest_stc_heads or - ``soft``: a SoftTerm -
    nbest_stc_heads_<soft.kind>"""
    dev = Wh.device
    R, nt, nb = dls.n_rows, dls.labels.n_top, dls.labels.n_bottom
    f = dict(dtype=torch.float32, device=dev)
    top, bott, fin = torch.empty(B, nt, **f), torch.empty(B, R - nt, **f), torch.empty(B, nb, **f)
    loss = torch.empty(4, **f)
    dcls = torch.empty(B, H, **f) if need_grad else None
    if need_grad and dWh is None:
        dWh, dbh = torch.zeros(R, H, **f), torch.zeros(R, **f)
    if ws is None:
        ws = _ws(lib().nbest_heads_ws_bytes(B, R, H), dev)
    name, extra = "stc_heads", ()
    if soft is not None:
        name = "stc_heads_" + soft.kind
        extra = tuple(ptr(t) for t in soft.tensors) + (float(soft.alpha),) + (() if soft.temperature is None else (float(soft.temperature),))
    check(getattr(lib(), "nbest_" + name)(
        ptr(hidden), cls_stride, ptr(Wh), ptr(bh), C.byref(dls.c), ptr(labels_f), *extra, ptr(top), ptr(bott), ptr(fin), ptr(loss),
        ptr(dcls), ptr(dWh), ptr(dbh), B, H, dtype_code(hidden.dtype), int(need_grad), int(accumulate), drop_p, seed, drop_stream,
        ptr(ws), ws.numel(), stream_ptr()), name)
    return top, bott, fin, loss, dcls, dWh, dbh


def stc_heads(hidden, cls_stride, Wh, bh, dls, labels_f, B, H, need_grad=True, accumulate=False, drop_p=0.0, seed=0,
              drop_stream=0, dWh=None, dbh=None, ws=None, soft=None):
    """``soft``: a SoftTerm whose tensors the caller has checked (model._heads); the wrappers below check theirs"""
    return _stc_heads_call(hidden, cls_stride, Wh, bh, dls, labels_f, B, H, need_grad, accumulate, drop_p, seed, drop_stream, dWh, dbh, ws,
                           soft)


def stc_heads_kd(hidden, cls_stride, Wh, bh, dls, labels_f, t_top, t_bott, t_final, alpha, B, H, need_grad=True, accumulate=False,
                 drop_p=0.0, seed=0, drop_stream=0, dWh=None, dbh=None, ws=None):
    """stc_heads with a teacher's probabilities (fp32 [B, n_top] / [B, R - n_top] / [B, n_bottom], the top / bott / final of
    another model's predict) as a second set of targets: loss[3] = the soft loss, the gradients are those of
    (1 - alpha) * hard + alpha * soft (nbest_stc_heads_kd)"""
    dev = Wh.device
    R, nt, nb = dls.n_rows, dls.labels.n_top, dls.labels.n_bottom
    for name, t, n in (("t_top", t_top, nt), ("t_bott", t_bott, R - nt), ("t_final", t_final, nb)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (B, n) or not t.is_contiguous():
            raise ValueError("stc_heads_kd: %s must be a contiguous fp32 [%d, %d] tensor on %s (got %s %s on %s)"
                             % (name, B, n, dev, t.dtype, tuple(t.shape), t.device))
    return _stc_heads_call(hidden, cls_stride, Wh, bh, dls, labels_f, B, H, need_grad, accumulate, drop_p, seed, drop_stream, dWh, dbh, ws,
                           soft=SoftTerm("kd", alpha, None, (t_top, t_bott, t_final)))


def stc_heads_kd_t(hidden, cls_stride, Wh, bh, dls, labels_f, t_logits, alpha, temperature, B, H, need_grad=True, accumulate=False,
                   drop_p=0.0, seed=0, drop_stream=0, dWh=None, dbh=None, ws=None):
    """stc_heads with a teacher's LOGITS (fp32 [B, R], another model's stc_heads_logits / predict(return_logits=True)) as soft
    targets at a temperature: both models' logits are divided by ``temperature`` inside the kernel, loss[3] = T^2 x the soft loss
    of the tempered scores, the gradients are those of (1 - alpha) * hard + alpha * that (nbest_stc_heads_kd_t).  The 7-tuple of
    stc_heads_kd; top / bott / final and loss[:3] are the T = 1 quantities"""
    dev = Wh.device
    R = dls.n_rows
    if t_logits is not None and (t_logits.dtype != torch.float32 or t_logits.device != dev or tuple(t_logits.shape) != (B, R)
                                 or not t_logits.is_contiguous()):
        raise ValueError("stc_heads_kd_t: t_logits must be a contiguous fp32 [%d, %d] tensor on %s (got %s %s on %s)"
                         % (B, R, dev, t_logits.dtype, tuple(t_logits.shape), t_logits.device))
    return _stc_heads_call(hidden, cls_stride, Wh, bh, dls, labels_f, B, H, need_grad, accumulate, drop_p, seed, drop_stream, dWh, dbh, ws,
                           soft=SoftTerm("kd_t", alpha, temperature, (t_logits,)))


def stc_heads_rdrop(hidden, cls_stride, Wh, bh, dls, labels_f, alpha, B2, H, need_grad=True, accumulate=False, drop_p=0.0, seed=0,
                    drop_stream=0, dWh=None, dbh=None, ws=None):
    """stc_heads on a batch of ``B2`` = 2 P rows whose rows b and b + P are twins (R-Drop): loss[3] = the sum over the pairs of the
    symmetric KL between the twins' outputs (unscaled), the gradients are those of the hard loss of all B2 rows + alpha * that
    (nbest_stc_heads_rdrop).  The 7-tuple of stc_heads; top / bott / final and loss[:3] are its bits"""
    return _stc_heads_call(hidden, cls_stride, Wh, bh, dls, labels_f, B2, H, need_grad, accumulate, drop_p, seed, drop_stream, dWh, dbh, ws,
                           soft=SoftTerm("rdrop", alpha))


def stc_heads_logits(hidden, cls_stride, Wh, bh, dls, B, H):
    """the logits of the heads on the CLS rows ``hidden[b * cls_stride : +H]`` (fp32 or bf16), no dropout: fp32 [B, R] in the order
    of Wh's rows (the top classifier, then the softmax heads in head order) - the numbers stc_heads makes its scores from
    (nbest_stc_heads_logits, one launch)"""
    logits = torch.empty(B, dls.n_rows, dtype=torch.float32, device=Wh.device)
    check(lib().nbest_stc_heads_logits(ptr(hidden), cls_stride, ptr(Wh), ptr(bh), C.byref(dls.c), ptr(logits), B, H,
                                       dtype_code(hidden.dtype), stream_ptr()), "stc_heads_logits")
    return logits


def stc_decode(top, bott, dls, out=None):
    """``out``: int32 [>= B, n_top] rows to decode into instead of a fresh device tensor - a PINNED host tensor makes the kernel
    write the rows straight into host memory (include/nbest_hip.h nbest_stc_decode)"""
    B = top.shape[0]
    if out is None:
        pred = torch.empty(B, dls.labels.n_top, dtype=torch.int32, device=top.device)
    else:
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape[0] >= B and out.shape[1] == dls.labels.n_top
        assert out.is_cuda or out.is_pinned(), "stc_decode: out must be device memory or pinned host memory"
        pred = out[:B]
    check(lib().nbest_stc_decode(ptr(top), ptr(bott), C.byref(dls.c), ptr(dls.none_flag), ptr(pred), B, stream_ptr()), "stc_decode")
    return pred


def stream_stamp(flag, value):
    """*flag = value in stream order (flag: one int32 of device or PINNED host memory)"""
    assert flag.dtype == torch.int32 and flag.numel() == 1 and (flag.is_cuda or flag.is_pinned())
    check(lib().nbest_stream_stamp(ptr(flag), int(value), stream_ptr()), "stream_stamp")


AMAX_TENSOR_WORDS = 1024        # include/nbest_hip.h NBEST_AMAX_TENSOR_WORDS


def fp8_amax_fold_max(slots, out):
    """out[t] = max(out[t], max over the recording slots of tensor t); the slots are zeroed (nbest_fp8_amax_fold_max)"""
    assert slots.numel() == out.numel() * AMAX_TENSOR_WORDS and slots.dtype == out.dtype == torch.int32
    check(lib().nbest_fp8_amax_fold_max(ptr(slots), ptr(out), out.numel(), stream_ptr()), "fp8_amax_fold_max")


def fp8_amax_fold(slots, out):
    """out[t] = max over the recording slots of tensor t; the slots are zeroed (nbest_fp8_amax_fold)"""
    assert slots.numel() == out.numel() * AMAX_TENSOR_WORDS and slots.dtype == out.dtype == torch.int32
    check(lib().nbest_fp8_amax_fold(ptr(slots), ptr(out), out.numel(), stream_ptr()), "fp8_amax_fold")


def cls_mse(hidden_a, stride_a, hidden_t, stride_t, B, H, da=None, dt=None, grad_scale=1.0):
    loss = torch.empty(1, dtype=torch.float32, device=hidden_a.device)
    check(lib().nbest_cls_mse(ptr(hidden_a), stride_a, ptr(hidden_t), stride_t, ptr(loss), ptr(da), ptr(dt), B, H,
                              dtype_code(hidden_a.dtype), grad_scale, stream_ptr()), "cls_mse")
    return loss


def cls_contrast_ws_bytes(B, H):
    return int(lib().nbest_cls_contrast_ws_bytes(B, H))


def cls_contrast(hidden_a, stride_a, hidden_t, stride_t, B, H, weight, temperature, keys=None, da=None, dt=None, accumulate_dt=False,
                 ws=None):
    """the in-batch contrastive loss between the CLS rows ``hidden_a[b * stride_a : +H]`` (ASR) and ``hidden_t[b * stride_t : +H]``
    (transcript), fp32 or bf16: returns ``out`` = fp32 [4] (the unweighted loss summed over the batch, the alignment hits, B, 0);
    ``da`` [B, H] += weight * dL/da, ``dt`` [B, H] = (or += when ``accumulate_dt``) weight * dL/dt; both None = loss only.
    ``keys``: int64 [B], rows with an equal key stay out of each other's denominators (nbest_cls_contrast)"""
    dev = hidden_a.device
    if keys is not None and (keys.dtype != torch.int64 or keys.device != dev or tuple(keys.shape) != (B,) or not keys.is_contiguous()):
        raise ValueError("cls_contrast: keys must be a contiguous int64 [%d] tensor on %s (got %s %s on %s)"
                         % (B, dev, keys.dtype, tuple(keys.shape), keys.device))
    for name, g in (("da", da), ("dt", dt)):
        if g is not None and (g.dtype != torch.float32 or g.device != dev or g.numel() != B * H or not g.is_contiguous()):
            raise ValueError("cls_contrast: %s must be a contiguous fp32 [%d, %d] tensor on %s" % (name, B, H, dev))
    if hidden_t.dtype != hidden_a.dtype:
        raise ValueError("cls_contrast: hidden_a is %s, hidden_t is %s" % (hidden_a.dtype, hidden_t.dtype))
    nbytes = cls_contrast_ws_bytes(B, H)
    if ws is None:
        ws = _ws(nbytes, dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    check(lib().nbest_cls_contrast(ptr(hidden_a), stride_a, ptr(hidden_t), stride_t, ptr(keys), weight, temperature, ptr(out), ptr(da),
                                   ptr(dt), int(bool(accumulate_dt)), B, H, dtype_code(hidden_a.dtype), ptr(ws),
                                   ws.numel() * ws.element_size(), stream_ptr()), "cls_contrast")
    return out


def cls_grad_scatter(dcls, B, S, H, dtype, out=None):
    dh = out if out is not None else torch.empty(B * S, H, dtype=dtype, device=dcls.device)
    check(lib().nbest_cls_grad_scatter(ptr(dcls), ptr(dh), B, S, H, dtype_code(dtype), stream_ptr()), "cls_grad_scatter")
    return dh


def cast_bf16(src, dst):
    check(lib().nbest_cast_f32_to_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()), "cast_f32_to_bf16")


class LoraTable:
    """an nbest_lora_desc table: ``host`` (ctypes array, tile_start / ws_off filled by nbest_lora_plan), ``dev`` (the same bytes on
    ``device``; None on the CPU), ``n``, ``n_tiles``, ``ws_bytes``.  ``blocks``: dicts with the descriptor's fields (stride defaults
    to cols)."""

    def __init__(self, blocks, device=None, plan=True):
        self.n = len(blocks)
        self.host = (LoraDesc * max(self.n, 1))()
        for d, b in zip(self.host, blocks):
            d.p_off, d.base_off, d.a_off, d.b_off = b["p_off"], b["base_off"], b["a_off"], b["b_off"]
            d.rows, d.cols, d.rank, d.scale = b["rows"], b["cols"], b["rank"], b["scale"]
            d.stride = b.get("stride", b["cols"])
        self.n_tiles, self.ws_bytes = 0, 0
        if plan:
            self.plan()
        self.dev = None
        if device is not None and torch.device(device).type == "cuda":
            self.upload(device)

    def plan(self):
        nt, wb = C.c_int(0), C.c_size_t(0)
        check(lib().nbest_lora_plan(self.host, self.n, C.byref(nt), C.byref(wb)), "lora_plan")
        self.n_tiles, self.ws_bytes = int(nt.value), int(wb.value)

    def upload(self, device):
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)


def lora_merge(p, p_lowp, base, ab, table):
    """every block of ``table``: p = base + scale B A (+ its bf16 copy in ``p_lowp``, or None) - nbest_lora_merge"""
    check(lib().nbest_lora_merge(ptr(p), ptr(p_lowp), ptr(base), ptr(ab), table.host, ptr(table.dev), table.n, stream_ptr()), "lora_merge")


def lora_grad(g, ab, g_ab, table, ws):
    """dA / dB of every block from the dense gradient ``g`` into ``g_ab`` - nbest_lora_grad (``ws``: uint8, >= table.ws_bytes)"""
    check(lib().nbest_lora_grad(ptr(g), ptr(ab), ptr(g_ab), table.host, ptr(table.dev), table.n, ptr(ws), ws.numel(), stream_ptr()),
          "lora_grad")
