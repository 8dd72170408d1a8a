"""ctypes binding of the C-ABI declared in include/mxvl.h (libmxvl.so).

This is the only place Python touches the native library.  Tensors cross the boundary as raw
device pointers + element strides; the stream is torch's current HIP stream (the reference
enqueues on at::cuda::getCurrentCUDAStream(), selective_scan.cpp:232-233).  Loading fails loudly:
there is no fallback implementation anywhere in the package.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int, c_int32, c_int64, c_uint32, c_void_p

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libmxvl.so")
ABI_VERSION = 13

MXVL_F32, MXVL_BF16, MXVL_F16 = 0, 1, 2
MXVL_W_INT8 = 0x100      # mxvl_gemv_desc.dtype flag: W / W2 are int8 codes, w_scale / w2_scale their row-wise absmax
MXVL_W_MXFP4 = 0x200     # mxvl_gemv_desc.dtype flag: W / W2 are packed E2M1 codes (N, K / 2), w_scale / w2_scale their E8M0 block scales (N, K / 32)
MXVL_W_FP8 = 0x800       # mxvl_gemv_desc.dtype flag: W / W2 are OCP E4M3 codes (N, K), w_scale / w2_scale their fp32 row scales (N)
MXVL_W_INT4 = 0x1000     # mxvl_gemv_desc.dtype flag: W / W2 are packed unsigned int4 codes (N, K / 2), w_scale / w2_scale (N, K / 128) words: fp16 group scale | zero point << 16
MXVL_KV_FP8 = 0x400     # mxvl_decode_attn_desc.dtype flag: k_cache / v_cache are OCP E4M3 bytes, kv_scale their two power-of-two scales
MXVL_QK_NORM = 0x2000   # mxvl_decode_attn_desc.dtype flag: the descriptor heads a DecodeAttnQkNormDesc; q / k heads are RMS-normalised in place in qkv
SCAN_DELTA_SOFTPLUS = 1
SCAN_OUT_F32 = 2          # out / dout fp32 whatever io_dtype is (the oflex i16o32 mode)
SCAN_FOLD_BATCH = 4       # the batch folded into the sequence (short rows; ask mxvl_scan_fold_ok)

STATUS = {
    0: "MXVL_OK", -1: "MXVL_ERR_NULL", -2: "MXVL_ERR_DTYPE", -3: "MXVL_ERR_SHAPE", -4: "MXVL_ERR_DSTATE",
    -5: "MXVL_ERR_STRIDE", -6: "MXVL_ERR_LAUNCH", -7: "MXVL_ERR_UNSUPPORTED", -8: "MXVL_ERR_CHECKPOINT",
}
MXVL_ERR_LAUNCH = -6


class ScanDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("dim", c_int32), ("seqlen", c_int32), ("dstate", c_int32), ("n_groups", c_int32),
        ("io_dtype", c_int32), ("flags", c_uint32), ("delta_group_ratio", c_int32),
        ("u_bs", c_int64), ("u_ds", c_int64), ("delta_bs", c_int64), ("delta_ds", c_int64),
        ("z_bs", c_int64), ("z_ds", c_int64), ("out_bs", c_int64), ("out_ds", c_int64),
        ("B_bs", c_int64), ("B_gs", c_int64), ("B_ns", c_int64),
        ("C_bs", c_int64), ("C_gs", c_int64), ("C_ns", c_int64),
        ("A_ds", c_int64), ("A_ns", c_int64),
        ("u", c_void_p), ("delta", c_void_p), ("A", c_void_p), ("B", c_void_p), ("C", c_void_p),
        ("D", c_void_p), ("delta_bias", c_void_p), ("z", c_void_p),
        ("out", c_void_p), ("last_state", c_void_p), ("ckpt", c_void_p),
    ]


class ScanBwdDesc(ctypes.Structure):
    _fields_ = [
        ("fwd", ScanDesc),
        ("dout_bs", c_int64), ("dout_ds", c_int64), ("du_bs", c_int64), ("du_ds", c_int64),
        ("ddelta_bs", c_int64), ("ddelta_ds", c_int64), ("dz_bs", c_int64), ("dz_ds", c_int64),
        ("dB_bs", c_int64), ("dB_gs", c_int64), ("dB_ns", c_int64),
        ("dC_bs", c_int64), ("dC_gs", c_int64), ("dC_ns", c_int64),
        ("dout", c_void_p), ("du", c_void_p), ("ddelta", c_void_p), ("dz", c_void_p),
        ("dA", c_void_p), ("dB", c_void_p), ("dC", c_void_p), ("dD", c_void_p), ("ddelta_bias", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class MambaInnerDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("dim", c_int32), ("seqlen", c_int32), ("dstate", c_int32), ("dt_rank", c_int32), ("width", c_int32),
        ("d_model", c_int32), ("io_dtype", c_int32), ("flags", c_uint32), ("reserved0", c_int32),
        ("xz", c_void_p), ("conv_weight", c_void_p), ("conv_bias", c_void_p), ("x_proj_weight", c_void_p), ("dt_proj_weight", c_void_p),
        ("out_proj_weight", c_void_p), ("out_proj_bias", c_void_p), ("A", c_void_p), ("D", c_void_p), ("delta_bias", c_void_p),
        ("out", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class MambaInnerBwdDesc(ctypes.Structure):
    _fields_ = [
        ("fwd", MambaInnerDesc),
        ("dout", c_void_p), ("dxz", c_void_p), ("dconv_weight", c_void_p), ("dconv_bias", c_void_p),
        ("dx_proj_weight", c_void_p), ("ddt_proj_weight", c_void_p), ("dout_proj_weight", c_void_p), ("dout_proj_bias", c_void_p),
        ("dA", c_void_p), ("dD", c_void_p), ("ddelta_bias", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class AttnDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("n_heads", c_int32), ("n_kv_heads", c_int32), ("seqlen_q", c_int32), ("seqlen_k", c_int32),
        ("head_dim", c_int32), ("io_dtype", c_int32), ("mask_mode", c_int32), ("cluster", c_int32), ("scale", ctypes.c_float),
        ("q_bs", c_int64), ("q_hs", c_int64), ("q_ts", c_int64), ("k_bs", c_int64), ("k_hs", c_int64), ("k_ts", c_int64),
        ("v_bs", c_int64), ("v_hs", c_int64), ("v_ts", c_int64), ("o_bs", c_int64), ("o_hs", c_int64), ("o_ts", c_int64),
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("out", c_void_p), ("lse", c_void_p), ("key_mask", c_void_p),
        ("bias", c_void_p), ("dropout_p", ctypes.c_float), ("dropout_seed", c_uint32),
    ]


class AttnBwdDesc(ctypes.Structure):
    _fields_ = [
        ("fwd", AttnDesc),
        ("dout_bs", c_int64), ("dout_hs", c_int64), ("dout_ts", c_int64), ("dq_bs", c_int64), ("dq_hs", c_int64), ("dq_ts", c_int64),
        ("dk_bs", c_int64), ("dk_hs", c_int64), ("dk_ts", c_int64), ("dv_bs", c_int64), ("dv_hs", c_int64), ("dv_ts", c_int64),
        ("dout", c_void_p), ("dq", c_void_p), ("dk", c_void_p), ("dv", c_void_p), ("delta", c_void_p),
    ]


class Conv1dDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("dim", c_int32), ("seqlen", c_int32), ("width", c_int32),
        ("io_dtype", c_int32), ("silu", c_int32),
        ("x_bs", c_int64), ("x_ds", c_int64), ("y_bs", c_int64), ("y_ds", c_int64),
        ("x", c_void_p), ("weight", c_void_p), ("bias", c_void_p), ("y", c_void_p),
    ]


class Conv1dBwdDesc(ctypes.Structure):
    _fields_ = [
        ("fwd", Conv1dDesc),
        ("dy_bs", c_int64), ("dy_ds", c_int64), ("dx_bs", c_int64), ("dx_ds", c_int64),
        ("dy", c_void_p), ("dx", c_void_p), ("dweight", c_void_p), ("dbias", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class GemvDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("K", c_int32), ("N", c_int32), ("swiglu", c_int32), ("out_f32", c_int32),
        ("eps", ctypes.c_float),
        ("x", c_void_p), ("norm_weight", c_void_p), ("W", c_void_p), ("W2", c_void_p), ("bias", c_void_p),
        ("residual", c_void_p), ("y", c_void_p), ("split_acc", c_void_p), ("k_splits", c_int32), ("dtype", c_int32),
        ("norm_gain_scale", ctypes.c_float),
        ("w_scale", c_void_p), ("w2_scale", c_void_p),
    ]


class RmsNormDesc(ctypes.Structure):
    _fields_ = [("rows", c_int32), ("K", c_int32), ("eps", ctypes.c_float), ("x", c_void_p), ("weight", c_void_p), ("y", c_void_p),
                ("acc", c_void_p), ("residual", c_void_p), ("x_out", c_void_p), ("dtype", c_int32), ("acc_splits", c_int32)]


class RopeDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("seqlen", c_int32), ("n_q_heads", c_int32), ("n_k_heads", c_int32), ("head_dim", c_int32),
        ("io_dtype", c_int32), ("cs_dtype", c_int32), ("backward", c_int32),
        ("q_bs", c_int64), ("q_ts", c_int64), ("q_hs", c_int64), ("k_bs", c_int64), ("k_ts", c_int64), ("k_hs", c_int64),
        ("qo_bs", c_int64), ("qo_ts", c_int64), ("qo_hs", c_int64), ("ko_bs", c_int64), ("ko_ts", c_int64), ("ko_hs", c_int64),
        ("cs_bs", c_int64), ("cs_ts", c_int64),
        ("q", c_void_p), ("k", c_void_p), ("cos", c_void_p), ("sin", c_void_p), ("q_out", c_void_p), ("k_out", c_void_p),
    ]


class RmsTrainDesc(ctypes.Structure):
    _fields_ = [("rows", c_int32), ("cols", c_int32), ("x_dtype", c_int32), ("w_dtype", c_int32), ("y_dtype", c_int32),
                ("eps", ctypes.c_float), ("x", c_void_p), ("weight", c_void_p), ("grad", c_void_p), ("y", c_void_p), ("rstd", c_void_p)]


class DecodeAttnDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("n_heads", c_int32), ("n_kv_heads", c_int32), ("head_dim", c_int32), ("max_len", c_int32),
        ("scale", ctypes.c_float),
        ("qkv", c_void_p), ("cos", c_void_p), ("sin", c_void_p), ("k_cache", c_void_p), ("v_cache", c_void_p),
        ("slot_table", c_void_p), ("pos", c_void_p), ("mask", c_void_p), ("out", c_void_p), ("q_rope", c_void_p),
        ("beams", c_int32), ("dtype", c_int32),
        ("kv_scale", c_void_p),
    ]


class DecodeAttnQkNormDesc(ctypes.Structure):
    """mxvl_decode_attn_qknorm_desc: what mxvl_decode_attn reads through its descriptor pointer when attn.dtype carries MXVL_QK_NORM"""
    _fields_ = [("attn", DecodeAttnDesc), ("q_norm_weight", c_void_p), ("k_norm_weight", c_void_p), ("qk_norm_eps", ctypes.c_float)]


GATE_TANH, GATE_WARM_TANH = 1, 2


class DecodeCrossAttnDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("n_heads", c_int32), ("n_kv_heads", c_int32), ("head_dim", c_int32), ("n_keys", c_int32),
        ("kv_rows_div", c_int32), ("gate_flags", c_int32), ("scale", ctypes.c_float),
        ("q_rope", c_void_p), ("k", c_void_p), ("v", c_void_p), ("key_mask", c_void_p), ("row_on", c_void_p),
        ("text_state", c_void_p), ("gate_weight", c_void_p), ("gate_bias", c_void_p), ("warm_up_gate", c_void_p),
        ("out", c_void_p), ("dtype", c_int32), ("reserved0", c_int32),
    ]


class DecodePrologueDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("hidden", c_int32), ("max_len", c_int32), ("head_dim", c_int32), ("prompt_len", c_int32),
        ("table_len", c_int32),
        ("tok", c_void_p), ("beam_src", c_void_p), ("cur", c_void_p), ("n_real", c_void_p), ("embed", c_void_p),
        ("cos_table", c_void_p), ("sin_table", c_void_p), ("slot_table", c_void_p), ("mask", c_void_p), ("x", c_void_p),
        ("cos", c_void_p), ("sin", c_void_p), ("pos", c_void_p),
    ]


class AddLnDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("cols", c_int32), ("res_dtype", c_int32), ("branch_dtype", c_int32), ("out_dtype", c_int32),
        ("eps", ctypes.c_float),
        ("x", c_void_p), ("branch", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
        ("h", c_void_p), ("n", c_void_p), ("mean", c_void_p), ("rstd", c_void_p),
    ]


class GemmSwigluDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_int32), ("K", c_int32), ("H", c_int32), ("io_dtype", c_int32), ("bias_dtype", c_int32),
        ("x_rs", c_int64), ("w_rs", c_int64), ("ab_rs", c_int64), ("h_rs", c_int64),
        ("x", c_void_p), ("weight", c_void_p), ("bias", c_void_p), ("ab", c_void_p), ("h", c_void_p),
    ]


class GemmNtDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_int32), ("K", c_int32), ("N", c_int32), ("io_dtype", c_int32), ("bias_dtype", c_int32), ("reserved0", c_int32),
        ("a_rs", c_int64), ("b_rs", c_int64), ("c_rs", c_int64),
        ("a", c_void_p), ("b", c_void_p), ("bias", c_void_p), ("c", c_void_p),
    ]


class GemmTnDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_int32), ("N", c_int32), ("K", c_int32), ("io_dtype", c_int32), ("accumulate", c_int32), ("slices_per_xcd", c_int32),
        ("a_rs", c_int64), ("b_rs", c_int64), ("c_rs", c_int64),
        ("a", c_void_p), ("b", c_void_p), ("c", c_void_p),
    ]


class GemmSwigluBwdDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_int32), ("K", c_int32), ("H", c_int32), ("io_dtype", c_int32),
        ("dy_rs", c_int64), ("w_rs", c_int64), ("ab_rs", c_int64), ("dab_rs", c_int64),
        ("dy", c_void_p), ("w3t", c_void_p), ("ab", c_void_p), ("dab", c_void_p), ("partial", c_void_p),
    ]


class AddLnBwdDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("cols", c_int32), ("res_dtype", c_int32), ("branch_dtype", c_int32), ("out_dtype", c_int32),
        ("n_partials", c_int32),
        ("dn", c_void_p), ("dh", c_void_p), ("h", c_void_p), ("gamma", c_void_p), ("mean", c_void_p), ("rstd", c_void_p),
        ("dx", c_void_p), ("dbranch", c_void_p), ("partial_dgamma", c_void_p), ("partial_dbeta", c_void_p),
        ("partial_dbranch", c_void_p),
    ]


class DirPermDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("dim", c_int32), ("seqlen", c_int32), ("padded_len", c_int32), ("n_dirs", c_int32), ("io_dtype", c_int32),
        ("rows_bs", c_int64), ("rows_ds", c_int64), ("stacked_bs", c_int64), ("stacked_ks", c_int64), ("stacked_ds", c_int64),
        ("index", c_void_p), ("rows", c_void_p), ("stacked", c_void_p),
        ("gate", c_void_p), ("pre", c_void_p), ("dgate", c_void_p),
        ("gate_bs", c_int64), ("gate_ds", c_int64), ("pre_bs", c_int64), ("pre_ds", c_int64), ("dgate_bs", c_int64), ("dgate_ds", c_int64),
        ("gate_scale", ctypes.c_float), ("reserved0", c_int32),
    ]


class BeamDesc(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("beams", c_int32), ("vocab", c_int32), ("max_new", c_int32), ("min_new", c_int32), ("n_eos", c_int32),
        ("early_stopping", c_int32), ("keep", c_int32),
        ("repetition_penalty", ctypes.c_float), ("no_repeat_ngram_size", c_int32),
        ("logits", c_void_p), ("run_seq", c_void_p), ("fin_seq", c_void_p), ("run_score", c_void_p), ("fin_score", c_void_p),
        ("fin_done", c_void_p), ("heur_open", c_void_p), ("cur", c_void_p), ("eos", c_void_p), ("len_tab", c_void_p),
        ("hyp_tab", c_void_p), ("tok", c_void_p), ("beam_src", c_void_p), ("unfinished", c_void_p), ("scratch", c_void_p),
        ("unfinished_log", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class SampleDesc(ctypes.Structure):
    _fields_ = [
        ("rows", c_int32), ("vocab", c_int32), ("max_new", c_int32), ("min_new", c_int32), ("n_eos", c_int32), ("top_k", c_int32),
        ("repetition_penalty", ctypes.c_float), ("temperature", ctypes.c_float), ("top_p", ctypes.c_float),
        ("no_repeat_ngram_size", c_int32),
        ("fill", c_int64),
        ("logits", c_void_p), ("seq", c_void_p), ("alive", c_void_p), ("tok", c_void_p), ("cur", c_void_p), ("eos", c_void_p),
        ("seed", c_void_p), ("unfinished", c_void_p), ("unfinished_log", c_void_p), ("scratch", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64), ("out_thresh", c_void_p), ("out_kept", c_void_p),
    ]


class ImageDesc(ctypes.Structure):
    _fields_ = [
        ("in_h", c_int32), ("in_w", c_int32), ("out_h", c_int32), ("out_w", c_int32),
        ("ksize_h", c_int32), ("ksize_v", c_int32), ("out_dtype", c_int32), ("flags", c_int32),
        ("src", c_void_p), ("bounds_h", c_void_p), ("kk_h", c_void_p), ("bounds_v", c_void_p), ("kk_v", c_void_p),
        ("lut", c_void_p), ("tmp", c_void_p), ("out", c_void_p),
        ("src_pitch", c_int64), ("batch", c_int32), ("reserved1", c_int32), ("items", c_void_p),
    ]


MXVL_IMG_FLIP_H, MXVL_IMG_GRAY = 1, 2


class ImageItem(ctypes.Structure):
    """mxvl_image_item: one image of a batched mxvl_image_preprocess call (a record of the device array ImageDesc.items names)."""
    _fields_ = [
        ("src", c_void_p), ("src_pitch", c_int64), ("in_h", c_int32), ("in_w", c_int32), ("ksize_h", c_int32), ("ksize_v", c_int32),
        ("flags", c_int32), ("reserved0", c_int32),
        ("bounds_h", c_void_p), ("kk_h", c_void_p), ("bounds_v", c_void_p), ("kk_v", c_void_p), ("tmp", c_void_p),
    ]


_P, _I, _I64 = c_void_p, c_int, c_int64
_DESC = (_I, [_P, _P])        # (const mxvl_*_desc* desc, void* hip_stream)

# every function include/mxvl.h declares: name -> (restype, argtypes).  load() applies it; tests/test_abi.py holds it to the header's
# prototypes (arity and type class per parameter) and checks the .so exports every name
SIGNATURES = {
    "mxvl_abi_version": (_I, []),
    "mxvl_last_hip_error": (_I, []),
    # selective scan
    "mxvl_scan_chunk_len": (_I, [_I, _I]),
    "mxvl_scan_n_chunks": (_I, [_I, _I]),
    "mxvl_scan_fold_ok": (_I, [_I, _I, _I]),
    "mxvl_scan_fold_slots": (_I, [_I, _I, _I, _I]),
    "mxvl_scan_fwd": _DESC,
    "mxvl_scan_bwd": _DESC,
    "mxvl_scan_bwd_workspace_bytes": (_I64, [_P]),
    "mxvl_set_scan_variant": (None, [_I]),
    "mxvl_last_scan_kernel": (ctypes.c_char_p, []),
    "mxvl_last_scan_bwd_kernel": (ctypes.c_char_p, []),
    "mxvl_state_update": (_I, [_P] * 10 + [_I] * 5 + [_P]),
    # causal conv1d
    "mxvl_conv1d_fwd": _DESC,
    "mxvl_conv1d_bwd": _DESC,
    "mxvl_conv1d_bwd_workspace_bytes": (_I64, [_P]),
    "mxvl_conv1d_update": (_I, [_P] * 5 + [_I] * 5 + [_P]),
    # fused Mamba inner block
    "mxvl_mamba_inner_fwd": _DESC,
    "mxvl_mamba_inner_bwd": _DESC,
    "mxvl_mamba_inner_workspace_bytes": (_I64, [ctypes.POINTER(MambaInnerDesc)]),       # typed: ctypes passes a descriptor by reference
    "mxvl_mamba_inner_bwd_workspace_bytes": (_I64, [ctypes.POINTER(MambaInnerDesc)]),
    # report decoder
    "mxvl_decode_gemv": _DESC,
    "mxvl_decode_gemm_plan": (_I, [ctypes.POINTER(GemvDesc), ctypes.POINTER(c_int32)]),
    "mxvl_set_decode_gemm_wide": (_I, [_I]),
    "mxvl_set_deterministic": (_I, [_I]),
    "mxvl_decode_attn": _DESC,
    "mxvl_decode_cross_attn": _DESC,
    "mxvl_decode_prologue": _DESC,
    "mxvl_decode_rmsnorm": _DESC,
    "mxvl_beam_step": _DESC,
    "mxvl_beam_workspace_bytes": (_I64, [_I] * 3),
    "mxvl_sample_step": _DESC,
    "mxvl_sample_workspace_bytes": (_I64, [_I] * 2),
    # VMamba / VisionMamba
    "mxvl_cross_scan": (_I, [_P, _P] + [_I] * 5 + [_P]),
    "mxvl_cross_merge": (_I, [_P, _P] + [_I] * 5 + [_P]),
    "mxvl_dir_gather": _DESC,
    "mxvl_dir_merge": _DESC,
    "mxvl_dwconv2d_fwd": (_I, [_P] * 4 + [_I] * 7 + [_P]),
    "mxvl_dwconv2d_bwd": (_I, [_P] * 7 + [_I] * 7 + [_P]),
    "mxvl_window_cols": (_I, [_P] * 3 + [_I] * 8 + [_P]),
    # norms, MLP, GEMMs
    "mxvl_add_layernorm_fwd": _DESC,
    "mxvl_add_layernorm_bwd": _DESC,
    "mxvl_add_layernorm_partials": (_I, [_I]),
    "mxvl_swiglu_fwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "mxvl_swiglu_bwd": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "mxvl_swiglu_partials": (_I, [_I, _I]),
    "mxvl_swiglu_bwd_colsum": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mxvl_gemm_swiglu_fwd": _DESC,
    "mxvl_gemm_swiglu_bwd": _DESC,
    "mxvl_gemm_swiglu_bwd_partials": (_I, [_I]),
    "mxvl_gemm_nt": _DESC,
    "mxvl_gemm_tn": _DESC,
    "mxvl_colsum": (_I, [_P, _P, _I, _I, _I64, _I, _I, _P]),
    "mxvl_colsum_partials": (_I, [_I, _I]),
    "mxvl_rope": _DESC,
    "mxvl_rmsnorm_train_fwd": _DESC,
    "mxvl_rmsnorm_train_bwd": _DESC,
    "mxvl_silu_mul": (_I, [_P] * 5 + [_I64, _I, _P]),
    "mxvl_attn_fwd": _DESC,
    "mxvl_attn_bwd": _DESC,
    # pre-training and image input
    "mxvl_row_gather": (_I, [_P] * 5 + [_I] * 4 + [_I64] * 2 + [_I] * 2 + [_P]),
    "mxvl_patch_loss": (_I, [_P] * 5 + [_I] * 6 + [_P]),
    "mxvl_patch_cols": (_I, [_P] * 2 + [_I] * 7 + [_P]),
    "mxvl_clip_loss": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mxvl_resample_ksize": (_I, [_I, _I, _I]),
    "mxvl_resample_coeffs": (_I, [_I, _I, _I, _P, _P]),
    "mxvl_image_preprocess": _DESC,
}
SYMBOLS = list(SIGNATURES)


_lib = None


def load() -> ctypes.CDLL:
    """dlopen libmxvl.so; raises (never falls back) when it is absent or its ABI is stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m medical_image_analysis_amd.build` "
            "(hipcc, gfx950). medical_image_analysis_amd has no CPU / PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.mxvl_abi_version.restype = c_int
    if lib.mxvl_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libmxvl.so ABI {lib.mxvl_abi_version()} != binding ABI {ABI_VERSION}: rebuild")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return MXVL_F32
    if dt == torch.bfloat16:
        return MXVL_BF16
    if dt == torch.float16:
        return MXVL_F16
    raise RuntimeError(f"mxvl: io dtype must be float32/bfloat16/float16, got {dt}")  # selective_scan.cpp:167


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def sizeof(struct) -> int:
    return ctypes.sizeof(struct)


def array_in(struct, count: int, buffer):
    """`count` records of `struct` laid over the first bytes of a writable host buffer (a pinned staging array): what the caller
    fills is what the device reads after the upload.  The records hold the buffer; drop them before it goes away."""
    return (struct * count).from_buffer(buffer)


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(*tensors) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("mxvl: expected a HIP device tensor (no CPU path exists); got a CPU tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("mxvl: tensors live on different devices")
    return dev


def check(rc: int, what: str) -> None:
    if rc != 0:
        # the thread's last hipError belongs to this call only when it failed a launch; a validation failure did not touch HIP
        hip = f" (hipError {load().mxvl_last_hip_error()})" if rc == MXVL_ERR_LAUNCH else ""
        raise RuntimeError(f"{what} failed: {STATUS.get(rc, rc)}{hip}")


# Deterministic mode (include/mxvl.h mxvl_set_deterministic).  _det_mode: what set_deterministic() asked for (None = follow torch);
# _det_lib: what the library was last told (it starts at 0).  launch() brings the two in step before it calls an entry.
_det_mode = None
_det_lib = 0


def set_deterministic(mode) -> None:
    """True / False: libmxvl's deterministic mode on / off; None (the default): follow torch.are_deterministic_algorithms_enabled()
    at each call.  With the mode on every fp32-accumulated gradient of the hand-written kernels is bit-identical from run to run
    (same inputs, shapes, strides, build and device model); vendor GEMMs, RCCL and torch's own ops are outside the guarantee.
    Under the mode mxvl_gemm_tn and the composed mxvl_mamba_inner_bwd refuse (MXVL_ERR_UNSUPPORTED): splitk_wgrad takes the library's
    plane-sum form by itself, mamba_inner_fn_native's backward raises.  When the mode comes from torch.use_deterministic_algorithms(True),
    torch also fills every torch.empty (torch.utils.deterministic.fill_uninitialized_memory), the slot workspaces included."""
    global _det_mode
    if mode is not None and not isinstance(mode, bool):
        raise TypeError("set_deterministic: mode must be True, False or None")
    _det_mode = mode


def is_deterministic() -> bool:
    """The mode the next libmxvl call runs in."""
    return torch.are_deterministic_algorithms_enabled() if _det_mode is None else _det_mode


def sync_deterministic() -> bool:
    """Tell the library the current mode if it changed since the last call (an int compare otherwise); returns the mode.  The
    callers that size a workspace by the mode (scan / conv1d backward) call it before they ask the library for the size."""
    global _det_lib
    want = 1 if is_deterministic() else 0
    if want != _det_lib:
        (_lib or load()).mxvl_set_deterministic(want)
        _det_lib = want
    return bool(want)


def det_workspace_bytes(name: str, desc) -> int:
    """Bytes of slot workspace the backward entry behind query `name` (mxvl_scan_bwd_workspace_bytes(fwd descriptor) /
    mxvl_conv1d_bwd_workspace_bytes(descriptor)) needs in the mode the next call runs in: 0 with deterministic mode off."""
    if not sync_deterministic():
        return 0
    nbytes = int(getattr(_lib or load(), name)(ctypes.byref(desc)))
    if nbytes < 0:
        raise RuntimeError(f"{name}: invalid descriptor")
    return nbytes


def launch(name: str, first, *rest, device) -> None:
    """The one way the package enqueues a libmxvl kernel: entry `name` (one whose prototype ends in `void *hip_stream`) on
    `device`'s current stream, with `device` current -- libmxvl's hipFuncSetAttribute calls act on the current device -- and a
    non-zero status raised by check().  A descriptor is an entry's first parameter (include/mxvl.h) and goes by reference; the
    other arguments pass as they are.  A name libmxvl does not export raises before anything is called."""
    fn = getattr(_lib or load(), name)
    sync_deterministic()
    with torch.cuda.device(device):
        rc = fn(ctypes.byref(first) if isinstance(first, ctypes.Structure) else first, *rest, stream_ptr(device))
    check(rc, name)
