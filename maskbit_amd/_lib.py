"""ctypes binding of libmaskbit_hip.so (include/maskbit_hip.h).

There is deliberately NO fallback: if the shared library is missing or fails to load the
product path raises.  (CPU restatements live in ``oracle/`` and are test infrastructure.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmaskbit_hip.so")
ABI_VERSION = 8


class GenCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("bits", "splits", "hidden", "heads", "depth", "mlp", "seq", "nclass", "prenorm", "embed_tables", "precision")]


class DecCfg(C.Structure):
    _fields_ = [("token_size", C.c_int), ("hidden_channels", C.c_int), ("num_resolutions", C.c_int),
                ("num_res_blocks", C.c_int), ("num_channels", C.c_int), ("channel_mult", C.c_int * 8),
                ("latent_size", C.c_int), ("build_encoder", C.c_int), ("sample_with_conv", C.c_int),
                ("enc_res_blocks", C.c_int)]


class SamplePlan(C.Structure):
    _fields_ = [("num_steps", C.c_int), ("use_guidance", C.c_int), ("scale", C.POINTER(C.c_float)),
                ("temperature", C.POINTER(C.c_float)), ("mask_len", C.POINTER(C.c_int)), ("step_begin", C.c_int), ("step_end", C.c_int)]


class EditPlan(C.Structure):
    _fields_ = [("num_steps", C.c_int), ("use_guidance", C.c_int), ("scale", C.POINTER(C.c_float)),
                ("temperature", C.POINTER(C.c_float)), ("mask_ratio", C.POINTER(C.c_float)), ("step_begin", C.c_int), ("step_end", C.c_int)]


class RequestStep(C.Structure):
    """mb_request_step: the constants of one request at one global step (24 bytes; ``step`` = -1: inactive)."""
    _fields_ = [("scale", C.c_float), ("temperature", C.c_float), ("mask_ratio", C.c_float), ("randomize_temperature", C.c_float),
                ("conf_weight", C.c_float), ("step", C.c_int32)]


class RequestPlan(C.Structure):
    _fields_ = [("num_steps", C.c_int), ("use_guidance", C.c_int), ("active", C.POINTER(C.c_int)), ("table", C.c_void_p)]


class SessionRows(C.Structure):
    """mb_session_rows (diagnostic): the per-row device arrays of a sampling session of ``max_active`` rows."""
    _fields_ = [(n, C.c_void_p) for n in ("label", "seed", "num_regen", "slot", "local_step", "N", "pool")] + [("max_active", C.c_int), ("max_steps", C.c_int)]


class ImageJob(C.Structure):
    """mb_image_job: one source of one resampling pass (72 bytes); ``work_offset``, ``kx``, ``ky`` are filled by mb_image_workspace_bytes."""
    _fields_ = ([(n, C.c_int64) for n in ("src_offset", "dst_offset", "work_offset")]
                + [(n, C.c_int32) for n in ("src_h", "src_w", "src_stride", "res_h", "res_w", "win_y", "win_x", "win_h", "win_w", "kx", "ky", "reserved")])


# name -> (restype, argtypes); every symbol include/maskbit_hip.h (the ABI) and include/maskbit_hip_diag.h (single-kernel test entries) declare
SIGNATURES = {
    "mb_gen_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_abi_version": (C.c_int, []),
    "mb_last_error": (C.c_char_p, []),
    "mb_gen_create": (C.c_int, [C.POINTER(GenCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "mb_gen_destroy": (None, [C.c_void_p]),
    "mb_gen_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_gen_set_alo": (C.c_int, [C.c_void_p, C.c_int]),
    "mb_gen_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_gen_forward_cfg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_gen_forward_attn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_sample_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_dec_create": (C.c_int, [C.POINTER(DecCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "mb_dec_destroy": (None, [C.c_void_p]),
    "mb_dec_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_dec_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_dec_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_enc_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_dec_create_vq": (C.c_int, [C.POINTER(DecCfg), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mb_dec_decode_latent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_enc_encode_vq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_vq_argmin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_vq_encode_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 5),
    "mb_vq_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_vq_pack_latent": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_lfq_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_lfq_latent": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mb_pack_image": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mb_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SamplePlan), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_sample_step_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_sample_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(EditPlan), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_sample_step_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_sample_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(EditPlan), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                   C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_sample_step_requests": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_sample_requests": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RequestPlan), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_session_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mb_session_destroy": (None, [C.c_void_p]),
    "mb_session_admit": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "mb_session_due": (C.c_int, [C.c_void_p]),
    "mb_session_active": (C.c_int, [C.c_void_p]),
    "mb_session_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_void_p]),
    "mb_session_row_table": (C.c_int, [C.POINTER(SessionRows), C.c_void_p, C.c_int, C.c_void_p]),
    "mb_session_admit_rows": (C.c_int, [C.POINTER(SessionRows), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_session_retire": (C.c_int, [C.POINTER(SessionRows), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p]),
    "mb_seeded_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p]),
    "mb_edit_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_edit_token_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_edit_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_gemm_ex": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mb_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mb_w4_from_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_w4lo_from_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_gemm_head": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.c_void_p]),
    "mb_cast_f32_to_h16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mb_split_f32_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_layernorm_f4": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_void_p]),
    "mb_layernorm_f4_seq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]),
    "mb_layernorm_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]),
    "mb_pairify": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]),
    "mb_embed_ln": (C.c_int, [C.c_void_p] * 17 + [C.c_int] * 6 + [C.c_void_p]),
    "mb_embed_pair": (C.c_int, [C.c_void_p] * 15 + [C.c_int] * 6 + [C.c_void_p]),
    "mb_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_attention_probs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_attention_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_attention_pair_f4": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_gemm_mini": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "mb_gemm_mini_seq": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "mb_gemm_mini_split": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p), C.c_void_p]),
    "mb_gemm_mini_ln": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 6 + [C.POINTER(C.c_void_p), C.c_void_p]),
    "mb_gemm_act_split": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p]),
    "mb_gemm": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                          C.c_int, C.c_int, C.c_void_p]),
    "mb_conv_layer": (C.c_int, [C.c_void_p] * 13 + [C.POINTER(C.c_int), C.POINTER(C.c_uint)] + [C.c_int] * 8 + [C.c_void_p]),
    "mb_conv_layer_ex": (C.c_int, [C.c_void_p] * 13 + [C.POINTER(C.c_int), C.POINTER(C.c_uint)] + [C.c_int] * 9 + [C.c_void_p]),
    "mb_autoenc_block": (C.c_int, [C.c_void_p] * 11 + [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.POINTER(C.c_uint)] + [C.c_int] * 5 + [C.c_void_p]),
    "mb_groupnorm_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_avgpool2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_s2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_eval_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mb_eval_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_eval_codebook": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_mlm_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mb_mlm_state_bytes": (C.c_size_t, []),
    "mb_mlm_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_mlm_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]),
    "mb_lpips_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mb_lpips_destroy": (None, [C.c_void_p]),
    "mb_lpips_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_lpips_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_lpips_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_conv_relu_layer": (C.c_int, [C.c_void_p] * 4 + [C.POINTER(C.c_uint)] + [C.c_int] * 6 + [C.c_void_p]),
    "mb_maxpool2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_lpips_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_lpips_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mb_lpips_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "mb_fid_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_is_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mb_is_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_manifold_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mb_knn_radii": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_manifold_cover": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "mb_image_workspace_bytes": (C.c_size_t, [C.POINTER(ImageJob), C.c_int, C.c_int]),
    "mb_image_resample": (C.c_int, [C.POINTER(ImageJob), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "mb_image_coeffs": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 4),
    "mb_inception_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mb_inception_destroy": (None, [C.c_void_p]),
    "mb_inception_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_inception_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_inception_forward_spatial": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_inception_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_convbn_layer": (C.c_int, [C.c_void_p] * 5 + [C.POINTER(C.c_uint)] + [C.c_int] * 15 + [C.c_void_p]),
    "mb_pool3": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p]),
    "mb_inception_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_inception_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "mb_bn_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "mb_spatial_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_fc_head": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]),
    "mb_channel_tap": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "mb_inception_folded_bn": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_resnet_folded_bn": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_resnet_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mb_resnet_destroy": (None, [C.c_void_p]),
    "mb_resnet_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_resnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3),
    "mb_resnet_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_convbn_layer_ex": (C.c_int, [C.c_void_p] * 5 + [C.POINTER(C.c_uint)] + [C.c_int] * 16 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mb_pool3_ex": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p]),
    "mb_resnet_input": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "mb_resnet_stem_cols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mb_resnet_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mb_resnet_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7),
    "mb_disc_create": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_void_p)]),
    "mb_disc_destroy": (None, [C.c_void_p]),
    "mb_disc_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_disc_forward": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4),
    "mb_disc_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_convbn_layer_leaky": (C.c_int, [C.c_void_p] * 5 + [C.POINTER(C.c_uint)] + [C.c_int] * 16 + [C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mb_disc_cols": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "mb_disc_down_chunks": (C.c_int, [C.c_int] * 3),
    "mb_disc_downsample": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]),
    "mb_disc_groupnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint)] + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "mb_disc_pool": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "mb_disc_logits": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 2 + [C.c_void_p]),
    "mb_taming_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mb_taming_destroy": (None, [C.c_void_p]),
    "mb_taming_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "mb_taming_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_taming_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_taming_decode_latent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mb_taming_saturation_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "mb_taming_set_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mb_taming_attn_block": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p]),
    "mb_taming_final": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]),
    "mb_taming_pack_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mb_spatial_attention": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "mb_gemm_f32": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]),
    "mb_attention_f32": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "mb_set_cu_count":(C.c_int, [C.c_int]),
    "mb_gen_set_walk": (C.c_int, [C.c_void_p, C.c_int]),
    "mb_diag_set_walk": (C.c_int, [C.c_int]),
    "mb_walk_tile": (C.c_int, [C.c_int] * 3),
    "mb_walk_seq": (C.c_int, [C.c_int] * 4),
    "mb_walk_row": (C.c_int, [C.c_int] * 5),
    "mb_walk_group": (C.c_int, [C.c_int] * 2),
    "mb_gemm_ht_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mb_prof_enable": (C.c_int, [C.c_int]),
    "mb_prof_read": (C.c_int, [C.c_char_p, C.c_int]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load (once) and type the shared library.  torch is imported first so that the HIP runtime
    the library binds to is the one torch already loaded (same SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads libamdhip64 before our DT_NEEDED entry is resolved)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MaskBit HIP kernels are not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (needs hipcc, gfx950). There is no CPU fallback in maskbit_amd.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    v = lib.mb_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"libmaskbit_hip.so ABI {v} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mb_last_error()
        raise RuntimeError(f"{what or 'libmaskbit_hip'} failed (code {rc}): {msg.decode() if msg else '?'}")


def prof_enable(on, every: int = 1) -> None:
    """HIP-event kernel timing on the launch stream; ``every`` = n times the kernels of every n-th generator forward only."""
    load().mb_prof_enable(max(1, int(every)) if on else 0)


def prof_read() -> dict:
    """-> {kernel name: (calls, total_ms)} measured with HIP events on the launch stream."""
    buf = C.create_string_buffer(1 << 16)
    n = load().mb_prof_read(buf, len(buf))
    if n < 0:
        check(n, "mb_prof_read")
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split()
        out[name] = (int(calls), float(ms))
    return out
