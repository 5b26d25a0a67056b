"""ctypes binding of libtld_hip.so (the C ABI declared in include/tld_hip.h).

The library is built in-tree by ``csrc/Makefile`` (``__graft_entry__.build()``).  There is no
fallback: if the shared object is missing or a call fails, a RuntimeError carrying
``tld_last_error()`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TLD_LIB", os.path.join(_HERE, "libtld_hip.so"))   # TLD_LIB: A/B-testing builds only

DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
DTYPE_U8 = 3                             # TLD_DTYPE_U8: quantised latents of a tld_batch_source

TRAIN_OPT_STATE_DOUBLES = 8 + 1024         # TLD_TRAIN_OPT_STATE_DOUBLES (include/tld_hip.h): the guarded optimizer step's fp64 state vector

KERNEL_CLASSES = ("gemm_qkv", "gemm_up", "gemm_down", "attention", "cross_row", "dwconv_gelu", "layernorm",
                  "embed", "tail", "update", "conditioning")

# every symbol include/tld_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "tld_engine_create", "tld_engine_load_tensor", "tld_engine_finalize_weights", "tld_denoiser_forward",
    "tld_sample", "tld_sample_from", "tld_sample_requests", "tld_sample_requests_guided", "tld_sample_requests_stochastic", "tld_debug_sampler_noise", "tld_sample_requests_shaped", "tld_debug_guidance_shape", "tld_engine_sample_rows", "tld_engine_set_gemm_dtype", "tld_engine_set_low_latency", "tld_debug_gemm_splitk", "tld_debug_quant_mx8", "tld_debug_quant_mx8_host", "tld_debug_gemm_mx8",
    "tld_engine_param_count", "tld_engine_refresh_weights", "tld_debug_quant_mx8_f32",
    "tld_session_open", "tld_session_admit", "tld_session_step", "tld_session_latent", "tld_session_copy_latent", "tld_session_stats", "tld_session_close",
    "tld_debug_decode_stage", "tld_engine_set_debug", "tld_engine_read_stage", "tld_engine_stage_shape", "tld_engine_set_debug_step", "tld_engine_debug_paths", "tld_debug_gemm_bf16", "tld_debug_gemm_bench", "tld_debug_gemm_plan", "tld_debug_qkv_pair_plan", "tld_debug_gemm_epilogue",
    "tld_engine_set_profile", "tld_engine_profile_reserve", "tld_engine_get_profile", "tld_engine_weight_bytes", "tld_engine_destroy",
    "tld_vae_create", "tld_vae_load_tensor", "tld_vae_finalize_weights", "tld_vae_decode", "tld_vae_set_debug",
    "tld_vae_read_stage", "tld_vae_set_profile", "tld_vae_get_profile", "tld_debug_conv3x3", "tld_vae_weight_bytes",
    "tld_vae_destroy",
    "tld_vae_enc_create", "tld_vae_enc_load_tensor", "tld_vae_enc_finalize_weights", "tld_vae_enc_encode", "tld_vae_enc_set_debug",
    "tld_vae_enc_read_stage", "tld_vae_enc_set_profile", "tld_vae_enc_get_profile", "tld_vae_enc_weight_bytes", "tld_vae_enc_destroy",
    "tld_debug_conv3x3_s2",
    "tld_clip_create", "tld_clip_load_tensor", "tld_clip_finalize_weights", "tld_clip_encode_text", "tld_clip_set_debug", "tld_clip_read_stage", "tld_clip_weight_bytes",
    "tld_clip_destroy",
    "tld_clip_vis_create", "tld_clip_vis_load_tensor", "tld_clip_vis_finalize_weights", "tld_clip_vis_encode_image", "tld_clip_vis_set_debug", "tld_clip_vis_read_stage",
    "tld_clip_vis_weight_bytes", "tld_clip_vis_destroy", "tld_debug_clip_vis_attention",
    "tld_train_create", "tld_train_param_count", "tld_train_tensor_count", "tld_train_param_layout", "tld_train_set_angular_speeds", "tld_train_bind",
    "tld_train_refresh_weights", "tld_train_forward_backward", "tld_train_forward_backward_cb", "tld_train_adam_ema", "tld_train_grad_guard", "tld_train_adam_ema_guarded",
    "tld_opt_plan_create", "tld_opt_plan_destroy", "tld_opt_plan_numel", "tld_opt_plan_segment_sqsums", "tld_train_grad_guard_grouped", "tld_train_adamw_ema_grouped",
    "tld_train_prepare_batch", "tld_train_prepare_batch_at",
    "tld_train_forward_loss", "tld_train_sample_loss", "tld_train_loss_buckets", "tld_debug_attention_bwd", "tld_debug_wgrad", "tld_debug_attention_fwd", "tld_debug_dwconv_gelu",
    "tld_train_set_debug", "tld_train_read_stage", "tld_train_debug_paths", "tld_train_destroy",
    "tld_feat_append", "tld_feat_moments", "tld_feat_kernel_sum_partials", "tld_feat_kernel_sum",
    "tld_last_error",
)

VAE_KERNEL_CLASSES = ("conv3x3", "gemm", "groupnorm", "other")


# void (*tld_grad_ready_fn)(void* user, int64_t offset, int64_t numel)   (include/tld_hip.h: tld_train_forward_backward_cb)
GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)


class TldConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("image_size", "noise_embed_dims", "patch_size", "embed_dim", "n_layers",
                                         "text_emb_size", "n_channels", "mlp_multiplier", "max_batch",
                                         "device_id")]


class TldSampleRequest(C.Structure):
    """tld_sample_request (include/tld_hip.h): one request's scalars of a tld_sample_requests call."""
    _fields_ = [("n_levels", C.c_int32), ("class_guidance", C.c_float), ("start_mix", C.c_float), ("has_negative", C.c_int32)]


class TldSessionRequest(C.Structure):
    """tld_session_request (include/tld_hip.h): one request of tld_session_admit; host arrays, then device pointers."""
    _fields_ = [("n_levels", C.c_int32), ("class_guidance", C.c_float), ("has_negative", C.c_int32), ("reserved", C.c_int32),
                ("coeffs", C.POINTER(C.c_float)), ("guidance", C.POINTER(C.c_float)), ("noise_coeff", C.POINTER(C.c_float)),
                ("noise_key", C.POINTER(C.c_uint64)), ("noise", C.c_void_p), ("label", C.c_void_p), ("neg_label", C.c_void_p)]


class TldVaeConfig(C.Structure):
    _fields_ = [("latent_channels", C.c_int32), ("out_channels", C.c_int32), ("n_blocks", C.c_int32),
                ("block_out_channels", C.c_int32 * 4), ("layers_per_block", C.c_int32), ("norm_num_groups", C.c_int32),
                ("mid_block_attention", C.c_int32), ("use_post_quant_conv", C.c_int32), ("latent_size", C.c_int32),
                ("max_batch", C.c_int32), ("device_id", C.c_int32)]


class TldVaeEncConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("latent_channels", C.c_int32), ("n_blocks", C.c_int32),
                ("block_out_channels", C.c_int32 * 4), ("layers_per_block", C.c_int32), ("norm_num_groups", C.c_int32),
                ("mid_block_attention", C.c_int32), ("use_quant_conv", C.c_int32), ("image_size", C.c_int32),
                ("max_batch", C.c_int32), ("device_id", C.c_int32)]


class TldBatchSource(C.Structure):
    """tld_batch_source (include/tld_hip.h): the resident dataset a tld_train_prepare_batch call gathers from."""
    _fields_ = [("latents", C.c_void_p), ("labels", C.c_void_p), ("dequant_table", C.c_void_p), ("rows", C.c_int64),
                ("latent_dtype", C.c_int32), ("label_dtype", C.c_int32), ("latent_elems", C.c_int32), ("text_emb", C.c_int32),
                ("vae_scale", C.c_float)]


class TldOptGroup(C.Structure):
    """tld_opt_group (include/tld_hip.h): one parameter group of a tld_opt_plan."""
    _fields_ = [("lr_scale", C.c_float), ("weight_decay", C.c_float), ("frozen", C.c_int32), ("reserved", C.c_int32)]


class TldClipConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "context_length", "width", "heads", "layers", "embed_dim", "max_batch",
                                         "device_id")]


class TldClipVisConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("image_size", "patch_size", "width", "heads", "layers", "embed_dim", "max_batch", "device_id")]


class TldGemmEpilogueArgs(C.Structure):
    """tld_gemm_epilogue_args (include/tld_hip.h): one GEMM launch with any non-conv epilogue, for tld_debug_gemm_epilogue."""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "W", "a_scale", "w_scale", "bias", "out_bf16", "vt", "resid", "stats_out", "ln_stats", "ln_c1", "ln_b1",
                                           "row_stats", "c_f32")] +
                [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldw", "epilogue", "f8", "ldo", "ntok", "d", "ldr", "ln_slots", "ldc", "w_batch_rows")] +
                [("w_batch_stride_bytes", C.c_uint32)])


_lib = None


def build(verbose: bool = False) -> None:
    """Compile libtld_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode:
        print(r.stdout)
    if r.returncode:
        raise RuntimeError("building libtld_hip.so failed")


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP engine is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C transformer_latent_diffusion_amd/csrc`). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64p = C.c_void_p, C.c_int32, C.POINTER(C.c_int64)
    L.tld_last_error.restype = C.c_char_p
    L.tld_engine_create.argtypes = [C.POINTER(TldConfig), C.POINTER(vp)]
    L.tld_engine_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
    L.tld_engine_finalize_weights.argtypes = [vp]
    L.tld_denoiser_forward.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.tld_sample.argtypes = [vp, vp, vp, C.POINTER(C.c_float), i32, C.c_float, C.c_float, C.c_float, vp, i32,
                             vp, vp, vp]
    if hasattr(L, "tld_sample_from"):                # (absent from A/B builds that predate image-to-image)
        L.tld_sample_from.argtypes = [vp, vp, vp, vp, C.c_float, vp, C.POINTER(C.c_float), i32, C.c_float, C.c_float, C.c_float, vp, i32,
                                      vp, vp, vp]
    if hasattr(L, "tld_sample_requests"):            # (absent from A/B builds that predate it)
        L.tld_sample_requests.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(TldSampleRequest), C.POINTER(C.c_float), i32, C.c_float, C.c_float, vp, i32,
                                          vp, vp, vp]
    if hasattr(L, "tld_sample_requests_guided"):     # (absent from A/B builds that predate per-step guidance)
        L.tld_sample_requests_guided.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(TldSampleRequest), C.POINTER(C.c_float), C.POINTER(C.c_float), i32,
                                                 C.c_float, C.c_float, vp, i32, vp, vp, vp]
        L.tld_engine_sample_rows.argtypes = [vp, i64p, i64p]
    if hasattr(L, "tld_sample_requests_stochastic"):     # (absent from A/B builds that predate the stochastic sampler)
        L.tld_sample_requests_stochastic.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(TldSampleRequest), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                     C.POINTER(C.c_float), C.POINTER(C.c_uint64), i32, C.c_float, C.c_float, vp, i32, vp, vp, vp]
        L.tld_debug_sampler_noise.argtypes = [vp, vp, i32, i32, vp, vp]
    if hasattr(L, "tld_sample_requests_shaped"):         # (absent from A/B builds that predate the shaped guidance update)
        L.tld_sample_requests_shaped.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(TldSampleRequest), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                 C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_float), i32, C.c_float, C.c_float, vp, i32,
                                                 vp, vp, vp]
        L.tld_debug_guidance_shape.argtypes = [vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i32, i32, vp, vp, vp, vp]
    if hasattr(L, "tld_session_open"):               # (absent from A/B builds that predate sampler sessions)
        L.tld_session_open.argtypes = [vp, i32, i32, C.c_float, C.c_float, vp, C.POINTER(vp)]
        L.tld_session_admit.argtypes = [vp, C.POINTER(TldSessionRequest), vp, C.POINTER(i32)]
        L.tld_session_step.argtypes = [vp, vp, C.POINTER(i32), i32, C.POINTER(i32)]
        L.tld_session_latent.argtypes = [vp, i32, C.POINTER(vp)]
        L.tld_session_copy_latent.argtypes = [vp, i32, vp, vp]
        L.tld_session_stats.argtypes = [vp, i64p]
        L.tld_session_close.argtypes = [vp]
    L.tld_engine_set_gemm_dtype.argtypes = [vp, i32]
    L.tld_engine_set_low_latency.argtypes = [vp, i32]
    L.tld_debug_gemm_splitk.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.tld_debug_quant_mx8.argtypes = [vp, vp, vp, i32, i32, vp]
    L.tld_debug_quant_mx8_host.argtypes = [C.POINTER(C.c_float), i32, i32, vp, vp]
    L.tld_debug_gemm_mx8.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    if hasattr(L, "tld_engine_refresh_weights"):     # (absent from A/B builds that predate the device weight refresh)
        L.tld_engine_param_count.argtypes = [vp]
        L.tld_engine_param_count.restype = C.c_int64
        L.tld_engine_refresh_weights.argtypes = [vp, vp, C.c_int64, vp]
        L.tld_debug_quant_mx8_f32.argtypes = [vp, vp, vp, i32, i32, vp]
    if hasattr(L, "tld_debug_decode_stage"):         # (absent from A/B builds that predate the shared stage store)
        L.tld_debug_decode_stage.argtypes = [vp, vp, i32, i32, i64p, C.c_int64, i32, i32, C.POINTER(C.c_float), C.c_int64]
    L.tld_engine_set_debug.argtypes = [vp, i32]
    L.tld_engine_read_stage.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int64]
    if hasattr(L, "tld_engine_stage_shape"):         # (absent from A/B builds that predate the per-block stage hook)
        L.tld_engine_stage_shape.argtypes = [vp, C.c_char_p, i64p]
        L.tld_engine_set_debug_step.argtypes = [vp, i32]
        L.tld_engine_debug_paths.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.tld_debug_gemm_bf16.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.tld_debug_gemm_bench.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(C.c_double)]
    if hasattr(L, "tld_debug_gemm_plan"):            # (absent from A/B builds that predate it)
        L.tld_debug_gemm_plan.argtypes = [vp, i32, vp]
    if hasattr(L, "tld_debug_qkv_pair_plan"):
        L.tld_debug_qkv_pair_plan.argtypes = [vp, i32, vp, vp]
    if hasattr(L, "tld_debug_gemm_epilogue"):
        L.tld_debug_gemm_epilogue.argtypes = [C.POINTER(TldGemmEpilogueArgs), vp]
    L.tld_engine_set_profile.argtypes = [vp, C.c_uint32]
    L.tld_engine_profile_reserve.argtypes = [vp, i32, C.c_int64]
    L.tld_engine_get_profile.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.tld_engine_weight_bytes.argtypes = [vp]
    L.tld_engine_weight_bytes.restype = C.c_int64
    L.tld_engine_destroy.argtypes = [vp]
    L.tld_vae_create.argtypes = [C.POINTER(TldVaeConfig), C.POINTER(vp)]
    L.tld_vae_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
    L.tld_vae_finalize_weights.argtypes = [vp]
    L.tld_vae_decode.argtypes = [vp, vp, vp, i32, i32, vp]
    L.tld_vae_set_debug.argtypes = [vp, i32]
    L.tld_vae_read_stage.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int64, i64p]
    L.tld_vae_set_profile.argtypes = [vp, i32]
    L.tld_vae_get_profile.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.tld_debug_conv3x3.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.tld_vae_weight_bytes.argtypes = [vp]
    L.tld_vae_weight_bytes.restype = C.c_int64
    L.tld_vae_destroy.argtypes = [vp]
    if hasattr(L, "tld_vae_enc_create"):             # (absent from A/B builds that predate the encoder)
        L.tld_vae_enc_create.argtypes = [C.POINTER(TldVaeEncConfig), C.POINTER(vp)]
        L.tld_vae_enc_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
        L.tld_vae_enc_finalize_weights.argtypes = [vp]
        L.tld_vae_enc_encode.argtypes = [vp, vp, vp, i32, i32, vp]
        L.tld_vae_enc_set_debug.argtypes = [vp, i32]
        L.tld_vae_enc_read_stage.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int64, i64p]
        L.tld_vae_enc_set_profile.argtypes = [vp, i32]
        L.tld_vae_enc_get_profile.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.tld_vae_enc_weight_bytes.argtypes = [vp]
        L.tld_vae_enc_weight_bytes.restype = C.c_int64
        L.tld_vae_enc_destroy.argtypes = [vp]
        L.tld_debug_conv3x3_s2.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.tld_clip_create.argtypes = [C.POINTER(TldClipConfig), C.POINTER(vp)]
    L.tld_clip_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
    L.tld_clip_finalize_weights.argtypes = [vp]
    L.tld_clip_encode_text.argtypes = [vp, vp, vp, vp, i32, vp]
    if hasattr(L, "tld_clip_set_debug"):             # (absent from A/B builds that predate the text tower's stage hook)
        L.tld_clip_set_debug.argtypes = [vp, i32]
        L.tld_clip_read_stage.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int64, i64p]
    L.tld_clip_weight_bytes.argtypes = [vp]
    L.tld_clip_weight_bytes.restype = C.c_int64
    L.tld_clip_destroy.argtypes = [vp]
    if hasattr(L, "tld_clip_vis_create"):            # (absent from A/B builds that predate the image tower)
        L.tld_clip_vis_create.argtypes = [C.POINTER(TldClipVisConfig), C.POINTER(vp)]
        L.tld_clip_vis_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
        L.tld_clip_vis_finalize_weights.argtypes = [vp]
        L.tld_clip_vis_encode_image.argtypes = [vp, vp, vp, i32, i32, vp]
        L.tld_clip_vis_set_debug.argtypes = [vp, i32]
        L.tld_clip_vis_read_stage.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int64, i64p]
        L.tld_clip_vis_weight_bytes.argtypes = [vp]
        L.tld_clip_vis_weight_bytes.restype = C.c_int64
        L.tld_clip_vis_destroy.argtypes = [vp]
        L.tld_debug_clip_vis_attention.argtypes = [vp, vp, i32, i32, i32, vp]
    f32 = C.c_float
    L.tld_train_create.argtypes = [C.POINTER(TldConfig), C.POINTER(vp)]
    L.tld_train_param_count.argtypes = [vp]
    L.tld_train_param_count.restype = C.c_int64
    L.tld_train_tensor_count.argtypes = [vp]
    L.tld_train_tensor_count.restype = C.c_int32
    L.tld_train_param_layout.argtypes = [vp, i32, C.c_char_p, i32, i64p, i64p]
    L.tld_train_set_angular_speeds.argtypes = [vp, C.POINTER(C.c_float), i32]
    L.tld_train_bind.argtypes = [vp, vp, vp]
    L.tld_train_refresh_weights.argtypes = [vp, vp]
    L.tld_train_forward_backward.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.tld_train_forward_backward_cb.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, GRAD_READY_FN, vp]
    L.tld_train_adam_ema.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, f32, f32, f32, f32, i32, f32, f32, vp]
    if hasattr(L, "tld_train_grad_guard"):           # (absent from A/B builds that predate the guarded optimizer step)
        L.tld_train_grad_guard.argtypes = [vp, vp, C.c_int64, f32, C.c_double, i32, f32, f32, vp, vp]
        L.tld_train_adam_ema_guarded.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, f32, f32, f32, f32, f32, f32, vp, vp]
    if hasattr(L, "tld_opt_plan_create"):            # (absent from A/B builds that predate the grouped optimizer step)
        L.tld_opt_plan_create.argtypes = [i32, i64p, C.POINTER(i32), i32, C.POINTER(TldOptGroup), i32, C.POINTER(f32), C.c_int64, C.POINTER(vp)]
        L.tld_opt_plan_destroy.argtypes = [vp]
        L.tld_opt_plan_destroy.restype = None
        L.tld_opt_plan_numel.argtypes = [vp]
        L.tld_opt_plan_numel.restype = C.c_int64
        L.tld_opt_plan_segment_sqsums.argtypes = [vp, C.POINTER(vp)]
        L.tld_train_grad_guard_grouped.argtypes = [vp, vp, C.c_int64, f32, C.c_double, i32, f32, f32, vp, vp]
        L.tld_train_adamw_ema_grouped.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, f32, f32, f32, f32, f32, f32, vp, vp]
    if hasattr(L, "tld_train_prepare_batch"):        # (absent from A/B builds that predate the device batch preparation)
        L.tld_train_prepare_batch.argtypes = [vp, C.POINTER(TldBatchSource), vp, i32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_double, f32,
                                              vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "tld_train_forward_loss"):         # (absent from A/B builds that predate the held-out loss)
        L.tld_train_prepare_batch_at.argtypes = L.tld_train_prepare_batch.argtypes + [vp]
        L.tld_train_forward_loss.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        L.tld_train_sample_loss.argtypes = [vp, vp, i32, i32, C.c_int64, vp, vp]
        L.tld_train_loss_buckets.argtypes = [vp, vp, i32, i32, vp, vp]
    L.tld_debug_attention_bwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.tld_debug_wgrad.argtypes = [vp, vp, vp, vp, C.c_int64, i32, i32, i32, vp]
    L.tld_debug_dwconv_gelu.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, i32, i32, i32, vp]
    L.tld_debug_attention_fwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.POINTER(C.c_float), vp]
    if hasattr(L, "tld_train_set_debug"):            # (absent from A/B builds that predate the stage hook)
        L.tld_train_set_debug.argtypes = [vp, i32]
        L.tld_train_read_stage.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int64, i64p]
        L.tld_train_debug_paths.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.tld_train_destroy.argtypes = [vp]
    if hasattr(L, "tld_feat_append"):                # (absent from A/B builds that predate the distribution metrics)
        L.tld_feat_append.argtypes = [vp, C.c_int64, C.c_int64, i32, i32, vp, i32, C.c_int64, i32, vp, vp]
        L.tld_feat_moments.argtypes = [vp, C.c_int64, i32, i32, vp, vp, vp]
        L.tld_feat_kernel_sum_partials.argtypes = [C.c_int64, C.c_int64, i32]
        L.tld_feat_kernel_sum_partials.restype = C.c_int64
        L.tld_feat_kernel_sum.argtypes = [vp, C.c_int64, vp, C.c_int64, i32, i32, C.c_double, i32, vp, C.c_int64, vp, vp]
    for name in ABI_SYMBOLS:
        if "TLD_LIB" in os.environ and not hasattr(L, name):     # an older A/B build: symbols added since are simply absent (tests/test_abi.py checks the real library)
            continue
        if name not in ("tld_last_error", "tld_engine_weight_bytes", "tld_vae_weight_bytes", "tld_vae_enc_weight_bytes", "tld_clip_weight_bytes", "tld_clip_vis_weight_bytes", "tld_train_param_count",
                        "tld_train_tensor_count", "tld_engine_param_count", "tld_opt_plan_numel", "tld_opt_plan_destroy", "tld_feat_kernel_sum_partials"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().tld_last_error()
        raise RuntimeError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")
