"""ctypes binding of libegoego_hip.so (C ABI: include/egoego_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libegoego_hip.so")
PERFDEBUG_LIB_PATH = os.path.join(os.path.dirname(_PKG), "tools", "_build", "libegoego_hip_perfdebug.so")  # tools/ only: `build --perfdebug`

ABI_VERSION = 8
FLAG_NO_GRAPH = 1
FLAG_FC24 = 2  # precision 9 only: fc's weights as three int8 slices (include/egoego_hip.h)
FLAG_FFN16 = 4  # precision 8 only: the FFN contractions on split-bf16 (int8 slices in the attention layer only)
PRED_NOISE, PRED_X0 = 0, 1
NOISE_INJECTED, NOISE_PHILOX, NOISE_NONE = 0, 1, 2
PREC_BF16X3, PREC_BF16X1, PREC_I8X3, PREC_I8X3_FC = 3, 1, 8, 9
K_QKV, K_ATTN, K_FC_LN, K_FFN1, K_FFN2_LN, K_EMBED, K_OUT = range(7)
KERNEL_NAMES = {"qkv": K_QKV, "attn": K_ATTN, "fc_ln": K_FC_LN, "ffn1": K_FFN1, "ffn2_ln": K_FFN2_LN,
                "embed": K_EMBED, "out": K_OUT}
DBG = {"embed": 0, "q": 1, "k": 2, "v": 3, "attn_out": 4, "attn_ln": 5, "ffn_hidden": 6, "out": 7}

c_float_p = C.POINTER(C.c_float)


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_feats", "d_model", "n_head", "n_dec_layers", "d_k", "d_v",
                                          "max_timesteps", "num_timesteps", "objective", "precision", "flags")]


class LayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_q", "b_q", "w_k", "b_k", "w_v", "b_v", "w_fc", "b_fc", "ln1_g", "ln1_b",
                                          "w_1", "b_1", "w_2", "b_2", "ln2_g", "ln2_b")]


class Weights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("start_conv_w", "start_conv_b", "position_vec", "linear_out_w",
                                          "linear_out_b", "time_mlp1_w", "time_mlp1_b", "time_mlp3_w",
                                          "time_mlp3_b")] + [("layers", C.POINTER(LayerWeights))]


class Schedule(C.Structure):
    _fields_ = [(n, c_float_p) for n in ("posterior_mean_coef1", "posterior_mean_coef2",
                                         "posterior_log_variance_clipped", "sqrt_recip_alphas_cumprod",
                                         "sqrt_recipm1_alphas_cumprod", "alphas_cumprod")]


class S1Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "d_feats", "d_model", "n_head", "n_dec_layers", "d_k", "d_v", "window")]


class S1Weights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("start_conv_w", "start_conv_b", "position_vec")] + [
        ("layers", C.POINTER(LayerWeights)), ("head_w", C.c_void_p * 8), ("head_b", C.c_void_p * 8)]


S1_HEADNET, S1_GRAVITYNET = 0, 1
FLOW_N_CONV = 20


class FlowWeights(C.Structure):
    _fields_ = [(n, C.c_void_p * FLOW_N_CONV) for n in ("conv_w", "bn_w", "bn_b", "bn_mean", "bn_var")] + [
        ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


BODY_N_JOINTS = 52
BODY_POSE_FEATS = 9 * (BODY_N_JOINTS - 1)


class BodyModelDesc(C.Structure):
    """egoego_body_model"""
    _fields_ = [(n, C.c_int32) for n in ("n_verts", "n_betas", "n_weights")] + [
        (n, C.c_void_p) for n in ("v_template", "shapedirs", "posedirs", "j_template", "j_shapedirs", "skin_weight", "skin_joint",
                                  "parents")]



class OptimState(C.Structure):
    """egoego_optim_state: the head of the fused update's state block"""
    _fields_ = [("adam_step", C.c_int64), ("applied", C.c_int64), ("skipped", C.c_int64), ("total_norm", C.c_double),
                ("total_norm_f32", C.c_float), ("last_skip", C.c_int32), ("step_size", C.c_float), ("bc2_sqrt", C.c_float),
                ("one_minus_decay", C.c_float), ("ema_action", C.c_int32), ("clip_coef", C.c_float)]


class OptimHyper(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")]


class OptimHyperW(C.Structure):
    """egoego_optim_hyper_w: decoupled weight decay and gradient clipping beside the five of OptimHyper"""
    _fields_ = OptimHyper._fields_ + [("decoupled", C.c_int), ("max_norm", C.c_double), ("clip_eps", C.c_double)]


class OptimEma(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("beta", "inv_gamma", "power", "min_value")] + [
        ("update_every", C.c_int64), ("update_after_step", C.c_int64), ("d_step", C.c_void_p), ("d_initted", C.c_void_p)]


EXPORTS = ["egoego_abi_version", "egoego_last_error", "egoego_ctx_create", "egoego_ctx_destroy",
           "egoego_load_weights", "egoego_load_schedule", "egoego_workspace_bytes", "egoego_denoise",
           "egoego_p_sample", "egoego_sample_loop", "egoego_denoise_ragged", "egoego_p_sample_ragged", "egoego_sample_loop_ragged",
           "egoego_ddim_loop", "egoego_ddim_loop_ragged", "egoego_rot6d_to_matrix", "egoego_convert_model_res", "egoego_window_prefix", "egoego_window_condition",
           "egoego_profile_begin", "egoego_profile_end", "egoego_debug_stage", "egoego_last_kernel_name", "egoego_outlier_stats",
           "egoego_s1_last_error", "egoego_s1_ctx_create", "egoego_s1_ctx_destroy", "egoego_s1_load_weights",
           "egoego_s1_workspace_bytes", "egoego_s1_encode", "egoego_s1_gravity_features", "egoego_s1_integrate",
           "egoego_s1_gravity_apply", "egoego_s1_gravity_align", "egoego_s1_head_pose_metrics", "egoego_flow_last_error", "egoego_flow_ctx_create", "egoego_flow_ctx_destroy",
           "egoego_flow_load_weights", "egoego_flow_workspace_bytes", "egoego_flow_features",
           "egoego_body_last_error", "egoego_body_ctx_create", "egoego_body_ctx_destroy", "egoego_body_load_model",
           "egoego_body_workspace_bytes", "egoego_body_forward",
           "egoego_eval_last_error", "egoego_eval_max_frames", "egoego_eval_fk", "egoego_eval_shift_xy",
           "egoego_eval_floor_contacts", "egoego_eval_metrics", "egoego_eval_root_to_floor", "egoego_eval_best",
           "egoego_win_last_error", "egoego_win_max_window", "egoego_win_build", "egoego_win_stats_workspace_bytes", "egoego_win_stats",
           "egoego_win_motion",
           "egoego_amass_last_error", "egoego_amass_max_frames", "egoego_amass_joints", "egoego_amass_floor_workspace_bytes",
           "egoego_amass_floor_contacts", "egoego_amass_head",
           "egoego_train_last_error", "egoego_train_ctx_create", "egoego_train_ctx_destroy", "egoego_train_workspace_bytes",
           "egoego_train_saves_bytes", "egoego_train_forward", "egoego_train_backward", "egoego_train_dropout_mask", "egoego_train_saved",
           "egoego_optim_last_error", "egoego_optim_ctx_create", "egoego_optim_ctx_destroy", "egoego_optim_workspace_bytes",
           "egoego_optim_state_bytes", "egoego_optim_set_tensors", "egoego_optim_step", "egoego_optimw_step", "egoego_optim_read_state",
           "egoego_s1_train_last_error", "egoego_s1_train_ctx_create", "egoego_s1_train_ctx_destroy", "egoego_s1_train_workspace_bytes",
           "egoego_s1_train_saves_bytes", "egoego_s1_train_forward", "egoego_s1_train_backward", "egoego_s1_train_dropout_mask",
           "egoego_s1_train_saved", "egoego_s1_headnet_loss_workspace_bytes", "egoego_s1_headnet_loss",
           "egoego_s1_data_last_error", "egoego_s1_gravity_batch", "egoego_s1_head_batch"]
S1_TRAIN_SAVED = {"ffn_hidden": 0, "attn_prob": 1, "attn_out": 2, "attn_ln": 3, "layer_out": 4, "layer_in": 5, "head_hidden": 6}
LOSS_L1, LOSS_L2 = 0, 1
TRAIN_SITE_ATTN, TRAIN_SITE_FC, TRAIN_SITE_FFN = 0, 1, 2
TRAIN_SAVED = {"ffn_hidden": 0, "attn_prob": 1, "attn_out": 2, "attn_ln": 3, "layer_out": 4, "layer_in": 5}
TRAIN_MAX_L = 197        # the longest window + 1 the training step accepts
TRAIN_GRAD_CHUNK = 512   # rows per partial of a weight / bias gradient sum (csrc/train_step.h)
OPTIM_CHUNK = 4096       # elements per chunk of the fused parameter update (csrc/optim_step.h)
OPTIM_MAX_LOSSES = 8
OPTIM_SKIP = {"nan": 0, "nonfinite": 1}
OPTIM_EMA_NONE, OPTIM_EMA_COPY, OPTIM_EMA_LERP = 0, 1, 2
EVAL_METRIC_KEYS = ("root_dist", "root_rot_dist", "root_trans_dist", "head_dist", "head_rot_dist", "head_trans_dist", "mpjpe",
                    "mpjpe_wo_hand", "accel_pred", "accel_gt", "accel_err", "pred_fs", "gt_fs")  # then single_jpe[22]
EVAL_N_METRICS = len(EVAL_METRIC_KEYS) + 22
OUTLIER_SITES = 16

_lib = None


class EgoEgoHipError(RuntimeError):
    pass


def use_perfdebug_build(tag=None):
    """tools/*_trace.py only: bind the perf-debug build (per-block timestamps, stage ablation; `tag` selects a variant
    built with `build --perfdebug --tag=X -D...`) instead of the product library.  Must be called before the first load()."""
    global LIB_PATH
    if _lib is not None:
        raise EgoEgoHipError("use_perfdebug_build() must be called before the library is loaded")
    tag = tag if tag is not None else os.environ.get("EGOEGO_PERFDEBUG_TAG", "")
    LIB_PATH = PERFDEBUG_LIB_PATH.replace(".so", f"_{tag}.so") if tag else PERFDEBUG_LIB_PATH


def load():
    """dlopen the library and declare prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EgoEgoHipError(
            f"{LIB_PATH} is missing: build it with `python -m egoego_release_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback for the sampling path.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t
    lib.egoego_abi_version.restype = i32
    lib.egoego_last_error.restype = C.c_char_p
    lib.egoego_ctx_create.argtypes = [C.POINTER(Config), i32, C.POINTER(vp)]
    lib.egoego_ctx_destroy.argtypes = [vp]
    lib.egoego_ctx_destroy.restype = None
    lib.egoego_load_weights.argtypes = [vp, C.POINTER(Weights), vp]
    lib.egoego_load_schedule.argtypes = [vp, C.POINTER(Schedule), vp]
    lib.egoego_workspace_bytes.argtypes = [vp, i32, i32]
    lib.egoego_workspace_bytes.restype = sz
    lib.egoego_denoise.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp]
    lib.egoego_p_sample.argtypes = [vp, vp, vp, vp, vp, vp, i32, u64, i64, i32, i32, i32, vp, sz, vp]
    lib.egoego_sample_loop.argtypes = [vp, vp, vp, i32, i32, vp, i32, u64, i64, vp, i32, vp, i32, i32, vp, sz, vp]
    # the ragged forms: + d_lengths (int32 [B]) / + d_lengths, d_window_ids (int64 [B]) behind d_row_mask
    lib.egoego_denoise_ragged.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp]
    lib.egoego_p_sample_ragged.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, u64, i64, i32, i32, i32, vp, sz, vp]
    lib.egoego_sample_loop_ragged.argtypes = [vp, vp, vp, i32, i32, vp, i32, u64, i64, vp, i32, vp, vp, vp, i32, i32, vp, sz, vp]
    lib.egoego_ddim_loop.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), i32, C.c_float, vp, i32, u64, i64, i32, i32, vp, sz, vp]
    # + d_prefix, prefix_len, d_row_mask, d_lengths, d_window_ids behind window_offset, as egoego_sample_loop_ragged orders them
    lib.egoego_ddim_loop_ragged.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), i32, C.c_float, vp, i32, u64, i64, vp, i32, vp, vp, vp,
                                            i32, i32, vp, sz, vp]
    lib.egoego_rot6d_to_matrix.argtypes = [vp, vp, i64, vp]
    lib.egoego_convert_model_res.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int32), i32, i32, i32, vp, vp, vp, vp]
    lib.egoego_window_condition.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.egoego_window_prefix.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int32), i32, i32, i32, i32, vp, vp]
    lib.egoego_profile_begin.argtypes = [vp, i32]
    lib.egoego_profile_end.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32)]
    lib.egoego_debug_stage.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, i32, i32, vp, sz, vp]
    lib.egoego_last_kernel_name.argtypes = [vp, i32]
    lib.egoego_last_kernel_name.restype = C.c_char_p
    lib.egoego_outlier_stats.argtypes = [vp, i32, i32, vp, sz, c_float_p, i32, i32, vp]
    lib.egoego_s1_last_error.restype = C.c_char_p
    lib.egoego_s1_ctx_create.argtypes = [C.POINTER(S1Config), i32, C.POINTER(vp)]
    lib.egoego_s1_ctx_destroy.argtypes = [vp]
    lib.egoego_s1_ctx_destroy.restype = None
    lib.egoego_s1_load_weights.argtypes = [vp, C.POINTER(S1Weights), vp]
    lib.egoego_s1_workspace_bytes.argtypes = [vp, i32]
    lib.egoego_s1_workspace_bytes.restype = sz
    lib.egoego_s1_encode.argtypes = [vp, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.egoego_s1_gravity_features.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.egoego_s1_integrate.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp, vp]
    lib.egoego_s1_gravity_apply.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.egoego_s1_gravity_align.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.egoego_s1_head_pose_metrics.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.egoego_flow_last_error.restype = C.c_char_p
    lib.egoego_flow_ctx_create.argtypes = [i32, i32, C.POINTER(vp)]
    lib.egoego_flow_ctx_destroy.argtypes = [vp]
    lib.egoego_flow_ctx_destroy.restype = None
    lib.egoego_flow_load_weights.argtypes = [vp, C.POINTER(FlowWeights), vp]
    lib.egoego_flow_workspace_bytes.argtypes = [vp, i32]
    lib.egoego_flow_workspace_bytes.restype = sz
    lib.egoego_flow_features.argtypes = [vp, vp, i32, vp, vp, vp, sz, vp]
    lib.egoego_body_last_error.restype = C.c_char_p
    lib.egoego_body_ctx_create.argtypes = [i32, i32, C.POINTER(vp)]
    lib.egoego_body_ctx_destroy.argtypes = [vp]
    lib.egoego_body_ctx_destroy.restype = None
    lib.egoego_body_load_model.argtypes = [vp, C.POINTER(BodyModelDesc), vp]
    lib.egoego_body_workspace_bytes.argtypes = [vp, i32, i32]
    lib.egoego_body_workspace_bytes.restype = sz
    lib.egoego_body_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.egoego_eval_last_error.restype = C.c_char_p
    lib.egoego_eval_max_frames.restype = i32
    lib.egoego_eval_fk.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), i32, vp, vp, vp]
    lib.egoego_eval_shift_xy.argtypes = [vp, i32, i32, i32, vp]
    lib.egoego_eval_floor_contacts.argtypes = [vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.egoego_eval_metrics.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.egoego_eval_root_to_floor.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.egoego_eval_best.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    lib.egoego_win_last_error.restype = C.c_char_p
    lib.egoego_win_max_window.restype = i32
    lib.egoego_win_build.argtypes = [vp, vp, vp, i32, vp, C.POINTER(C.c_int32), vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.egoego_win_stats_workspace_bytes.argtypes = [i32, i32]
    lib.egoego_win_stats_workspace_bytes.restype = sz
    lib.egoego_win_stats.argtypes = [vp, vp, vp, i32, i32, vp, vp, sz, vp]
    lib.egoego_win_motion.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.egoego_amass_last_error.restype = C.c_char_p
    lib.egoego_amass_max_frames.restype = i32
    lib.egoego_amass_joints.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int32), i32, vp, vp, vp]
    lib.egoego_amass_floor_workspace_bytes.argtypes = [i32, i32]
    lib.egoego_amass_floor_workspace_bytes.restype = sz
    lib.egoego_amass_floor_contacts.argtypes = [vp, C.POINTER(C.c_int32), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.egoego_amass_head.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.egoego_train_last_error.restype = C.c_char_p
    lib.egoego_train_ctx_create.argtypes = [C.POINTER(Config), i32, C.POINTER(vp)]
    lib.egoego_train_ctx_destroy.argtypes = [vp]
    lib.egoego_train_ctx_destroy.restype = None
    lib.egoego_train_workspace_bytes.argtypes = [vp, i32, i32]
    lib.egoego_train_workspace_bytes.restype = sz
    lib.egoego_train_saves_bytes.argtypes = [vp, i32, i32]
    lib.egoego_train_saves_bytes.restype = sz
    # ctx, weights, x_start, noise, cond_noise, cond_mask, t, row_mask, 3 schedule tables, objective, loss type, p_drop, seed, window ids,
    # B, T, saves, bytes, workspace, bytes, loss, model_out, stream
    lib.egoego_train_forward.argtypes = [vp, C.POINTER(Weights), vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, u64, vp, i32, i32,
                                         vp, sz, vp, sz, vp, vp, vp]
    # ctx, weights, saves, bytes, upstream, grads (the layout of Weights), p_drop, seed, B, T, workspace, bytes, stream
    lib.egoego_train_backward.argtypes = [vp, C.POINTER(Weights), vp, sz, vp, C.POINTER(Weights), C.c_float, u64, i32, i32, vp, sz, vp]
    lib.egoego_train_dropout_mask.argtypes = [vp, C.c_float, u64, i32, i32, vp, i32, i32, vp, vp, sz, vp]
    lib.egoego_train_saved.argtypes = [vp, vp, sz, i32, i32, i32, i32, vp, vp]
    lib.egoego_optim_last_error.restype = C.c_char_p
    lib.egoego_optim_ctx_create.argtypes = [i32, i32, C.POINTER(i64), C.POINTER(vp)]
    lib.egoego_optim_ctx_destroy.argtypes = [vp]
    lib.egoego_optim_ctx_destroy.restype = None
    lib.egoego_optim_workspace_bytes.argtypes = [vp]
    lib.egoego_optim_workspace_bytes.restype = sz
    lib.egoego_optim_state_bytes.argtypes = [vp]
    lib.egoego_optim_state_bytes.restype = sz
    # ctx, p, g, m, v, ema (host arrays of device pointers; g, m, v / ema may be NULL), state, bytes, stream
    lib.egoego_optim_set_tensors.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, sz, vp]
    # ctx, hyper, ema, losses (host array of device pointers), n_losses, inv_scale, found_inf, skip_on, zero_grads, do_adam, do_ema,
    # state, bytes, workspace, bytes, stream
    lib.egoego_optim_step.argtypes = [vp, C.POINTER(OptimHyper), C.POINTER(OptimEma), C.POINTER(vp), i32, vp, vp, i32, i32, i32, i32,
                                      vp, sz, vp, sz, vp]
    lib.egoego_optimw_step.argtypes = [vp, C.POINTER(OptimHyperW)] + lib.egoego_optim_step.argtypes[2:]
    lib.egoego_optim_read_state.argtypes = [vp, vp, sz, vp, vp]
    lib.egoego_s1_train_last_error.restype = C.c_char_p
    lib.egoego_s1_train_ctx_create.argtypes = [C.POINTER(S1Config), i32, C.POINTER(vp)]
    lib.egoego_s1_train_ctx_destroy.argtypes = [vp]
    lib.egoego_s1_train_ctx_destroy.restype = None
    lib.egoego_s1_train_workspace_bytes.argtypes = [vp, i32]
    lib.egoego_s1_train_workspace_bytes.restype = sz
    lib.egoego_s1_train_saves_bytes.argtypes = [vp, i32]
    lib.egoego_s1_train_saves_bytes.restype = sz
    # ctx, weights, feats, valid, p_drop, seed, window ids, W, saves, bytes, workspace, bytes, heads, stream
    lib.egoego_s1_train_forward.argtypes = [vp, C.POINTER(S1Weights), vp, vp, C.c_float, u64, vp, i32, vp, sz, vp, sz, vp, vp]
    # ctx, weights, saves, bytes, d_heads, grads (the layout of S1Weights), p_drop, seed, W, workspace, bytes, stream
    lib.egoego_s1_train_backward.argtypes = [vp, C.POINTER(S1Weights), vp, sz, vp, C.POINTER(S1Weights), C.c_float, u64, i32, vp, sz, vp]
    lib.egoego_s1_train_dropout_mask.argtypes = [vp, C.c_float, u64, i32, i32, vp, i32, vp, vp, sz, vp]
    lib.egoego_s1_train_saved.argtypes = [vp, vp, sz, i32, i32, i32, vp, vp]
    lib.egoego_s1_headnet_loss_workspace_bytes.argtypes = [i32]
    lib.egoego_s1_headnet_loss_workspace_bytes.restype = sz
    # heads, window, B, T, head_pose, head_vels, dist_scale, w_rotation, w_va, w_dist, loss, d_heads fp64, d_heads fp32, workspace, bytes, stream
    lib.egoego_s1_headnet_loss.argtypes = [vp, i32, i32, i32, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, sz, vp]
    lib.egoego_s1_data_last_error.restype = C.c_char_p
    # pose, rows, offsets, sequences, seq ids, draw ids, B, window, seed, for_eval, planted start / rot / scale, ori_head_pose,
    # head_rot_mat, head_trans, seq_len, aligned_rot_mat, aligned_scale, floor_normal, start_t_idx, aug_scale, stream
    lib.egoego_s1_gravity_batch.argtypes = [vp, i32, vp, i32, vp, vp, i32, i32, u64, i32, vp, vp, vp] + [vp] * 9 + [vp]
    # pose, vels, feats, rows, D, offsets, sequences, slam32, slam_trans64, slam offsets, slam rows, seq ids, draw ids, B, window, seed,
    # for_eval, planted start, head_pose, head_vels, of, seq_len, start_t_idx, the six SLAM arrays, pose_len, stream
    lib.egoego_s1_head_batch.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, u64, i32, vp] + [vp] * 12 + [vp]
    if lib.egoego_abi_version() != ABI_VERSION:
        raise EgoEgoHipError(f"ABI mismatch: library {lib.egoego_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def _checker(module, last_error):
    """-> check(rc): raises EgoEgoHipError with the module's own last error on a non-zero return code; check.last_error() reads
    that text."""
    def read():
        return getattr(load(), last_error)().decode()

    def check(rc):
        if rc != 0:
            raise EgoEgoHipError(f"libegoego_hip {module}error {rc}: {read()}")

    check.last_error = read
    return check


check = _checker("", "egoego_last_error")
check_s1 = _checker("stage-1 ", "egoego_s1_last_error")
check_flow = _checker("flow-CNN ", "egoego_flow_last_error")
check_body = _checker("body-model ", "egoego_body_last_error")
check_eval = _checker("evaluation ", "egoego_eval_last_error")
check_win = _checker("motion-window ", "egoego_win_last_error")
check_amass = _checker("AMASS-preprocessing ", "egoego_amass_last_error")
check_train = _checker("training-step ", "egoego_train_last_error")
check_optim = _checker("parameter-update ", "egoego_optim_last_error")
check_s1_train = _checker("stage-1 training ", "egoego_s1_train_last_error")
check_s1_data = _checker("stage-1 data ", "egoego_s1_data_last_error")
