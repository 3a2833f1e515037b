"""ctypes binding of ``libgbnf_hip.so`` (C ABI: ``include/gbnf.h``).

There is NO fallback: if the shared library is missing, or a call fails, this
module raises.  Device buffers are PyTorch-ROCm tensors; only their
``data_ptr()`` and the current HIP stream cross the boundary.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GBNF_LIB_PATH: diagnostic builds only (e.g. the -DGBNF_STAMPS library of tools/build_stamps.sh)
LIB_PATH = os.environ.get("GBNF_LIB_PATH") or os.path.join(_HERE, "libgbnf_hip.so")

KIND = {"glow": 0, "realnvp": 1}
ACT = {"tanh": 0, "relu": 1, "residual": 2}     # GBNF_ACT_TANH / _RELU / _RESIDUAL_RELU
COUPLING = {"affine": 0, "additive": 1}
MATH = {"default": -1, "f32": 0, "f16x3": 1, "bf16x6": 2}
MATH_NAME = {v: k for k, v in MATH.items()}

# every symbol include/gbnf.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = (
    "gbnf_version", "gbnf_last_error", "gbnf_saturation_count", "gbnf_training_saturation_count",
    "gbnf_flow_create", "gbnf_flow_create_mode", "gbnf_flow_create_ex", "gbnf_flow_destroy", "gbnf_flow_info", "gbnf_flow_forward",
    "gbnf_flow_inverse",
    "gbnf_mixture_create", "gbnf_mixture_destroy", "gbnf_mixture_set_base",
    "gbnf_mixture_component_log_prob", "gbnf_mixture_component_log_prob_strided",
    "gbnf_mixture_component_log_prob_multi", "gbnf_mixture_component_forward", "gbnf_mixture_lse",
    "gbnf_mixture_log_prob",
    "gbnf_actnorm_init", "gbnf_boosting_weights",
    "gbnf_flow_validate", "gbnf_trainer_create", "gbnf_trainer_destroy", "gbnf_trainer_forward",
    "gbnf_trainer_grad_floats", "gbnf_trainer_workspace_bytes", "gbnf_trainer_backward", "gbnf_trainer_trace_floats",
    "gbnf_trainer_bind_batch_stats", "gbnf_trainer_set_batch_stats", "gbnf_trainer_create_mode", "gbnf_trainer_repair_count",
    "gbnf_trainer_apply_update", "gbnf_trainer_step_workspace_bytes", "gbnf_trainer_nll_step",
    "gbnf_trainer_set_deterministic", "gbnf_trainer_get_deterministic",
    "gbnf_image_flow_create", "gbnf_image_flow_destroy", "gbnf_image_flow_info", "gbnf_image_flow_workspace_bytes",
    "gbnf_image_flow_forward", "gbnf_image_flow_prior", "gbnf_image_flow_eps_floats", "gbnf_image_flow_inverse",
    "gbnf_image_flow_numerics", "gbnf_image_flow_repair_counts", "gbnf_image_flow_create_mode", "gbnf_image_flow_actnorm_stats",
    "gbnf_comm_unique_id", "gbnf_comm_create", "gbnf_comm_destroy", "gbnf_comm_info", "gbnf_mixture_group_log_prob",
    "gbnf_group_graph_create", "gbnf_group_graph_launch", "gbnf_group_graph_destroy",
    "gbnf_flow_numerics", "gbnf_mixture_numerics", "gbnf_tuning_set", "gbnf_tuning_get",
    "gbnf_resample_workspace_bytes", "gbnf_resample_rows", "gbnf_boosted_step_workspace_bytes", "gbnf_boosted_nll_step",
    "gbnf_mixture_rho_step",
    "gbnf_flow_numerics_inverse", "gbnf_image_flow_inverse_check_counts",
    "gbnf_image_trainer_create", "gbnf_image_trainer_destroy", "gbnf_image_trainer_trace_floats", "gbnf_image_trainer_workspace_bytes",
    "gbnf_image_trainer_forward", "gbnf_image_trainer_grad_floats", "gbnf_image_trainer_backward",
    "gbnf_image_trainer_set_deterministic", "gbnf_image_trainer_get_deterministic",
    "gbnf_image_trainer_actnorm_count", "gbnf_image_trainer_actnorm_init_workspace_bytes", "gbnf_image_trainer_actnorm_init",
    "gbnf_image_trainer_bind_lu", "gbnf_image_trainer_bind_top", "gbnf_image_trainer_step_grad_floats",
    "gbnf_image_trainer_step_workspace_bytes", "gbnf_image_trainer_apply_update", "gbnf_image_trainer_nll_step",
    "gbnf_image_rho_step_workspace_bytes", "gbnf_image_mixture_rho_step",
    "gbnf_image_boosted_step_workspace_bytes", "gbnf_image_boosted_nll_step",
    "gbnf_mixture_sample_workspace_bytes", "gbnf_mixture_sample_begin", "gbnf_mixture_sample_finish",
    "gbnf_image_flow_set_ycond", "gbnf_image_flow_y_classes", "gbnf_image_flow_forward_y", "gbnf_image_flow_prior_y",
    "gbnf_image_trainer_bind_ycond", "gbnf_image_trainer_y_classes", "gbnf_image_trainer_nll_step_y",
    "gbnf_image_boosted_step_workspace_bytes_y", "gbnf_image_boosted_nll_step_y",
    "gbnf_image_flow_set_deterministic", "gbnf_image_flow_get_deterministic",
    "gbnf_image_flow_forward_classes", "gbnf_class_posterior", "gbnf_image_mixture_rho_step_y",
    "gbnf_image_trainer_backward_x", "gbnf_image_score_seed", "gbnf_mixture_responsibilities",
    "gbnf_image_mixture_score_workspace_bytes", "gbnf_image_mixture_score",
    "gbnf_trainer_backward_x_workspace_bytes", "gbnf_trainer_backward_x", "gbnf_score_seed",
    "gbnf_mixture_score_workspace_bytes", "gbnf_mixture_score",
    "gbnf_image_flow_encode",
    "gbnf_eval_workspace_bytes", "gbnf_eval_accumulate", "gbnf_eval_accumulate_class_loss", "gbnf_mixture_evaluate",
    "gbnf_image_mixture_evaluate_workspace_bytes", "gbnf_image_mixture_evaluate", "gbnf_image_mixture_evaluate_y",
    "gbnf_weights_em_workspace_bytes", "gbnf_weights_em", "gbnf_weights_to_rho",
    "gbnf_mixture_step_workspace_bytes", "gbnf_mixture_nll_step",
)
# all mixture weights at once (include/gbnf.h: EM over a cached table of component log-likelihoods)
WEIGHTS_SYMBOLS = ("gbnf_weights_em_workspace_bytes", "gbnf_weights_em", "gbnf_weights_to_rho")
WEIGHTS_MAX_COMPONENTS = 64
WEIGHTS_STATE_DOUBLES = 8 + WEIGHTS_MAX_COMPONENTS
# state[7] reads bad_start + 2 * (entries weights_to_rho clamped); the weights start at WEIGHTS_STATE["weights"]
WEIGHTS_STATE = {"iters": 0, "converged": 1, "rows": 2, "excluded": 3, "L0": 4, "L": 5, "delta": 6, "flags": 7, "weights": 8}

# the evaluation state of the validation pass (include/gbnf.h: GBNF_EVAL_STATE_DOUBLES and its layout)
EVAL_STATE_DOUBLES = 16
EVAL_STATE = {"rows": 0, "batches": 1, "sum_G": 2, "sum_g": 3, "sum_G_minus_g": 4, "sum_E": 5, "batch_mean_G": 6, "batch_mean_g": 7,
              "batch_mean_E": 8, "non_finite_rows": 9, "sum_ce": 10, "batch_mean_ce": 11, "sum_correct": 12}
# the grid of the accumulate kernels: min(ceil(n / EVAL_ROWS_PER_WORKGROUP), EVAL_MAX_PARTIALS) workgroups, a grid-stride loop beyond
EVAL_ROWS_PER_WORKGROUP = 1024
EVAL_MAX_PARTIALS = 256


class GbnfError(RuntimeError):
    pass


class _Linear(C.Structure):
    _fields_ = [("weight", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)),
                ("out_features", C.c_int32), ("in_features", C.c_int32)]


class _Net(C.Structure):
    _fields_ = [("activation", C.c_int32), ("n_layers", C.c_int32), ("layers", C.POINTER(_Linear))]


class _GlowStep(C.Structure):
    _fields_ = [("actnorm_bias", C.POINTER(C.c_float)), ("actnorm_logs", C.POINTER(C.c_float)),
                ("perm_indices", C.POINTER(C.c_int64)), ("block", _Net)]


class _RealNVPStep(C.Structure):
    _fields_ = [("flipped", C.c_int32), ("has_batch_norm", C.c_int32),
                ("bn_log_gamma", C.POINTER(C.c_float)), ("bn_beta", C.POINTER(C.c_float)),
                ("bn_running_mean", C.POINTER(C.c_float)), ("bn_running_var", C.POINTER(C.c_float)),
                ("bn_eps", C.c_float), ("t_net", _Net), ("s_net", _Net)]


class _FlowDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("d", C.c_int32), ("n_steps", C.c_int32), ("coupling", C.c_int32),
                ("glow_steps", C.POINTER(_GlowStep)), ("realnvp_steps", C.POINTER(_RealNVPStep))]


class _Conv(C.Structure):
    _fields_ = [("weight", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)),
                ("actnorm_bias", C.POINTER(C.c_float)), ("actnorm_logs", C.POINTER(C.c_float)),
                ("logs", C.POINTER(C.c_float)),
                ("out_channels", C.c_int32), ("in_channels", C.c_int32), ("kernel_size", C.c_int32)]


class _ImageStep(C.Structure):
    _fields_ = [("actnorm_bias", C.POINTER(C.c_float)), ("actnorm_logs", C.POINTER(C.c_float)),
                ("perm_weight", C.POINTER(C.c_float)), ("perm_indices", C.POINTER(C.c_int64)),
                ("n_convs", C.c_int32), ("convs", C.POINTER(_Conv))]


class _ImageLevel(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("steps", C.POINTER(_ImageStep)), ("split_prior", C.POINTER(_Conv))]


class _ImageFlowDesc(C.Structure):
    _fields_ = [("channels", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("n_levels", C.c_int32),
                ("coupling", C.c_int32), ("hidden", C.c_int32), ("bounds", C.c_float),
                ("levels", C.POINTER(_ImageLevel)), ("learn_top", C.POINTER(_Conv))]


class KernelInfo(C.Structure):
    _fields_ = [("hidden_tiles", C.c_int32), ("out_tiles", C.c_int32), ("samples_per_wave", C.c_int32),
                ("n_steps", C.c_int32), ("macs_per_sample", C.c_double),
                ("padded_macs_per_sample", C.c_double), ("packed_bytes", C.c_int64),
                ("math_mode", C.c_int32), ("probe_rel_err", C.c_float)]


class NumericsStatus(C.Structure):
    """gbnf_numerics_status: the library's own re-check of a DEFAULT handle's f16x3 choice on the caller's data."""
    _fields_ = [("math_mode", C.c_int32), ("demoted", C.c_int32), ("checks", C.c_int64),
                ("worst_rel_err", C.c_float), ("tolerance", C.c_float)]


OPT_KIND = {"sgd": 0, "adamw": 1}      # GBNF_OPT_SGD / _ADAMW


class _OptHyper(C.Structure):
    """gbnf_opt_hyper (48 bytes)."""
    _fields_ = [("kind", C.c_int32), ("reserved0", C.c_int32), ("step", C.c_int64),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("bn_momentum", C.c_float),
                ("reserved1", C.c_float)]


_lib = None


def tuning_set(key, value):
    """Launch-policy knob of the library (include/gbnf.h, gbnf_tuning_set): tests, soak runs, tuning."""
    _check(lib().gbnf_tuning_set(key.encode(), int(value)))


def tuning_get(key):
    v = C.c_int32()
    _check(lib().gbnf_tuning_get(key.encode(), C.byref(v)))
    return v.value


def lib():
    """Load the library (once).  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GbnfError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
            "(or gradient-boosted-normalizing-flows_amd/csrc/build.py). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.gbnf_version.restype = C.c_int
    L.gbnf_last_error.restype = C.c_char_p
    L.gbnf_flow_create.argtypes = [C.POINTER(_FlowDesc), C.POINTER(vp)]
    L.gbnf_saturation_count.argtypes = [C.POINTER(C.c_int64), i32]
    L.gbnf_training_saturation_count.argtypes = [C.POINTER(C.c_int64), i32]
    L.gbnf_flow_create_mode.argtypes = [C.POINTER(_FlowDesc), i32, C.POINTER(vp)]
    L.gbnf_flow_create_ex.argtypes = [C.POINTER(_FlowDesc), i32, i32, C.POINTER(vp)]
    L.gbnf_flow_destroy.argtypes = [vp]
    L.gbnf_flow_info.argtypes = [vp, C.POINTER(KernelInfo)]
    L.gbnf_flow_forward.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.gbnf_flow_inverse.argtypes = [vp, vp, i64, vp, vp, vp]
    L.gbnf_mixture_create.argtypes = [C.POINTER(vp), i32, C.POINTER(vp)]
    L.gbnf_mixture_destroy.argtypes = [vp]
    L.gbnf_mixture_set_base.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.gbnf_mixture_component_log_prob.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.gbnf_mixture_component_log_prob_strided.argtypes = [vp, vp, i64, i32, i32, vp, i64, vp]
    L.gbnf_mixture_component_log_prob_multi.argtypes = [vp, C.POINTER(vp), i32, i64, i32, i32, vp, i64, vp]
    L.gbnf_mixture_component_forward.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp]
    L.gbnf_mixture_lse.argtypes = [vp, i64, vp, i32, i64, vp, vp]
    L.gbnf_mixture_log_prob.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    L.gbnf_actnorm_init.argtypes = [vp, i64, i32, C.c_float, vp, vp, vp]
    L.gbnf_boosting_weights.argtypes = [vp, i64, C.c_float, vp, vp]
    L.gbnf_resample_workspace_bytes.argtypes = [i64, C.POINTER(i64)]
    L.gbnf_resample_rows.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp]
    L.gbnf_boosted_step_workspace_bytes.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
    L.gbnf_boosted_nll_step.argtypes = [vp, i32, vp, C.c_float, vp, vp, i64, vp, vp, vp, vp, C.POINTER(_OptHyper), vp, vp, vp, i64, vp]
    L.gbnf_mixture_rho_step.argtypes = [vp, vp, i64, i32, vp, C.c_float, vp, vp, vp]
    L.gbnf_flow_validate.argtypes = [C.POINTER(_FlowDesc)]
    L.gbnf_flow_numerics.argtypes = [vp, C.POINTER(NumericsStatus)]
    L.gbnf_mixture_numerics.argtypes = [vp, C.POINTER(NumericsStatus)]
    L.gbnf_flow_numerics_inverse.argtypes = [vp, C.POINTER(NumericsStatus)]
    L.gbnf_tuning_set.argtypes = [C.c_char_p, i32]
    L.gbnf_tuning_get.argtypes = [C.c_char_p, C.POINTER(i32)]
    L.gbnf_trainer_create.argtypes = [C.POINTER(_FlowDesc), C.POINTER(vp)]
    L.gbnf_trainer_create_mode.argtypes = [C.POINTER(_FlowDesc), C.c_int32, C.POINTER(vp)]
    L.gbnf_trainer_repair_count.argtypes = [vp, C.POINTER(i64), C.c_int32]
    L.gbnf_trainer_destroy.argtypes = [vp]
    L.gbnf_trainer_forward.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.gbnf_trainer_trace_floats.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_trainer_bind_batch_stats.argtypes = [vp, i32, vp, vp]
    L.gbnf_trainer_set_batch_stats.argtypes = [vp, i32]
    L.gbnf_trainer_set_deterministic.argtypes = [vp, i32]
    L.gbnf_trainer_get_deterministic.argtypes = [vp, C.POINTER(i32)]
    L.gbnf_trainer_grad_floats.argtypes = [vp, C.POINTER(i64)]
    L.gbnf_trainer_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_trainer_backward.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_trainer_apply_update.argtypes = [vp, vp, vp, vp, C.POINTER(_OptHyper), vp, vp]
    L.gbnf_trainer_step_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_trainer_nll_step.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, C.POINTER(_OptHyper), vp, vp, i64, vp]
    L.gbnf_image_flow_create.argtypes = [C.POINTER(_ImageFlowDesc), C.POINTER(vp)]
    L.gbnf_image_flow_create_mode.argtypes = [C.POINTER(_ImageFlowDesc), i32, C.POINTER(vp)]
    L.gbnf_image_flow_actnorm_stats.argtypes = [vp, vp, vp, i64, i32, vp, vp, C.POINTER(i32), vp, i64, vp]
    L.gbnf_image_flow_destroy.argtypes = [vp]
    L.gbnf_image_flow_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]
    L.gbnf_image_flow_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_image_flow_forward.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_flow_prior.argtypes = [vp, C.POINTER(C.c_float)]
    L.gbnf_image_flow_numerics.argtypes = [vp, C.POINTER(NumericsStatus)]
    L.gbnf_image_flow_repair_counts.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_float)]
    L.gbnf_image_flow_inverse_check_counts.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_float)]
    L.gbnf_comm_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.gbnf_comm_create.argtypes = [C.POINTER(C.c_uint8), i32, i32, C.POINTER(vp)]
    L.gbnf_comm_destroy.argtypes = [vp]
    L.gbnf_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.gbnf_mixture_group_log_prob.argtypes = [vp, vp, C.POINTER(vp), i32, i64, i32, vp, vp, vp, vp, vp]
    L.gbnf_group_graph_create.argtypes = [vp, vp, C.POINTER(vp), i32, i64, i32, vp, vp, vp, vp, C.POINTER(vp)]
    L.gbnf_group_graph_launch.argtypes = [vp, vp]
    L.gbnf_group_graph_destroy.argtypes = [vp]
    L.gbnf_image_flow_eps_floats.argtypes = [vp, C.POINTER(i64)]
    L.gbnf_image_flow_set_deterministic.argtypes = [vp, i32]
    L.gbnf_image_flow_get_deterministic.argtypes = [vp, C.POINTER(i32)]
    L.gbnf_image_trainer_create.argtypes = [C.POINTER(_ImageFlowDesc), C.POINTER(vp)]
    L.gbnf_image_trainer_destroy.argtypes = [vp]
    L.gbnf_image_trainer_trace_floats.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_image_trainer_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_image_trainer_forward.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_trainer_grad_floats.argtypes = [vp, C.POINTER(i64)]
    L.gbnf_image_trainer_backward.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_trainer_set_deterministic.argtypes = [vp, i32]
    L.gbnf_image_trainer_get_deterministic.argtypes = [vp, C.POINTER(i32)]
    L.gbnf_image_trainer_actnorm_count.argtypes = [vp, C.POINTER(i32)]
    L.gbnf_image_trainer_actnorm_init_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_image_trainer_actnorm_init.argtypes = [vp, vp, vp, i64, C.c_float, vp, vp, i64, vp]
    L.gbnf_image_trainer_bind_lu.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.gbnf_image_trainer_bind_top.argtypes = [vp, vp, vp, vp]
    L.gbnf_image_trainer_step_grad_floats.argtypes = [vp, C.POINTER(i64)]
    L.gbnf_image_trainer_step_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_image_trainer_apply_update.argtypes = [vp, vp, vp, vp, C.POINTER(_OptHyper), vp, vp]
    L.gbnf_image_trainer_nll_step.argtypes = [vp, vp, vp, i64, C.c_float, vp, vp, vp, C.POINTER(_OptHyper), vp, vp, i64, vp]
    L.gbnf_image_flow_inverse.argtypes = [vp, vp, vp, C.c_float, i64, vp, vp, i64, vp]
    L.gbnf_image_flow_encode.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_rho_step_workspace_bytes.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(i64)]
    L.gbnf_image_mixture_rho_step.argtypes = [C.POINTER(vp), i32, vp, vp, i64, vp, C.c_float, vp, vp, vp, i64, vp]
    L.gbnf_image_boosted_step_workspace_bytes.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.gbnf_image_boosted_nll_step.argtypes = [vp, C.c_float, vp, vp, vp, i64, C.c_float, vp, vp, vp, C.POINTER(_OptHyper), vp, vp, i64, vp]
    L.gbnf_mixture_sample_workspace_bytes.argtypes = [i32, i64, i32, C.POINTER(i64)]
    L.gbnf_mixture_sample_begin.argtypes = [vp, i32, vp, vp, i64, i32, vp, vp, vp, vp, i64, vp]
    L.gbnf_mixture_sample_finish.argtypes = [C.POINTER(vp), i32, C.POINTER(i64), vp, i64, vp, vp, vp, i64, vp]
    L.gbnf_image_flow_set_ycond.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.gbnf_image_flow_y_classes.argtypes = [vp, C.POINTER(i32)]
    L.gbnf_image_flow_forward_y.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_flow_prior_y.argtypes = [vp, vp, i64, vp, C.c_float, vp, vp, vp]
    L.gbnf_image_trainer_bind_ycond.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.gbnf_image_trainer_y_classes.argtypes = [vp, C.POINTER(i32)]
    L.gbnf_image_trainer_nll_step_y.argtypes = [vp, vp, vp, vp, i64, C.c_float, C.c_float, vp, vp, vp, C.POINTER(_OptHyper), vp, vp, i64, vp]
    L.gbnf_image_boosted_step_workspace_bytes_y.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.gbnf_image_boosted_nll_step_y.argtypes = [vp, C.c_float, vp, vp, vp, vp, i64, C.c_float, C.c_float, vp, vp, vp, C.POINTER(_OptHyper),
                                                vp, vp, i64, vp]
    L.gbnf_image_flow_forward_classes.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_class_posterior.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    L.gbnf_image_mixture_rho_step_y.argtypes = [C.POINTER(vp), i32, vp, vp, vp, i64, vp, C.c_float, vp, vp, vp, i64, vp]
    L.gbnf_image_trainer_backward_x.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, i64, vp]
    L.gbnf_image_score_seed.argtypes = [vp, vp, i64, vp, i64, i32, i32, vp, vp, vp]
    L.gbnf_mixture_responsibilities.argtypes = [vp, vp, i32, i64, vp, vp, vp]
    L.gbnf_image_mixture_score_workspace_bytes.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(i64)]
    L.gbnf_image_mixture_score.argtypes = [C.POINTER(vp), i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.gbnf_trainer_backward_x_workspace_bytes.argtypes = [vp, i64, C.POINTER(i64)]
    L.gbnf_trainer_backward_x.argtypes = [vp, vp, i64, vp, vp, vp, vp, i32, vp, i64, vp]
    L.gbnf_score_seed.argtypes = [vp, vp, vp, vp, i64, i32, vp, vp, vp, vp]
    L.gbnf_mixture_score_workspace_bytes.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(i64)]
    L.gbnf_mixture_score.argtypes = [C.POINTER(vp), i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.gbnf_eval_workspace_bytes.argtypes = [i64, C.POINTER(i64)]
    L.gbnf_eval_accumulate.argtypes = [vp, i64, i32, i64, vp, i32, vp, vp, vp, i64, vp]
    L.gbnf_eval_accumulate_class_loss.argtypes = [vp, vp, i64, i32, vp, i32, i32, vp, vp, i64, vp]
    L.gbnf_mixture_evaluate.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_mixture_evaluate_workspace_bytes.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(i64)]
    L.gbnf_image_mixture_evaluate.argtypes = [C.POINTER(vp), i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_image_mixture_evaluate_y.argtypes = [C.POINTER(vp), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbnf_weights_em_workspace_bytes.argtypes = [i32, i64, C.POINTER(i64)]
    L.gbnf_weights_em.argtypes = [vp, i64, i32, i64, vp, i32, C.c_double, vp, vp, i64, vp]
    L.gbnf_weights_to_rho.argtypes = [vp, i32, C.c_float, C.c_float, vp, vp]
    L.gbnf_mixture_step_workspace_bytes.argtypes = [C.POINTER(vp), i32, i64, C.POINTER(i64)]
    L.gbnf_mixture_nll_step.argtypes = [C.POINTER(vp), i32, vp, vp, i64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(_OptHyper),
                                        vp, vp, vp, vp, i64, vp]
    for name in ABI_SYMBOLS:
        if name not in ("gbnf_version", "gbnf_last_error"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise GbnfError(f"libgbnf_hip error {rc}: {lib().gbnf_last_error().decode(errors='replace')}")


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class _Keep:
    """Keeps the numpy arrays / ctypes arrays referenced by a descriptor alive."""

    def __init__(self):
        self.refs = []

    def f32(self, a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        self.refs.append(a)
        return _fptr(a)

    def i64(self, a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
        self.refs.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_int64))

    def net(self, net):
        arr = (_Linear * len(net["layers"]))()
        for k, (w, b) in enumerate(net["layers"]):
            w = np.asarray(w)
            arr[k] = _Linear(self.f32(w), self.f32(b), int(w.shape[0]), int(w.shape[1]))
        self.refs.append(arr)
        return _Net(ACT[net["act"]], len(net["layers"]), arr)


def flow_desc_from_spec(spec):
    """flow spec (see spec.py) -> (ctypes gbnf_flow_desc, keep-alive object)."""
    keep = _Keep()
    K = len(spec["steps"])
    desc = _FlowDesc()
    desc.kind = KIND[spec["kind"]]
    desc.d = int(spec["d"])
    desc.n_steps = K
    desc.coupling = COUPLING[spec.get("coupling") or "affine"]
    if spec["kind"] == "glow":
        steps = (_GlowStep * K)()
        for k, st in enumerate(spec["steps"]):
            steps[k] = _GlowStep(keep.f32(st["an_bias"]), keep.f32(st["an_logs"]), keep.i64(st["perm"]),
                                 keep.net(st["net"]))
        desc.glow_steps = steps
    else:
        steps = (_RealNVPStep * K)()
        for k, st in enumerate(spec["steps"]):
            s = _RealNVPStep()
            s.flipped = int(bool(st["flipped"]))
            bn = st["bn"]
            s.has_batch_norm = int(bn is not None)
            if bn is not None:
                s.bn_log_gamma = keep.f32(bn["log_gamma"])
                s.bn_beta = keep.f32(bn["beta"])
                s.bn_running_mean = keep.f32(bn["running_mean"])
                s.bn_running_var = keep.f32(bn["running_var"])
                s.bn_eps = float(bn["eps"])
            s.t_net = keep.net(st["t_net"])
            s.s_net = keep.net(st["s_net"])
            steps[k] = s
        desc.realnvp_steps = steps
    keep.refs.append(steps)
    return desc, keep


def _require_device_f32(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GbnfError(f"{name} must be a tensor on the MI355X (cuda) device; there is no CPU path")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise GbnfError(f"{name} must be contiguous float32")
    return t


def _stream_ptr():
    """The current HIP stream of the current device as a void*.  torch.cuda.current_stream() builds a Stream object through
    three Python layers (15 us per call, a fifth of a module call's host time); the raw-handle accessor is one C call."""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return C.c_void_p(raw(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the calling idiom: every entry point below hands tensors, handle lists, size queries and workspaces over with these
def _ptr(t):
    """A tensor's address as a void* (None: null; an empty tensor's address is null already)."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _handle_array(objs):
    """The ``handle``s of a list of library objects as a void*[]."""
    return (C.c_void_p * len(objs))(*[o.handle for o in objs])


def _addr_array(tensors):
    """The addresses of a list of tensors (None: null) as a void*[]."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _query_i64(fn, *args):
    """``fn(*args, &out)`` of a library call that reports one int64 (a size, a count): asked anew on every call."""
    out = C.c_int64()
    _check(fn(*args, C.byref(out)))
    return int(out.value)


def _workspace_arg(workspace, nbytes, device):
    """The ``workspace`` argument of a call: None -> a new float32 buffer of ``nbytes()`` bytes (the size query runs only then);
    anything else must be a contiguous device tensor (its size is checked by the library)."""
    if workspace is None:
        import torch
        return torch.empty((nbytes() + 3) // 4, dtype=torch.float32, device=device)
    return _check_workspace(workspace)


def _check_workspace(workspace):
    """A caller's workspace must be a contiguous device tensor (its size is checked by the library)."""
    import torch
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous():
        raise GbnfError("workspace must be a contiguous device tensor")
    return workspace


def _grown(buf, nbytes, device, dtype=None):
    """A cached workspace for a call that needs ``nbytes``: ``buf`` itself while it is large enough and on ``device``, else a new one
    (float32 unless ``dtype`` says otherwise).  The caller asks the library for ``nbytes`` on every call and keeps what it gets back.
    (The three tabular training steps make the same test in line: their host time is counted in microseconds.)"""
    if buf is None or buf.numel() * buf.element_size() < nbytes or buf.device != device:
        import torch
        dtype = torch.float32 if dtype is None else dtype
        item = torch.finfo(dtype).bits // 8
        buf = torch.empty((nbytes + item - 1) // item, dtype=dtype, device=device)
    return buf


def _check_noise(noise, x):
    """The dequantisation noise of an image call: None, or a device tensor of x's shape."""
    if noise is None:
        return
    _require_device_f32(noise, "noise")
    if noise.shape != x.shape:
        raise GbnfError("noise must have the shape of x")


def _check_log_w(log_w, n_components):
    _require_device_f32(log_w, "log_w")
    if tuple(log_w.shape) != (n_components,):
        raise GbnfError(f"log_w must be ({n_components},), got {tuple(log_w.shape)}")


class _Handle:
    """Owner of one library object: ``handle`` (a void*, None once closed) and ``_destroy``, the symbol that frees it."""

    _destroy = None

    def close(self):
        if getattr(self, "handle", None):
            getattr(lib(), self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_direction(direction):
    """``"forward"`` or ``"inverse"`` (which direction's on-data checks a numerics status reports); anything else: ValueError."""
    if direction not in ("forward", "inverse"):
        raise ValueError(f"direction must be 'forward' or 'inverse', got {direction!r}")
    return direction


class NativeFlow(_Handle):
    """One packed component on the device (gbnf_flow)."""

    _destroy = "gbnf_flow_destroy"

    def __init__(self, spec, math="default", per_step_activation=False):
        """``per_step_activation``: pack for the kernel variants that read the activation per step although this
        component uses one activation throughout (GBNF_CREATE_PER_STEP_ACTIVATION): lets it share a NativeMixture with
        components that do not (`--coupling_network random`); see ``flows_for_mixture``."""
        desc, keep = flow_desc_from_spec(spec)
        h = C.c_void_p()
        _check(lib().gbnf_flow_create_ex(C.byref(desc), MATH[math], 1 if per_step_activation else 0, C.byref(h)))
        del keep
        self.handle = h
        self.d = int(spec["d"])

    def info(self):
        ki = KernelInfo()
        _check(lib().gbnf_flow_info(self.handle, C.byref(ki)))
        return ki

    def numerics(self, direction="forward"):
        """gbnf_flow_numerics: (math mode of the next launch, demoted?, completed checks, worst relative error); no sync.
        ``direction="inverse"``: gbnf_flow_numerics_inverse, the checks of the z -> x direction (math mode and demoted are the
        handle's, shared by both directions)."""
        fn = lib().gbnf_flow_numerics_inverse if check_direction(direction) == "inverse" else lib().gbnf_flow_numerics
        st = NumericsStatus()
        _check(fn(self.handle, C.byref(st)))
        return st

    def forward(self, x, want_z=True, want_ldj=True, want_ll=False):
        """x (n,d) cuda f32 -> (z|None, ldj|None, ll|None); enqueued on the current stream."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        n = x.shape[0]
        z = torch.empty_like(x) if want_z else None
        ldj = torch.empty(n, dtype=torch.float32, device=x.device) if want_ldj else None
        ll = torch.empty(n, dtype=torch.float32, device=x.device) if want_ll else None
        _check(lib().gbnf_flow_forward(self.handle, _ptr(x), n, _ptr(z), _ptr(ldj), _ptr(ll), _stream_ptr()))
        return z, ldj, ll

    def inverse(self, z, want_ldj=True):
        """z (n,d) -> (x (n,d), log|det dx/dz| (n,) | None): the flow's steps last to first (gbnf_flow_inverse), in the handle's math
        mode (the same kernels under a runtime flag)."""
        import torch
        _require_device_f32(z, "z")
        if z.dim() != 2 or z.shape[1] != self.d:
            raise GbnfError(f"z must be (n,{self.d}), got {tuple(z.shape)}")
        n = z.shape[0]
        x = torch.empty_like(z)
        ldj = torch.empty(n, dtype=torch.float32, device=z.device) if want_ldj else None
        _check(lib().gbnf_flow_inverse(self.handle, _ptr(z), n, _ptr(x), _ptr(ldj), _stream_ptr()))
        return x, ldj


def image_flow_desc_from_spec(spec):
    """image flow spec (synth.synth_image_glow_spec / spec.image_spec_from_glow_module) -> (ctypes gbnf_image_flow_desc, keep-alive object)."""
    keep = _Keep()

    def conv(c):
        w = np.asarray(c["w"])
        cc = _Conv()
        cc.weight = keep.f32(w)
        for field, key in (("bias", "b"), ("actnorm_bias", "an_bias"), ("actnorm_logs", "an_logs"), ("logs", "logs")):
            if c[key] is not None:
                setattr(cc, field, keep.f32(np.asarray(c[key]).reshape(-1)))
        cc.out_channels, cc.in_channels, cc.kernel_size = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        return cc

    desc = _ImageFlowDesc()
    desc.channels, desc.height, desc.width = (int(v) for v in spec["input_size"])
    desc.n_levels = len(spec["levels"])
    desc.coupling = COUPLING[spec.get("coupling") or "affine"]
    desc.hidden = int(spec["hidden"])
    desc.bounds = float(spec.get("bounds", 0.9))
    levels = (_ImageLevel * desc.n_levels)()
    for l, lv in enumerate(spec["levels"]):
        steps = (_ImageStep * len(lv["steps"]))()
        for k, st in enumerate(lv["steps"]):
            s_ = _ImageStep()
            s_.actnorm_bias = keep.f32(np.asarray(st["an_bias"]).reshape(-1))
            s_.actnorm_logs = keep.f32(np.asarray(st["an_logs"]).reshape(-1))
            if st.get("perm_w") is not None:
                s_.perm_weight = keep.f32(st["perm_w"])
            else:
                s_.perm_indices = keep.i64(st["perm"])
            arr = (_Conv * len(st["convs"]))(*[conv(c) for c in st["convs"]])
            keep.refs.append(arr)
            s_.n_convs, s_.convs = len(st["convs"]), arr
            steps[k] = s_
        keep.refs.append(steps)
        levels[l].n_steps, levels[l].steps = len(lv["steps"]), steps
        if lv["split"] is not None:
            sp = conv(lv["split"])
            keep.refs.append(sp)
            levels[l].split_prior = C.pointer(sp)
    desc.levels = levels
    if spec.get("learn_top") is not None:
        top = conv(spec["learn_top"])
        keep.refs.append(top)
        desc.learn_top = C.pointer(top)
    return desc, keep


class NativeImageFlow(_Handle):
    """One packed image Glow component (gbnf_image_flow).  ``spec``: the image flow spec of ``synth.synth_image_glow_spec``
    / ``spec.image_spec_from_glow_module`` (numpy arrays)."""

    _destroy = "gbnf_image_flow_destroy"
    y_classes = 0              # (class defaults: a plain handle, also for an object wrapped around a raw handle without __init__)
    has_class_head = False

    def __init__(self, spec, math="default"):
        desc, keep = image_flow_desc_from_spec(spec)
        h = C.c_void_p()
        if math not in ("default", "f32", "f16x3"):
            raise GbnfError(f"image components run in math mode default | f32 | f16x3, not {math!r}")
        _check(lib().gbnf_image_flow_create_mode(C.byref(desc), MATH[math], C.byref(h)))
        del keep
        self.handle = h
        self.input_size = tuple(int(v) for v in spec["input_size"])
        self.n_levels = len(spec["levels"])
        zc, zh, zw, macs = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        _check(lib().gbnf_image_flow_info(h, C.byref(zc), C.byref(zh), C.byref(zw), C.byref(macs)))
        self.z_shape = (zc.value, zh.value, zw.value)
        self.macs_per_image = macs.value
        self._ws = None
        self.y_classes = 0
        self.has_class_head = False
        if spec.get("ycond") is not None:
            self.set_ycond(spec["ycond"])

    @property
    def deterministic(self):
        """Deterministic mode of the handle (gbnf_image_flow_get_deterministic / gbnf_image_flow_set_deterministic): while it is on,
        ``forward`` stores every log-det partial to a slot of its image and adds an image's slots in a fixed order -- z, ldj, ll (and
        y_logits) of identical calls are bit-identical and an image's ldj / ll do not depend on the batch around it.  Off at creation.
        A captured graph keeps the mode the handle had when it was captured.  The workspace is larger while the mode is on: every call
        asks the library for the size of the handle's current mode and grows the cached buffer when it is short."""
        on = C.c_int32()
        _check(lib().gbnf_image_flow_get_deterministic(self.handle, C.byref(on)))
        return bool(on.value)

    @deterministic.setter
    def deterministic(self, on):
        _check(lib().gbnf_image_flow_set_deterministic(self.handle, 1 if on else 0))
        # (the workspace size depends on the mode: the next call finds the cached buffer short and re-sizes it)

    def workspace_bytes(self, n):
        """Bytes of a call's workspace at a batch of n images in the handle's current mode (gbnf_image_flow_workspace_bytes)."""
        return _query_i64(lib().gbnf_image_flow_workspace_bytes, self.handle, int(n))

    def set_ycond(self, yc):
        """gbnf_image_flow_set_ycond: make the handle class-conditional.  ``yc``: the spec's ``"ycond"`` entry -- ``cond_w`` (2Cz, Y),
        ``cond_b``, ``cond_logs`` (2Cz,) of project_ycond and ``class_w`` (Y, Cz), ``class_b``, ``class_logs`` (Y,) of project_class
        (``class_w`` None: no class head), numpy arrays."""
        keep = _Keep()
        cz = self.z_shape[0]
        cond_w = np.asarray(yc["cond_w"], dtype=np.float32)
        if cond_w.ndim != 2 or cond_w.shape[0] != 2 * cz:
            raise GbnfError(f"ycond cond_w must be (2*{cz}, Y), got {cond_w.shape}")
        y = int(cond_w.shape[1])
        want = {"cond_b": (2 * cz,), "cond_logs": (2 * cz,)}
        head = yc.get("class_w") is not None
        if head:
            want.update({"class_w": (y, cz), "class_b": (y,), "class_logs": (y,)})
        ptrs = {"cond_w": keep.f32(cond_w)}
        for key, shape in want.items():
            a = np.asarray(yc[key], dtype=np.float32)
            if a.size != int(np.prod(shape)):
                raise GbnfError(f"ycond {key} must have shape {shape}, got {a.shape}")
            ptrs[key] = keep.f32(a.reshape(-1))
        null = C.c_void_p(0)
        as_vp = lambda k: C.cast(ptrs[k], C.c_void_p) if k in ptrs else null
        _check(lib().gbnf_image_flow_set_ycond(self.handle, y, as_vp("cond_w"), as_vp("cond_b"), as_vp("cond_logs"), as_vp("class_w"),
                                               as_vp("class_b"), as_vp("class_logs")))
        del keep
        self.y_classes, self.has_class_head = y, head

    def _check_y(self, y, n):
        _require_device_f32(y, "y")
        if y.dim() != 2 or tuple(y.shape) != (n, self.y_classes):
            raise GbnfError(f"y must be ({n},{self.y_classes}), got {tuple(y.shape)}")
        return y.contiguous()

    def prior_y(self, y, e=None, temperature=1.0, want_prior=True):
        """gbnf_image_flow_prior_y: y (n, Y) -> (mean (n,Cz), log-variance (n,Cz)) of the per-image prior and, with standard-normal
        ``e`` (n,Cz,Hz,Wz), the top latent z = mean + exp(log-variance) * temperature * e of a class-conditional draw
        (models/glow.py:116 as written).  Returns (mean, logvar, z | None); current stream."""
        import torch
        n = y.shape[0] if y is not None and hasattr(y, "shape") else 0
        y = self._check_y(y, n)
        cz = self.z_shape[0]
        ml = torch.empty((n, 2 * cz), dtype=torch.float32, device=y.device) if want_prior else None
        z = None
        if e is not None:
            _require_device_f32(e, "e")
            if tuple(e.shape) != (n,) + self.z_shape:
                raise GbnfError(f"e must be {(n,) + self.z_shape}, got {tuple(e.shape)}")
            e = e.contiguous()
            z = torch.empty_like(e)
        _check(lib().gbnf_image_flow_prior_y(self.handle, _ptr(y), n, _ptr(e), float(temperature), _ptr(ml), _ptr(z), _stream_ptr()))
        if ml is None:
            return None, None, z
        return ml[:, :cz], ml[:, cz:], z

    def numerics(self):
        """gbnf_image_flow_numerics: math mode the handle runs in, the create-time probe's verdict (worst_rel_err, demoted),
        calls that repaired an out-of-range image so far (checks); no synchronisation."""
        st = NumericsStatus()
        _check(lib().gbnf_image_flow_numerics(self.handle, C.byref(st)))
        return st

    def repair_counts(self):
        """gbnf_image_flow_repair_counts: what the same-call protocol behind the split-f16 pass has done so far (pinned
        words, no synchronisation): calls that marked an image, images re-evaluated on exact f32, on-data checks completed /
        failed, the worst relative difference a check has seen."""
        a, b, c, d, w = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_float()
        _check(lib().gbnf_image_flow_repair_counts(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(w)))
        return {"marked_calls": a.value, "repaired_images": b.value, "data_checks": c.value, "failed_checks": d.value,
                "worst_check_rel_err": w.value}

    def inverse_check_counts(self):
        """gbnf_image_flow_inverse_check_counts: the on-data checks of the z -> x direction (pinned words, no synchronisation):
        images checked / failed, the worst relative difference of x a check has seen."""
        c, d, w = C.c_int64(), C.c_int64(), C.c_float()
        _check(lib().gbnf_image_flow_inverse_check_counts(self.handle, C.byref(c), C.byref(d), C.byref(w)))
        return {"data_checks": c.value, "failed_checks": d.value, "worst_rel_err": w.value}

    def actnorm_stats(self, x, noise, index):
        """gbnf_image_flow_actnorm_stats: (mean (C,), var (C,)) device tensors of the tensor that reaches ActNorm2d number
        ``index`` (module order) on the batch -- the two numbers the reference's data-dependent initialisation needs
        (models/layers.py:473-486)."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        if noise is not None:
            _require_device_f32(noise, "noise")
        n = x.shape[0]
        self._ws = _grown(self._ws, self.workspace_bytes(n), x.device)
        mean = torch.empty(512, dtype=torch.float32, device=x.device)
        var = torch.empty(512, dtype=torch.float32, device=x.device)
        ch = C.c_int32()
        _check(lib().gbnf_image_flow_actnorm_stats(self.handle, _ptr(x), _ptr(noise), n, int(index), _ptr(mean), _ptr(var), C.byref(ch),
                                                   _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        return mean[: ch.value], var[: ch.value]

    def prior(self):
        """(mean (Cz,), log-variance (Cz,)) of the top prior, numpy."""
        buf = (C.c_float * (2 * self.z_shape[0]))()
        _check(lib().gbnf_image_flow_prior(self.handle, buf))
        a = np.frombuffer(buf, dtype=np.float32).copy()
        return a[: self.z_shape[0]], a[self.z_shape[0]:]

    def forward(self, x, noise=None, want_z=True, y=None, want_logits=None):
        """x (n,C,H,W) in [0,1] (+ dequantisation noise) -> (z | None, ldj (n,), ll (n,)); current stream.  A class-conditional
        handle needs ``y`` (n, Y) (gbnf_image_flow_forward_y) and returns (z | None, ldj, ll, y_logits (n, Y) | None): the logits
        when the handle has a class head (``want_logits`` False: not asked for)."""
        import torch
        if y is not None or self.y_classes > 0:
            return self._forward_y(x, noise, want_z, y, want_logits)
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        z = torch.empty((n,) + self.z_shape, dtype=torch.float32, device=x.device) if want_z else None
        ldj = torch.empty(n, dtype=torch.float32, device=x.device)
        ll = torch.empty(n, dtype=torch.float32, device=x.device)
        if n:
            self._ws = _grown(self._ws, self.workspace_bytes(n), x.device)
            _check(lib().gbnf_image_flow_forward(self.handle, _ptr(x), _ptr(noise), n, _ptr(z), _ptr(ldj), _ptr(ll),
                                                 _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        return z, ldj, ll

    def _forward_y(self, x, noise, want_z, y, want_logits):
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        if y is not None and self.y_classes > 0:
            y = self._check_y(y, n)
        if want_logits is None:
            want_logits = self.has_class_head
        z = torch.empty((n,) + self.z_shape, dtype=torch.float32, device=x.device) if want_z else None
        ldj = torch.empty(n, dtype=torch.float32, device=x.device)
        ll = torch.empty(n, dtype=torch.float32, device=x.device)
        logits = torch.empty((n, self.y_classes), dtype=torch.float32, device=x.device) if want_logits else None
        self._ws = _grown(self._ws, self.workspace_bytes(n), x.device)
        # (a null y, a handle without conditioning: the library refuses, nothing launched)
        _check(lib().gbnf_image_flow_forward_y(self.handle, _ptr(x), _ptr(noise), _ptr(y), n, _ptr(z), _ptr(ldj), _ptr(ll), _ptr(logits),
                                               _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        return z, ldj, ll, logits

    def forward_classes(self, x, noise=None, want_z=False, want_logits=False):
        """gbnf_image_flow_forward_classes: x (n,C,H,W) -> (z | None, ldj (n,), table (n, Y), y_logits (n, Y) | None) of a
        class-conditional handle, without labels: ``table[i, k]`` is the ll ``forward(x, noise, y=e_k)`` gives row i, for every class k,
        from ONE pass of the flow and one small launch (the class enters the top prior only).  Current stream."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        z = torch.empty((n,) + self.z_shape, dtype=torch.float32, device=x.device) if want_z else None
        ldj = torch.empty(n, dtype=torch.float32, device=x.device)
        table = torch.empty((n, self.y_classes), dtype=torch.float32, device=x.device)
        logits = torch.empty((n, self.y_classes), dtype=torch.float32, device=x.device) if want_logits else None
        self._ws = _grown(self._ws, self.workspace_bytes(n), x.device)
        # (a handle without conditioning, logits without a class head: the library refuses, nothing launched)
        _check(lib().gbnf_image_flow_forward_classes(self.handle, _ptr(x), _ptr(noise), n, _ptr(z), _ptr(ldj), _ptr(table), _ptr(logits),
                                                     _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        return z, ldj, table, logits

    def split_shapes(self):
        """(C_l/2, H_l, W_l) of the half each Split2d level drops (and re-draws on the way back), first level first."""
        c, h, w = self.input_size
        out = []
        for l in range(self.n_levels):
            c, h, w = c * 4, h // 2, w // 2
            if l < self.n_levels - 1:
                out.append((c // 2, h, w))
                c //= 2
        return out

    def encode(self, x, noise=None, want_ll=False):
        """gbnf_image_flow_encode: x (n,C,H,W) in [0,1] (+ dequantisation noise) -> (z, eps, ldj (n,), ll (n,) | None), the forward
        with the half each Split2d level drops kept: ``eps`` is a list with one (n, C_l/2, H_l, W_l) tensor per entry of
        ``split_shapes()`` (views of one allocation) -- the form ``inverse`` takes, so that ``inverse(z, eps, 1.0)`` returns the
        dequantised input (255 x + noise) / 256.  A class-conditional handle is accepted without ``y`` (x -> z, eps, ldj does not
        depend on it); its ll needs y, so ``want_ll`` raises there.  No gradient flows through the call.  Current stream."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        per = _query_i64(lib().gbnf_image_flow_eps_floats, self.handle)
        z = torch.empty((n,) + self.z_shape, dtype=torch.float32, device=x.device)
        flat = torch.empty(per * n, dtype=torch.float32, device=x.device)
        ldj = torch.empty(n, dtype=torch.float32, device=x.device)
        ll = torch.empty(n, dtype=torch.float32, device=x.device) if want_ll else None
        self._ws = _grown(self._ws, self.workspace_bytes(n), x.device)
        # (ll asked of a class-conditional handle: the library refuses, nothing launched)
        _check(lib().gbnf_image_flow_encode(self.handle, _ptr(x.contiguous()), _ptr(noise.contiguous() if noise is not None else None), n,
                                            _ptr(z), _ptr(flat), _ptr(ldj), _ptr(ll), _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        eps, off = [], 0
        for sh in self.split_shapes():
            k = n * sh[0] * sh[1] * sh[2]
            eps.append(flat[off:off + k].view((n,) + sh))
            off += k
        return z, eps, ldj, ll

    def inverse(self, z, eps=None, temperature=1.0):
        """z (n,Cz,Hz,Wz) -> x (n,C,H,W): the reference's Glow.decode(z, None, temperature) (gbnf_image_flow_inverse).
        ``eps``: one standard-normal tensor (n, C_l/2, H_l, W_l) per Split2d level, first level first (``split_shapes``);
        None draws them from torch's generator on z's device."""
        import torch
        _require_device_f32(z, "z")
        if z.dim() != 4 or tuple(z.shape[1:]) != self.z_shape:
            raise GbnfError(f"z must be (n,{self.z_shape}), got {tuple(z.shape)}")
        n = z.shape[0]
        shapes = self.split_shapes()
        if eps is None:
            eps = [torch.randn((n,) + sh, dtype=torch.float32, device=z.device) for sh in shapes]
        if len(eps) != len(shapes):
            raise GbnfError(f"eps needs {len(shapes)} tensors, got {len(eps)}")
        for e, sh in zip(eps, shapes):
            _require_device_f32(e, "eps")
            if tuple(e.shape) != (n,) + sh:
                raise GbnfError(f"eps tensor must be {(n,) + sh}, got {tuple(e.shape)}")
        per = _query_i64(lib().gbnf_image_flow_eps_floats, self.handle)
        flat = torch.cat([e.reshape(-1) for e in eps]) if eps else None
        if flat is not None and flat.numel() != per * n:
            raise GbnfError("eps size disagrees with gbnf_image_flow_eps_floats")
        x = torch.empty((n,) + self.input_size, dtype=torch.float32, device=z.device)
        if n:
            self._ws = _grown(self._ws, self.workspace_bytes(n), z.device)
            _check(lib().gbnf_image_flow_inverse(self.handle, _ptr(z.contiguous()), _ptr(flat), float(temperature), n, _ptr(x),
                                                 _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        return x

    _rho_ws = {}       # device -> workspace of rho_step (grown to the largest call so far)

    @staticmethod
    def rho_step(flows, x, noise, component, rho, step_size, y=None):
        """One iteration of ``update_rho`` for image ``component`` >= 1 on the device (gbnf_image_mixture_rho_step): the forwards of
        ``flows[0 .. component]`` (``NativeImageFlow`` handles in component order, the same ``noise`` for all, None = none) one after
        another on the current stream, the reference's un-normalised recursion, grad = mean(fixed_ll - new_ll) and
        ``rho[component] = clamp(rho[component] - step_size * grad, 0.01, 100)`` written IN PLACE into ``rho`` (a contiguous float32
        device tensor; no version counter moves).  -> stats (4,) device tensor: grad, rho before, rho after, |after - before|.  The
        (component + 1, n) log-likelihood table of the call stays in ``flows[component].rho_ll``.  ``y`` (n, Y) for class-conditional
        handles (gbnf_image_mixture_rho_step_y: every component's ll under its prior of each row's y; all handles conditioned, one Y)."""
        import torch
        component = int(component)
        flows = list(flows)[: max(component, 0) + 1]
        if component < 1 or len(flows) != component + 1:
            raise GbnfError(f"rho_step needs component >= 1 and handles of components 0 .. component, got component = {component} "
                            f"and {len(flows)} handle(s)")
        _require_device_f32(x, "x")
        _require_device_f32(rho, "rho")
        if x.dim() != 4 or x.shape[0] < 1 or any(tuple(x.shape[1:]) != f.input_size for f in flows):
            raise GbnfError(f"x must be (n,{flows[0].input_size}) with n >= 1 for every handle, got {tuple(x.shape)}")
        _check_noise(noise, x)
        if rho.dim() != 1 or rho.numel() <= component:
            raise GbnfError("rho has no entry for this component")
        n = x.shape[0]
        if y is not None:                       # (plain handles among them, two class counts: the library refuses, nothing launched)
            _require_device_f32(y, "y")
            if y.dim() != 2 or y.shape[0] != n or y.shape[1] != max(int(f.y_classes) for f in flows):
                raise GbnfError(f"y must be ({n}, y_classes), got {tuple(y.shape)}")
        handles = _handle_array(flows)
        nb = _query_i64(lib().gbnf_image_rho_step_workspace_bytes, handles, len(flows), n)
        ws = NativeImageFlow._rho_ws[x.device] = _grown(NativeImageFlow._rho_ws.get(x.device), nb, x.device)
        table = flows[component].rho_ll = torch.empty((component + 1, n), dtype=torch.float32, device=x.device)
        stats = torch.zeros(4, dtype=torch.float32, device=x.device)
        if y is not None:
            _check(lib().gbnf_image_mixture_rho_step_y(handles, component, _ptr(x), _ptr(noise), _ptr(y), n, _ptr(rho), float(step_size),
                                                       _ptr(table), _ptr(stats), _ptr(ws), ws.numel() * 4, _stream_ptr()))
            return stats
        _check(lib().gbnf_image_mixture_rho_step(handles, component, _ptr(x), _ptr(noise), n, _ptr(rho), float(step_size), _ptr(table),
                                                 _ptr(stats), _ptr(ws), ws.numel() * 4, _stream_ptr()))
        return stats

    _eval_ws = {}      # device -> workspace of evaluate (grown to the largest call so far)
    _eval_ll = {}      # device -> the (n_used, n) table of the last evaluate call (kept while the size repeats)

    @staticmethod
    def evaluate(flows, x, noise, component, rho, state, y=None):
        """One batch of the validation pass over image components on the device (gbnf_image_mixture_evaluate): the forwards of
        ``flows`` (``NativeImageFlow`` handles in component order: all of them are used, the same ``noise`` for all, None = none) one
        after another on the current stream, then the running sums of ``eval_accumulate`` with ``g = flows[component]`` ADDED into
        ``state`` (``eval_state``).  ``y`` (n, Y) for class-conditional handles (gbnf_image_mixture_evaluate_y: every component's ll under
        its prior of each row's y, and every component's share of the class loss into entries 10 - 12).  -> the call's (len(flows), n)
        log-likelihood table: scratch that is kept while the size repeats, so the next call of that size overwrites it."""
        import torch
        flows, component = list(flows), int(component)
        if not flows or not 0 <= component < len(flows):
            raise GbnfError(f"evaluate needs handles of components 0 .. n_used - 1 and 0 <= component < n_used, got component = {component} "
                            f"and {len(flows)} handle(s)")
        _require_device_f32(x, "x")
        _require_device_f32(rho, "rho")
        _require_eval_state(state)
        if x.dim() != 4 or x.shape[0] < 1 or any(tuple(x.shape[1:]) != f.input_size for f in flows):
            raise GbnfError(f"x must be (n,{flows[0].input_size}) with n >= 1 for every handle, got {tuple(x.shape)}")
        _check_noise(noise, x)
        if rho.dim() != 1 or rho.numel() < len(flows):
            raise GbnfError("rho is shorter than the handle list")
        n = x.shape[0]
        if y is not None:                       # (plain handles among them, two class counts, no head: the library refuses, nothing launched)
            _require_device_f32(y, "y")
            if y.dim() != 2 or y.shape[0] != n or y.shape[1] != max(int(f.y_classes) for f in flows):
                raise GbnfError(f"y must be ({n}, y_classes), got {tuple(y.shape)}")
        handles = _handle_array(flows)
        nb = _query_i64(lib().gbnf_image_mixture_evaluate_workspace_bytes, handles, len(flows), n)
        ws = NativeImageFlow._eval_ws[x.device] = _grown(NativeImageFlow._eval_ws.get(x.device), nb, x.device)
        table = NativeImageFlow._eval_ll.get(x.device)
        if table is None or tuple(table.shape) != (len(flows), n):
            table = NativeImageFlow._eval_ll[x.device] = torch.empty((len(flows), n), dtype=torch.float32, device=x.device)
        if y is not None:
            _check(lib().gbnf_image_mixture_evaluate_y(handles, len(flows), component, _ptr(x), _ptr(noise), _ptr(y), n, _ptr(rho), _ptr(table),
                                                       None, _ptr(state), _ptr(ws), ws.numel() * 4, _stream_ptr()))
            return table
        _check(lib().gbnf_image_mixture_evaluate(handles, len(flows), component, _ptr(x), _ptr(noise), n, _ptr(rho), _ptr(table), None,
                                                 _ptr(state), _ptr(ws), ws.numel() * 4, _stream_ptr()))
        return table


class _TrainerBase(_Handle):
    """What ``NativeTrainer`` and ``NativeImageTrainer`` share: the identity key, the deterministic switch, gbnf_opt_hyper and the
    update call.  A subclass names its library symbols and the attribute that holds the floats of the buffer ``apply_update`` walks."""

    _get_deterministic = _set_deterministic = _apply_update = None
    _update_floats = "grad_floats"

    def key(self):
        return tuple(t.data_ptr() for t in self._tensors)

    @property
    def deterministic(self):
        """Deterministic mode of the trainer (the class's gbnf_*_get_deterministic / gbnf_*_set_deterministic)."""
        on = C.c_int32(0)
        _check(getattr(lib(), self._get_deterministic)(self.handle, C.byref(on)))
        return bool(on.value)

    @deterministic.setter
    def deterministic(self, on):
        _check(getattr(lib(), self._set_deterministic)(self.handle, 1 if on else 0))
        self._deterministic = bool(on)

    def _hyper(self, state, lr, weight_decay=0.0, max_grad_norm=0.0, betas=(0.9, 0.999), eps=1e-8, bn_momentum=-1.0):
        """The gbnf_opt_hyper of the NEXT update of ``state`` (its ``step`` + 1)."""
        return _OptHyper(kind=OPT_KIND[state.kind], step=state.step + 1, lr=lr, beta1=betas[0], beta2=betas[1], eps=eps,
                         weight_decay=weight_decay, max_grad_norm=max_grad_norm, bn_momentum=bn_momentum)

    def apply_update(self, flat_grads, state, **hyper):
        """clip_grad_norm_ + one optimiser step on the bound tensors, in place, from a flat gradient buffer (gbnf_trainer_apply_update:
        the layout of ``backward``; gbnf_image_trainer_apply_update: the STEP layout).  ``state``: an ``OptState`` of this trainer,
        advanced by one step.  ``hyper``: lr, weight_decay, max_grad_norm, betas, eps.  -> stats (4,) device tensor: [1] gradient norm,
        [2] clip coefficient.  The parameters change behind autograd's back: no version counter moves (the modules' ``training_step``
        takes care of that)."""
        import torch
        _require_device_f32(flat_grads, "flat_grads")
        floats = getattr(self, self._update_floats)
        if flat_grads.numel() != floats:
            raise GbnfError(f"flat_grads has {flat_grads.numel()} elements, expected {floats}")
        state.check(self)
        h = self._hyper(state, **hyper)
        stats = torch.zeros(4, dtype=torch.float32, device=flat_grads.device)
        _check(getattr(lib(), self._apply_update)(self.handle, _ptr(flat_grads), _ptr(state.exp_avg), _ptr(state.exp_avg_sq), C.byref(h),
                                                  _ptr(stats), _stream_ptr()))
        state.step += 1
        return stats


class NativeImageTrainer(_TrainerBase):
    """Training path of one image Glow component (gbnf_image_trainer): forward on the LIVE device parameters and the backward pass,
    exact f32.

    ``dev_spec`` has the shape of an image flow spec (synth.synth_image_glow_spec) but every float array is a contiguous float32
    CUDA tensor -- the caller's parameter storage itself (``perm`` stays a host int64 array; ``perm_w`` is the composed C x C matrix
    of an InvertibleConv1x1).  Nothing is copied: the library keeps the addresses, this object keeps the tensors alive.  ``learn_top``
    is ignored (the top prior is the caller's).  ``ldj`` of ``forward`` EXCLUDES the log-determinants of the ``perm_w`` matrices.
    ``backward`` returns the parameters' gradients, ``backward_x`` the gradient with respect to x (with or without them).

    ``deterministic``: the weight gradients are flushed as per-slice partials and the log-det sums as per-wave slots, both added in
    a fixed order (gbnf_image_trainer_set_deterministic): ``forward``, ``backward``, ``nll_step`` and the step of
    ``boosted_nll_step`` are bit-reproducible for fixed inputs, parameters and batch size.  The workspaces grow; their sizes are
    asked of the library on every call."""

    _destroy = "gbnf_image_trainer_destroy"
    _get_deterministic, _set_deterministic = "gbnf_image_trainer_get_deterministic", "gbnf_image_trainer_set_deterministic"
    _apply_update, _update_floats = "gbnf_image_trainer_apply_update", "step_grad_floats"
    CONV_KEYS = ("w", "b", "an_bias", "an_logs", "logs")          # order of a convolution's arrays in the flat gradient buffer

    def __init__(self, dev_spec, deterministic=False):
        self._tensors = []
        self._regions = []          # (path, offset, shape) in the order of the flat gradient buffer
        self._region_tensors = []   # the bound tensor of each
        self._lu = {}               # (level, step) -> the LU factors bound there (bind_lu), in bind order
        self._top = None            # (weight | None, bias, logs) of learn_top_fn (bind_top)
        self._ycond = None          # the six tensors of project_ycond / project_class (bind_ycond)
        self.y_classes = 0
        self._off = 0
        fp = C.POINTER(C.c_float)
        keep = _Keep()

        def dptr(t):
            _require_device_f32(t, "parameter")
            self._tensors.append(t)
            return C.cast(C.c_void_p(t.data_ptr()), fp)

        def region(path, t):
            self._regions.append((path, self._off, tuple(t.shape)))
            self._region_tensors.append(t)
            self._off += t.numel()

        def conv(c, path):
            w = c["w"]
            cc = _Conv()
            cc.out_channels, cc.in_channels, cc.kernel_size = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
            for field, key in (("weight", "w"), ("bias", "b"), ("actnorm_bias", "an_bias"), ("actnorm_logs", "an_logs"), ("logs", "logs")):
                if c.get(key) is not None:
                    if key != "w" and c[key].numel() != cc.out_channels:
                        raise GbnfError(f"{path + (key,)}: {c[key].numel()} elements, expected {cc.out_channels}")
                    setattr(cc, field, dptr(c[key]))
                    region(path + (key,), c[key])
            return cc

        desc = _ImageFlowDesc()
        desc.channels, desc.height, desc.width = (int(v) for v in dev_spec["input_size"])
        desc.n_levels = len(dev_spec["levels"])
        desc.coupling = COUPLING[dev_spec.get("coupling") or "affine"]
        desc.hidden = int(dev_spec["hidden"])
        desc.bounds = float(dev_spec.get("bounds", 0.9))
        levels = (_ImageLevel * desc.n_levels)()
        ch, hh, ww = desc.channels, desc.height, desc.width
        self.level_pixels = []
        for l, lv in enumerate(dev_spec["levels"]):
            ch, hh, ww = ch * 4, hh // 2, ww // 2
            self.level_pixels.append(hh * ww)
            steps = (_ImageStep * len(lv["steps"]))()
            for k, st in enumerate(lv["steps"]):
                path = ("levels", l, "steps", k)
                s_ = _ImageStep()
                for key in ("an_bias", "an_logs"):
                    if st[key].numel() != ch:
                        raise GbnfError(f"{path + (key,)}: {st[key].numel()} elements, expected {ch}")
                s_.actnorm_bias = dptr(st["an_bias"])
                region(path + ("an_bias",), st["an_bias"])
                s_.actnorm_logs = dptr(st["an_logs"])
                region(path + ("an_logs",), st["an_logs"])
                if st.get("perm_w") is not None:
                    if tuple(st["perm_w"].shape) != (ch, ch):
                        raise GbnfError(f"{path + ('perm_w',)}: shape {tuple(st['perm_w'].shape)}, expected {(ch, ch)}")
                    s_.perm_weight = dptr(st["perm_w"])
                    region(path + ("perm_w",), st["perm_w"])
                else:
                    s_.perm_indices = keep.i64(st["perm"])
                arr = (_Conv * len(st["convs"]))(*[conv(c, path + ("convs", q)) for q, c in enumerate(st["convs"])])
                keep.refs.append(arr)
                s_.n_convs, s_.convs = len(st["convs"]), arr
                steps[k] = s_
            keep.refs.append(steps)
            levels[l].n_steps, levels[l].steps = len(lv["steps"]), steps
            if lv["split"] is not None:
                sp = conv(lv["split"], ("levels", l, "split"))
                keep.refs.append(sp)
                levels[l].split_prior = C.pointer(sp)
                ch //= 2
        desc.levels = levels
        self.input_size = (desc.channels, desc.height, desc.width)
        self.z_shape = (ch, hh, ww)
        h = C.c_void_p()
        _check(lib().gbnf_image_trainer_create(C.byref(desc), C.byref(h)))
        del keep
        self.handle = h
        self.grad_floats = _query_i64(lib().gbnf_image_trainer_grad_floats, h)
        if self.grad_floats != self._off:
            raise GbnfError("gradient-buffer layout mismatch between the library and the binding")
        self.device = self._tensors[0].device
        self._ws = None
        self._step_ws = None
        self._boost_ws = None       # workspace of boosted_nll_step
        self._layout_step()
        self._deterministic = False
        if deterministic:
            self.deterministic = True

    def workspace_bytes(self, n):
        """Bytes of the forward / backward workspace at a batch of n images (gbnf_image_trainer_workspace_bytes)."""
        return _query_i64(lib().gbnf_image_trainer_workspace_bytes, self.handle, int(n))

    def step_workspace_bytes(self, n):
        """Bytes of the workspace of ``nll_step`` at a batch of n images (gbnf_image_trainer_step_workspace_bytes)."""
        return _query_i64(lib().gbnf_image_trainer_step_workspace_bytes, self.handle, int(n))

    # ---- data-dependent ActNorm2d initialisation in one pass (gbnf_image_trainer_actnorm_init)
    def actnorm_count(self):
        """ActNorm2d layers of the component in module order: per FlowStep its own, then one behind each Conv2d of its coupling net."""
        k = C.c_int32()
        _check(lib().gbnf_image_trainer_actnorm_count(self.handle, C.byref(k)))
        return int(k.value)

    def actnorm_init_workspace_bytes(self, n):
        return _query_i64(lib().gbnf_image_trainer_actnorm_init_workspace_bytes, self.handle, int(n))

    def actnorm_init(self, x, noise, scale=1.0, skip=None, workspace=None):
        """The reference's first training-mode forward for every ActNorm2d at once: bias = -mean, logs = log(scale / (sqrt(var) + 1e-6))
        of the tensor that reaches each layer, written INTO the bound tensors in forward order, on the current stream, with no host
        read.  ``skip``: a sequence of ``actnorm_count()`` flags, true = leave that layer alone (it is initialised); None = all.
        ``workspace``: a device tensor of at least ``actnorm_init_workspace_bytes(n)`` bytes (None: allocated here; its contents
        on entry do not matter).  Returns nothing: run ``forward`` afterwards."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        flags = None
        if skip is not None:
            flags = np.ascontiguousarray([1 if s else 0 for s in skip], dtype=np.uint8)
            if flags.size != self.actnorm_count():
                raise GbnfError(f"skip has {flags.size} entries, the component has {self.actnorm_count()} ActNorm2d layers")
        workspace = _workspace_arg(workspace, lambda: self.actnorm_init_workspace_bytes(max(n, 1)), x.device)
        _check(lib().gbnf_image_trainer_actnorm_init(self.handle, _ptr(x), _ptr(noise), n, float(scale),
                                                     C.c_void_p(flags.ctypes.data) if flags is not None else C.c_void_p(0), _ptr(workspace),
                                                     workspace.numel() * workspace.element_size(), _stream_ptr()))

    # ---- the one-call training step (gbnf_image_trainer_nll_step / _apply_update)
    def _layout_step(self):
        """The STEP layout (include/gbnf.h): the regions of ``backward`` -- the composed matrix of an LU step reserved --, then per bound
        LU step lower / upper / log_s, then the top prior.  ``params`` / ``_sizes``: tensor | None and size per region, what
        ``OptState`` walks."""
        regions, tensors = [], []
        for (path, off, shape), t in zip(self._regions, self._region_tensors):
            reserved = path[-1] == "perm_w" and (path[1], path[3]) in self._lu
            regions.append((path, off, shape))
            tensors.append(None if reserved else t)
        off = self._off
        for (l, k), (lower, upper, log_s) in self._lu.items():
            for name, t in (("lower", lower), ("upper", upper), ("log_s", log_s)):
                regions.append((("levels", l, "steps", k, name), off, tuple(t.shape)))
                tensors.append(t)
                off += t.numel()
        if self._top is not None:
            for name, t in zip(("w", "b", "logs"), self._top):
                if t is not None:
                    regions.append((("learn_top", name), off, tuple(t.shape)))
                    tensors.append(t)
                    off += t.numel()
        if self._ycond is not None:
            for name, t in zip(self.YCOND_KEYS, self._ycond):
                regions.append((("ycond", name), off, tuple(t.shape)))
                tensors.append(t)
                off += t.numel()
        self.step_grad_floats = _query_i64(lib().gbnf_image_trainer_step_grad_floats, self.handle)
        if self.step_grad_floats != off:
            raise GbnfError("step gradient-buffer layout mismatch between the library and the binding")
        self._step_regions = regions
        self.params = tensors
        self._sizes = [int(np.prod(shape)) for _, _, shape in regions]

    def bind_lu(self, level, step, p, sign_s, lower, upper, log_s):
        """The live LU factors of one 1x1 step (gbnf_image_trainer_bind_lu; contiguous float32 device tensors): ``nll_step`` composes
        the step's bound ``perm_w`` from them and returns their gradients; the ``perm_w`` region of the step layout becomes reserved."""
        c = self._region_shape(("levels", int(level), "steps", int(step), "perm_w"))
        for name, t, shape in (("p", p, c), ("sign_s", sign_s, c and c[:1]), ("lower", lower, c), ("upper", upper, c), ("log_s", log_s, c and c[:1])):
            _require_device_f32(t, name)
            if c is not None and tuple(t.shape) != shape:
                raise GbnfError(f"bind_lu: {name} has shape {tuple(t.shape)}, expected {shape}")
        _check(lib().gbnf_image_trainer_bind_lu(self.handle, int(level), int(step), _ptr(p), _ptr(sign_s), _ptr(lower), _ptr(upper), _ptr(log_s)))
        self._tensors += [p, sign_s, lower, upper, log_s]
        self._lu[(int(level), int(step))] = (lower, upper, log_s)
        self._layout_step()

    def _region_shape(self, path):
        return next((shape for q, _, shape in self._regions if q == path), None)

    def bind_top(self, weight, bias, logs):
        """learn_top_fn's conv weight (or None), conv bias and logs (gbnf_image_trainer_bind_top): the learned top prior of ``nll_step``."""
        cz2 = 2 * self.z_shape[0]
        for name, t, numel in (("weight", weight, cz2 * cz2 * 9), ("bias", bias, cz2), ("logs", logs, cz2)):
            if t is None and name == "weight":
                continue
            _require_device_f32(t, name)
            if t.numel() != numel:
                raise GbnfError(f"bind_top: {name} has {t.numel()} elements, expected {numel}")
        _check(lib().gbnf_image_trainer_bind_top(self.handle, _ptr(weight), _ptr(bias), _ptr(logs)))
        self._tensors += [t for t in (weight, bias, logs) if t is not None]
        self._top = (weight, bias, logs)
        self._layout_step()

    YCOND_KEYS = ("cond_w", "cond_b", "cond_logs", "class_w", "class_b", "class_logs")     # order of the conditioning's regions

    def bind_ycond(self, cond_w, cond_b, cond_logs, class_w, class_b, class_logs):
        """The live tensors of project_ycond ((2Cz, Y), (2Cz,), (2Cz,)) and project_class ((Y, Cz), (Y,), (Y,))
        (gbnf_image_trainer_bind_ycond): the trainer becomes class-conditional -- ``nll_step`` and ``boosted_nll_step`` need ``y`` --
        and the STEP layout gains their six regions behind the top prior's."""
        cz = self.z_shape[0]
        _require_device_f32(cond_w, "cond_w")
        if cond_w.dim() != 2 or cond_w.shape[0] != 2 * cz:
            raise GbnfError(f"bind_ycond: cond_w has shape {tuple(cond_w.shape)}, expected (2*{cz}, Y)")
        y = int(cond_w.shape[1])
        ts = (cond_w, cond_b, cond_logs, class_w, class_b, class_logs)
        for name, t, numel in zip(self.YCOND_KEYS, ts, (2 * cz * y, 2 * cz, 2 * cz, y * cz, y, y)):
            _require_device_f32(t, name)
            if t.numel() != numel:
                raise GbnfError(f"bind_ycond: {name} has {t.numel()} elements, expected {numel}")
        _check(lib().gbnf_image_trainer_bind_ycond(self.handle, y, *[_ptr(t) for t in ts]))
        self._tensors += list(ts)
        self._ycond = ts
        self.y_classes = y
        self._layout_step()

    def _check_y(self, y, n):
        if self.y_classes == 0:
            raise GbnfError("the trainer has no conditioning bound (bind_ycond): it takes no y")
        _require_device_f32(y, "y")
        if tuple(y.shape) != (n, self.y_classes):
            raise GbnfError(f"y must be ({n},{self.y_classes}), got {tuple(y.shape)}")
        return y.contiguous()

    def step_views(self, flat):
        """{path: view} of a flat buffer in the STEP layout: the paths of ``backward`` plus (..., "lower" | "upper" | "log_s") of the
        bound LU steps, ("learn_top", "w" | "b" | "logs") and ("ycond", one of ``YCOND_KEYS``)."""
        if flat.numel() != self.step_grad_floats:
            raise GbnfError(f"flat has {flat.numel()} elements, expected {self.step_grad_floats}")
        return {path: flat[off: off + int(np.prod(shape))].view(shape) for path, off, shape in self._step_regions}

    def nll_step(self, x, noise, state, loss_scale=1.0, y=None, y_weight=0.01, **hyper):
        """One whole training step of this component on the device (gbnf_image_trainer_nll_step): 1x1 log-dets (LU matrices composed) ->
        forward on the live parameters -> loss_scale * mean nll and its seed -> backward -> log-det / LU / top-prior gradients -> clip ->
        optimiser update, no host read in between.  -> (stats (4,) device tensor: mean nll in nats (unscaled), norm of the scaled
        gradient, clip coefficient, 0; the flat unclipped scaled gradient in the STEP layout).
        With ``y`` (n, Y) on a trainer with conditioning bound (gbnf_image_trainer_nll_step_y): the loss is loss_scale * mean nll under
        the per-image prior + ``y_weight`` * mean cross-entropy of the class head against argmax y, and stats has 8 floats: [4] the
        mean cross-entropy, [5] the rows classified correctly, [6] [7] 0."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        if y is not None:
            y = self._check_y(y, n)
        state.check(self)
        h = self._hyper(state, **hyper)
        self._step_ws = _grown(self._step_ws, self.step_workspace_bytes(n), x.device)
        flat = torch.empty(self.step_grad_floats, dtype=torch.float32, device=x.device)
        if y is not None:
            stats = torch.zeros(8, dtype=torch.float32, device=x.device)
            _check(lib().gbnf_image_trainer_nll_step_y(self.handle, _ptr(x), _ptr(noise), _ptr(y), n, float(loss_scale), float(y_weight),
                                                       _ptr(flat), _ptr(state.exp_avg), _ptr(state.exp_avg_sq), C.byref(h), _ptr(stats),
                                                       _ptr(self._step_ws), self._step_ws.numel() * 4, _stream_ptr()))
            state.step += 1
            return stats, flat
        stats = torch.zeros(4, dtype=torch.float32, device=x.device)
        _check(lib().gbnf_image_trainer_nll_step(self.handle, _ptr(x), _ptr(noise), n, float(loss_scale), _ptr(flat), _ptr(state.exp_avg),
                                                 _ptr(state.exp_avg_sq), C.byref(h), _ptr(stats), _ptr(self._step_ws),
                                                 self._step_ws.numel() * 4, _stream_ptr()))
        state.step += 1
        return stats, flat

    def boosted_nll_step(self, fixed, x, noise, state, *, g_floor=-10.0, loss_scale=1.0, y=None, y_weight=0.01, **hyper):
        """``nll_step`` with the fixed-mixture term of the boosted image loss (gbnf_image_boosted_nll_step): the forward of ``fixed`` (a
        ``NativeImageFlow`` of the same input size) on the same ``(x, noise)``, G_nll = mean(-max(ll_G, g_floor)) (``g_floor``
        = -inf: no clamp), then the step of this component, unchanged -- the G term is never differentiated.  -> (stats (8,) device
        tensor: [0..3] as ``nll_step``, [4] G_nll in nats, [5] nll - G_nll, [6] rows below the floor or non-finite, [7] 0; the flat
        unclipped scaled gradient in the STEP layout).  With ``y`` (gbnf_image_boosted_nll_step_y; ``fixed`` and this trainer both
        class-conditional): stats (12,): [0..7] as ``nll_step`` with y, [8] G_nll, [9] nll - G_nll, [10] that row count, [11] 0."""
        import torch
        if not isinstance(fixed, NativeImageFlow) or not fixed.handle:
            raise GbnfError("fixed must be an open NativeImageFlow")
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size or tuple(fixed.input_size) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}) and fixed take the same images, got {tuple(x.shape)} and {fixed.input_size}")
        _check_noise(noise, x)
        n = x.shape[0]
        state.check(self)
        h = self._hyper(state, **hyper)
        if y is not None:
            y = self._check_y(y, n)
        query = lib().gbnf_image_boosted_step_workspace_bytes_y if y is not None else lib().gbnf_image_boosted_step_workspace_bytes
        ws = self._boost_ws = _grown(self._boost_ws, _query_i64(query, fixed.handle, self.handle, n), x.device)
        flat = torch.empty(self.step_grad_floats, dtype=torch.float32, device=x.device)
        if y is not None:
            stats = torch.zeros(12, dtype=torch.float32, device=x.device)
            _check(lib().gbnf_image_boosted_nll_step_y(fixed.handle, float(g_floor), self.handle, _ptr(x), _ptr(noise), _ptr(y), n,
                                                       float(loss_scale), float(y_weight), _ptr(flat), _ptr(state.exp_avg),
                                                       _ptr(state.exp_avg_sq), C.byref(h), _ptr(stats), _ptr(ws), ws.numel() * 4,
                                                       _stream_ptr()))
            state.step += 1
            return stats, flat
        stats = torch.zeros(8, dtype=torch.float32, device=x.device)
        _check(lib().gbnf_image_boosted_nll_step(fixed.handle, float(g_floor), self.handle, _ptr(x), _ptr(noise), n, float(loss_scale),
                                                 _ptr(flat), _ptr(state.exp_avg), _ptr(state.exp_avg_sq), C.byref(h), _ptr(stats), _ptr(ws),
                                                 ws.numel() * 4, _stream_ptr()))
        state.step += 1
        return stats, flat

    def _workspace(self, n):
        self._ws = _grown(self._ws, self.workspace_bytes(n), self.device)
        return self._ws

    def forward(self, x, noise=None, want_trace=True):
        """x (n,C,H,W) in [0,1] (+ dequantisation noise) -> (z, ldj (n,), trace | None) on the live parameters; current stream."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        _check_noise(noise, x)
        n = x.shape[0]
        z = torch.empty((n,) + self.z_shape, dtype=torch.float32, device=x.device)
        ldj = torch.empty(n, dtype=torch.float32, device=x.device)
        nt = _query_i64(lib().gbnf_image_trainer_trace_floats, self.handle, n)
        trace = torch.empty(nt, dtype=torch.float32, device=x.device)      # (the state storage of the pass: always needed)
        if n:
            ws = self._workspace(n)
            _check(lib().gbnf_image_trainer_forward(self.handle, _ptr(x), _ptr(noise), n, _ptr(z), _ptr(ldj), _ptr(trace), _ptr(ws),
                                                    ws.numel() * 4, _stream_ptr()))
        return z, ldj, (trace if want_trace else None)

    def backward(self, trace, g_z=None, g_ldj=None, out=None):
        """-> (flat gradient buffer, {path: view}) with path = ("levels", l, "steps", k, "an_bias" | "an_logs" | "perm_w") |
        ("levels", l, "steps", k, "convs", q, key) | ("levels", l, "split", key), key in CONV_KEYS.  ``out``: a flat buffer to
        ACCUMULATE into (None: a zeroed one)."""
        import torch
        _require_device_f32(trace, "trace")
        nt = _query_i64(lib().gbnf_image_trainer_trace_floats, self.handle, 1)
        if nt == 0 or trace.numel() % nt:
            raise GbnfError("trace is not one of this trainer's")
        n = trace.numel() // nt
        if g_z is not None:
            _require_device_f32(g_z, "g_z")
            if tuple(g_z.shape) != (n,) + self.z_shape:
                raise GbnfError(f"g_z must be {(n,) + self.z_shape}, got {tuple(g_z.shape)}")
        if g_ldj is not None:
            _require_device_f32(g_ldj, "g_ldj")
            if tuple(g_ldj.shape) != (n,):
                raise GbnfError(f"g_ldj must be ({n},), got {tuple(g_ldj.shape)}")
        if out is None:
            out = torch.zeros(self.grad_floats, dtype=torch.float32, device=trace.device)
        else:
            _require_device_f32(out, "out")
            if out.numel() != self.grad_floats:
                raise GbnfError(f"out has {out.numel()} elements, expected {self.grad_floats}")
        if n:
            ws = self._workspace(n)
            _check(lib().gbnf_image_trainer_backward(self.handle, _ptr(trace), n, _ptr(g_z), _ptr(g_ldj), _ptr(out), _ptr(ws),
                                                     ws.numel() * 4, _stream_ptr()))
        return out, {path: out[off: off + int(np.prod(shape))].view(shape) for path, off, shape in self._regions}

    def backward_x(self, trace, x, noise=None, g_z=None, g_ldj=None, want_grads=False, out=None, g_x=None, workspace=None):
        """The gradient with respect to the input (gbnf_image_trainer_backward_x): ``x`` and ``noise`` as the ``forward`` that left
        ``trace`` took them.  -> g_x (n, C, H, W); with ``want_grads`` (or a flat buffer ``out`` to accumulate into) also the weight
        gradients, (g_x, flat, {path: view}) as ``backward`` returns them.  Without them no weight-gradient kernel runs: the form
        the score uses.  ``g_x``: a tensor to ACCUMULATE into (None: a new one, stored).  ``workspace``: a contiguous device tensor
        to use instead of the trainer's own (its size is checked by the library)."""
        import torch
        _require_device_f32(trace, "trace")
        _require_device_f32(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_size:
            raise GbnfError(f"x must be (n,{self.input_size}), got {tuple(x.shape)}")
        n = x.shape[0]
        nt = _query_i64(lib().gbnf_image_trainer_trace_floats, self.handle, n)
        if trace.numel() != nt:
            raise GbnfError(f"trace has {trace.numel()} floats: not this trainer's at n = {n} ({nt})")
        _check_noise(noise, x)
        if g_z is not None:
            _require_device_f32(g_z, "g_z")
            if tuple(g_z.shape) != (n,) + self.z_shape:
                raise GbnfError(f"g_z must be {(n,) + self.z_shape}, got {tuple(g_z.shape)}")
        if g_ldj is not None:
            _require_device_f32(g_ldj, "g_ldj")
            if tuple(g_ldj.shape) != (n,):
                raise GbnfError(f"g_ldj must be ({n},), got {tuple(g_ldj.shape)}")
        if out is not None:
            _require_device_f32(out, "out")
            if out.numel() != self.grad_floats:
                raise GbnfError(f"out has {out.numel()} elements, expected {self.grad_floats}")
        elif want_grads:
            out = torch.zeros(self.grad_floats, dtype=torch.float32, device=x.device)
        accumulate = g_x is not None
        if accumulate:
            _require_device_f32(g_x, "g_x")
            if g_x.shape != x.shape:
                raise GbnfError(f"g_x must have the shape of x, got {tuple(g_x.shape)}")
        else:
            g_x = torch.empty_like(x)
        if n:
            ws = _check_workspace(self._workspace(n) if workspace is None else workspace)
            _check(lib().gbnf_image_trainer_backward_x(self.handle, _ptr(trace), _ptr(x), _ptr(noise), n, _ptr(g_z), _ptr(g_ldj), _ptr(out),
                                                       _ptr(g_x), 1 if accumulate else 0, _ptr(ws), ws.numel() * ws.element_size(),
                                                       _stream_ptr()))
        if out is None:
            return g_x
        return g_x, out, {path: out[off: off + int(np.prod(shape))].view(shape) for path, off, shape in self._regions}


class NativeTrainer(_TrainerBase):
    """Training path of one component (gbnf_trainer): forward on the LIVE device parameters and the backward pass.

    ``dev_spec`` has the shape of a flow spec (spec.py) but every float array is a contiguous float32 CUDA tensor --
    the caller's parameter / buffer storage itself (``perm`` stays a host int64 array).  Nothing is copied: the
    library keeps the addresses, this object keeps the tensors alive.

    ``math``: "f16x3" (default: the fast sweeps, operands beyond +-65504 saturate and are counted) or "bf16x6" (range-safe: f32
    range in every sweep, the re-pack and the weight gradients) or "repair" (f16x3 first; a call that met the range is re-run in
    bf16x6 within the same call, decided on the device: GBNF_MATH_DEFAULT) -- gbnf_trainer_create_mode.  A geometry without the
    kernels of the mode raises GbnfError; nothing falls back.

    ``deterministic``: the weight gradients are flushed as per-chunk partials and added in a fixed order
    (gbnf_trainer_set_deterministic): ``backward``, ``nll_step`` and ``boosted_nll_step`` are bit-reproducible for fixed inputs,
    parameters and batch size.  A call that would run the per-step kernels (unordered float atomics) raises GbnfError with the
    library's reason.  The workspaces grow: every helper asks the library for the size at every call."""

    _destroy = "gbnf_trainer_destroy"
    _get_deterministic, _set_deterministic = "gbnf_trainer_get_deterministic", "gbnf_trainer_set_deterministic"
    _apply_update, _update_floats = "gbnf_trainer_apply_update", "grad_floats"
    TRAIN_MATH = {"f16x3": MATH["f16x3"], "bf16x6": MATH["bf16x6"], "repair": MATH["default"]}

    def __init__(self, dev_spec, math="f16x3", deterministic=False):
        import torch
        if math not in self.TRAIN_MATH:
            raise GbnfError(f"NativeTrainer: math must be one of {sorted(self.TRAIN_MATH)}, got {math!r}")
        self.math = math
        self._tensors = []        # keep-alive; also the identity check for re-creation
        self.params = []          # tensors in the order of the flat gradient buffer (None = reserved, unused region)
        self._sizes = []
        keep = []
        K = len(dev_spec["steps"])
        self.d = d = int(dev_spec["d"])
        fp = C.POINTER(C.c_float)

        def dptr(t, numel):
            _require_device_f32(t, "parameter")
            if t.numel() != numel:
                raise GbnfError(f"parameter has {t.numel()} elements, expected {numel}")
            self._tensors.append(t)
            return C.cast(C.c_void_p(t.data_ptr()), fp)

        def region(t, numel):
            self.params.append(t)
            self._sizes.append(numel)

        def net(n):
            arr = (_Linear * len(n["layers"]))()
            for k, (w, b) in enumerate(n["layers"]):
                out_f, in_f = int(w.shape[0]), int(w.shape[1])
                arr[k] = _Linear(dptr(w, out_f * in_f), dptr(b, out_f), out_f, in_f)
                region(w, out_f * in_f)
                region(b, out_f)
            keep.append(arr)
            return _Net(ACT[n["act"]], len(n["layers"]), arr)

        desc = _FlowDesc()
        desc.kind = KIND[dev_spec["kind"]]
        desc.d = d
        desc.n_steps = K
        desc.coupling = COUPLING[dev_spec.get("coupling") or "affine"]
        hk = _Keep()
        if dev_spec["kind"] == "glow":
            steps = (_GlowStep * K)()
            for k, st in enumerate(dev_spec["steps"]):
                region(st["an_bias"], d)
                region(st["an_logs"], d)
                steps[k] = _GlowStep(dptr(st["an_bias"], d), dptr(st["an_logs"], d), hk.i64(st["perm"]), net(st["net"]))
            desc.glow_steps = steps
        else:
            steps = (_RealNVPStep * K)()
            for k, st in enumerate(dev_spec["steps"]):
                s = _RealNVPStep()
                s.flipped = int(bool(st["flipped"]))
                bn = st["bn"]
                s.has_batch_norm = int(bn is not None)
                if bn is not None:
                    s.bn_log_gamma = dptr(bn["log_gamma"], d)
                    s.bn_beta = dptr(bn["beta"], d)
                    s.bn_running_mean = dptr(bn["running_mean"], d)
                    s.bn_running_var = dptr(bn["running_var"], d)
                    s.bn_eps = float(bn["eps"])
                    region(bn["log_gamma"], d)
                    region(bn["beta"], d)
                else:
                    region(None, d)
                    region(None, d)
                s.t_net = net(st["t_net"])
                s.s_net = net(st["s_net"])
                steps[k] = s
            desc.realnvp_steps = steps
        h = C.c_void_p()
        _check(lib().gbnf_trainer_create_mode(C.byref(desc), self.TRAIN_MATH[math], C.byref(h)))
        self.handle = h
        # BatchNorm on batch statistics (the reference's train() mode): bind the buffers that receive them
        self.has_batch_stats = False
        if dev_spec["kind"] == "realnvp":
            bound = 0
            for k, st in enumerate(dev_spec["steps"]):
                bn = st["bn"]
                if bn is not None and bn.get("batch_mean") is not None:
                    for t in (bn["batch_mean"], bn["batch_var"]):
                        _require_device_f32(t, "batch statistics buffer")
                        self._tensors.append(t)
                    _check(lib().gbnf_trainer_bind_batch_stats(h, k, C.c_void_p(bn["batch_mean"].data_ptr()),
                                                               C.c_void_p(bn["batch_var"].data_ptr())))
                    bound += 1
            n_bn = sum(1 for st in dev_spec["steps"] if st["bn"] is not None)
            self.has_batch_stats = bound == n_bn and n_bn > 0
        self.batch_stats = False
        self.grad_floats = _query_i64(lib().gbnf_trainer_grad_floats, h)
        if self.grad_floats != sum(self._sizes):
            raise GbnfError("gradient-buffer layout mismatch between the library and the binding")
        self._ws = None
        self._step_ws = None
        self._boost_ws = None
        self.device = self._tensors[0].device
        self._deterministic = False
        if deterministic:
            self.deterministic = True

    def nll_step(self, x, state, rows=None, **hyper):
        """One whole training step of this component on the device (gbnf_trainer_nll_step): [x[rows]] -> forward on the live parameters ->
        NLL and its seed -> backward -> clip -> optimiser update, no host read in between.  ``rows``: int64 device indices into x
        (repeats allowed) or None.  ``hyper`` as for ``apply_update``, plus bn_momentum (>= 0: batch-statistics mode also moves the
        bound running statistics).  -> (stats (4,) device tensor: nll, gradient norm, clip coefficient, 0; the flat unclipped gradient)."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        n_x = n = x.shape[0]
        if rows is not None:
            if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.int64 or not rows.is_contiguous() or rows.dim() != 1:
                raise GbnfError("rows must be a contiguous 1-d int64 tensor on the device")
            n = rows.shape[0]
        state.check(self)
        h = self._hyper(state, **hyper)
        nb = C.c_int64()         # (the size query and the cached-buffer test in line: this is the per-step path, see _grown)
        _check(lib().gbnf_trainer_step_workspace_bytes(self.handle, n, C.byref(nb)))
        if self._step_ws is None or self._step_ws.numel() * 4 < nb.value or self._step_ws.device != x.device:
            self._step_ws = _grown(None, nb.value, x.device)
        flat = torch.empty(self.grad_floats, dtype=torch.float32, device=x.device)
        stats = torch.zeros(4, dtype=torch.float32, device=x.device)
        _check(lib().gbnf_trainer_nll_step(self.handle, _ptr(x), n_x, _ptr(rows), n, _ptr(flat), _ptr(state.exp_avg), _ptr(state.exp_avg_sq),
                                           C.byref(h), _ptr(stats), _ptr(self._step_ws), self._step_ws.numel() * 4, _stream_ptr()))
        state.step += 1
        return stats, flat

    def boosted_nll_step(self, mixture, n_fixed, rho, x, u, state, beta=1.0, want_rows=False, **hyper):
        """One whole BOOSTED training step of this component on the device (gbnf_boosted_nll_step): the mixture log-density of the
        ``n_fixed`` fixed components of ``mixture`` (a ``NativeMixture``) under ``rho`` -> boosting weights -> the weighted resample on the
        caller's uniforms ``u`` ((n,) float32 in [0,1), on the device) -> ``nll_step`` on the drawn rows, no host read in between.
        ``hyper`` as for ``nll_step``.  -> (stats (8,) device tensor: nll, gradient norm, clip coefficient, 0, G_nll, effective sample
        size, bad-weight count, 0; the flat unclipped gradient; the drawn rows (n,) int64 when ``want_rows``, else None)."""
        import torch
        _require_device_f32(x, "x")
        _require_device_f32(u, "u")
        _require_device_f32(rho, "rho")
        if x.dim() != 2 or x.shape[1] != self.d or x.shape[0] < 1:
            raise GbnfError(f"x must be (n,{self.d}) with n >= 1, got {tuple(x.shape)}")
        n = x.shape[0]
        if u.dim() != 1 or u.shape[0] != n:
            raise GbnfError(f"u must be ({n},), one uniform per draw, got {tuple(u.shape)}")
        n_fixed = int(n_fixed)
        if rho.dim() != 1 or rho.numel() < n_fixed:
            raise GbnfError("rho shorter than n_fixed")
        state.check(self)
        h = self._hyper(state, **hyper)
        nb = C.c_int64()         # (in line as in nll_step)
        _check(lib().gbnf_boosted_step_workspace_bytes(mixture.handle, n_fixed, self.handle, n, C.byref(nb)))
        if self._boost_ws is None or self._boost_ws.numel() * 8 < nb.value or self._boost_ws.device != x.device:
            self._boost_ws = _grown(None, nb.value, x.device, torch.float64)
        flat = torch.empty(self.grad_floats, dtype=torch.float32, device=x.device)
        stats = torch.zeros(8, dtype=torch.float32, device=x.device)
        rows = torch.empty(n, dtype=torch.int64, device=x.device) if want_rows else None
        _check(lib().gbnf_boosted_nll_step(mixture.handle, n_fixed, _ptr(rho), float(beta), self.handle, _ptr(x), n, _ptr(u), _ptr(flat),
                                           _ptr(state.exp_avg), _ptr(state.exp_avg_sq), C.byref(h), _ptr(stats), _ptr(rows),
                                           _ptr(self._boost_ws), self._boost_ws.numel() * 8, _stream_ptr()))
        state.step += 1
        return stats, flat, rows

    def set_batch_stats(self, on):
        """RealNVP BatchNorm on batch statistics (True = the reference's train() mode) or running statistics (False)."""
        on = bool(on)
        if on != self.batch_stats:
            _check(lib().gbnf_trainer_set_batch_stats(self.handle, int(on)))
            self.batch_stats = on

    def forward(self, x, want_trace=False):
        """-> (z, ldj) or (z, ldj, trace): ``trace`` holds every step's normalised state; passing it to ``backward``
        saves that call the forward sweep (valid while the parameters are unchanged)."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        n = x.shape[0]
        z = torch.empty_like(x)
        ldj = torch.empty(n, dtype=torch.float32, device=x.device)
        trace = None
        if want_trace:
            trace = torch.empty(_query_i64(lib().gbnf_trainer_trace_floats, self.handle, n), dtype=torch.float32, device=x.device)
        if n:
            _check(lib().gbnf_trainer_forward(self.handle, _ptr(x), n, _ptr(z), _ptr(ldj), _ptr(trace), _stream_ptr()))
        return (z, ldj, trace) if want_trace else (z, ldj)

    def backward(self, x, g_z=None, g_ldj=None, want_gx=False, trace=None):
        """-> (g_x | None, [gradient per entry of ``self.params`` (views of one flat buffer; None for reserved regions)])."""
        import torch
        _require_device_f32(x, "x")
        n = x.shape[0]
        for t, name in ((g_z, "g_z"), (g_ldj, "g_ldj")):
            if t is not None:
                _require_device_f32(t, name)
        flat = torch.zeros(self.grad_floats, dtype=torch.float32, device=x.device)
        g_x = torch.empty_like(x) if want_gx else None
        if n:
            nb = C.c_int64()         # (in line as in nll_step)
            _check(lib().gbnf_trainer_workspace_bytes(self.handle, n, C.byref(nb)))
            if self._ws is None or self._ws.numel() * 4 < nb.value or self._ws.device != x.device:
                self._ws = _grown(None, nb.value, x.device)
            _check(lib().gbnf_trainer_backward(self.handle, _ptr(x), n, _ptr(trace), _ptr(g_z), _ptr(g_ldj), _ptr(g_x), _ptr(flat),
                                               _ptr(self._ws), self._ws.numel() * 4, _stream_ptr()))
        grads, off = [], 0
        for t, size in zip(self.params, self._sizes):
            grads.append(None if t is None else flat[off:off + size].view(t.shape))
            off += size
        return g_x, grads

    def backward_x_workspace_bytes(self, n):
        return _query_i64(lib().gbnf_trainer_backward_x_workspace_bytes, self.handle, int(n))

    def backward_x(self, x, g_z=None, g_ldj=None, trace=None, g_x=None, workspace=None):
        """The gradient with respect to the input alone (gbnf_trainer_backward_x): the sweeps of ``backward`` with no weight-gradient
        launch, no partial-sum reduce and no gradient buffer -> g_x (n, d), bit-equal to ``backward(..., want_gx=True)[0]``.  ``g_x``:
        a tensor to ACCUMULATE into (None: a new one, stored).  ``trace`` as for ``backward``.  ``workspace``: a contiguous device
        tensor to use instead of the trainer's own (its size is checked by the library).  A trainer in batch-statistics mode raises
        GbnfError: that gradient needs the batch sums of the full backward."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        n = x.shape[0]
        if g_z is not None:
            _require_device_f32(g_z, "g_z")
            if g_z.shape != x.shape:
                raise GbnfError(f"g_z must be ({n},{self.d}), got {tuple(g_z.shape)}")
        if g_ldj is not None:
            _require_device_f32(g_ldj, "g_ldj")
            if tuple(g_ldj.shape) != (n,):
                raise GbnfError(f"g_ldj must be ({n},), got {tuple(g_ldj.shape)}")
        if trace is not None:
            _require_device_f32(trace, "trace")
            nt = _query_i64(lib().gbnf_trainer_trace_floats, self.handle, n)
            if trace.numel() != nt:
                raise GbnfError(f"trace has {trace.numel()} floats: not this trainer's at n = {n} ({nt})")
        accumulate = g_x is not None
        if accumulate:
            _require_device_f32(g_x, "g_x")
            if g_x.shape != x.shape:
                raise GbnfError(f"g_x must have the shape of x, got {tuple(g_x.shape)}")
        else:
            g_x = torch.empty_like(x)
        if not n:
            return g_x
        if workspace is None:
            ws = self._bx_ws = _grown(getattr(self, "_bx_ws", None), self.backward_x_workspace_bytes(n), x.device)
        else:
            ws = _check_workspace(workspace)
        _check(lib().gbnf_trainer_backward_x(self.handle, _ptr(x), n, _ptr(trace), _ptr(g_z), _ptr(g_ldj), _ptr(g_x), 1 if accumulate else 0,
                                             _ptr(ws), ws.numel() * ws.element_size(), _stream_ptr()))
        return g_x

    def repair_count(self, reset=False):
        """Forward / backward calls of this trainer whose bf16x6 re-run actually ran (a "repair" trainer; always 0 otherwise).
        Synchronises with the device (gbnf_trainer_repair_count)."""
        n = C.c_int64(0)
        _check(lib().gbnf_trainer_repair_count(self.handle, C.byref(n), 1 if reset else 0))
        return int(n.value)


class OptState:
    """Caller-owned optimiser state of one trainer's parameters for ``NativeTrainer.apply_update`` / ``nll_step`` (or those of a
    ``NativeImageTrainer``, whose step layout sizes it: create it after ``bind_lu`` / ``bind_top``): ``exp_avg`` and
    ``exp_avg_sq`` as flat device tensors in the layout of the flat gradient buffer (None for SGD), ``step`` = updates taken so far,
    ``kind`` = "adamw" | "sgd".  It maps one to one onto the state of a ``torch.optim.AdamW`` (``load_from`` / ``store_to``)."""

    def __init__(self, trainer, kind="adamw", device=None):
        import torch
        if kind not in OPT_KIND:
            raise GbnfError(f"OptState: kind must be one of {sorted(OPT_KIND)}, got {kind!r}")
        self.kind = kind
        self.step = 0
        self.grad_floats = self._floats_of(trainer)
        self._shapes = [(None if t is None else tuple(t.shape), size) for t, size in zip(trainer.params, trainer._sizes)]
        self.exp_avg_device = device = trainer.device if device is None else device
        self.exp_avg = self.exp_avg_sq = None
        if kind == "adamw":
            self.exp_avg = torch.zeros(self.grad_floats, dtype=torch.float32, device=device)
            self.exp_avg_sq = torch.zeros(self.grad_floats, dtype=torch.float32, device=device)

    @staticmethod
    def _floats_of(trainer):
        """Floats of the buffer the trainer's update walks: an image trainer's STEP layout, a tabular trainer's gradient buffer."""
        return getattr(trainer, "step_grad_floats", None) or trainer.grad_floats

    def check(self, trainer):
        if self.grad_floats != self._floats_of(trainer):
            raise GbnfError("OptState belongs to a trainer of another geometry")

    def _views(self, flat):
        out, off = [], 0
        for shape, size in self._shapes:
            out.append(None if shape is None or flat is None else flat[off:off + size].view(shape))
            off += size
        return out

    def views(self):
        """-> (exp_avg views, exp_avg_sq views), one per entry of ``trainer.params`` (None for reserved regions and for SGD)."""
        return self._views(self.exp_avg), self._views(self.exp_avg_sq)

    def load_from(self, optimizer, params):
        """Take exp_avg / exp_avg_sq / step of every tensor of ``params`` (``trainer.params``; matched by identity) from a
        ``torch.optim.AdamW``; a parameter the optimiser has no state for yet keeps zeros.  Steps must agree across parameters."""
        import torch
        if self.kind != "adamw":
            raise GbnfError("OptState.load_from: only AdamW has state")
        steps = set()
        with torch.no_grad():
            for p, m, v in zip(params, *self.views()):
                st = optimizer.state.get(p) if p is not None else None
                if not st:
                    continue
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                steps.add(int(st["step"]))
        if len(steps) > 1:
            raise GbnfError(f"OptState.load_from: the parameters are at different steps {sorted(steps)}")
        self.step = steps.pop() if steps else 0
        return self

    def store_to(self, optimizer, params):
        """The other direction: write this state into the ``torch.optim.AdamW``'s per-parameter state (created where missing)."""
        import torch
        if self.kind != "adamw":
            raise GbnfError("OptState.store_to: only AdamW has state")
        with torch.no_grad():
            for p, m, v in zip(params, *self.views()):
                if p is None:
                    continue
                st = optimizer.state[p]
                if "exp_avg" in st:
                    st["exp_avg"].copy_(m)
                    st["exp_avg_sq"].copy_(v)
                else:
                    st["exp_avg"], st["exp_avg_sq"] = m.clone(), v.clone()
                old = st.get("step")
                st["step"] = torch.full_like(old, float(self.step)) if isinstance(old, torch.Tensor) else torch.tensor(float(self.step))
        return self


def saturation_count(reset=False):
    """How many waves stored a split-f16 operand beyond +-65504 (it saturates there) since the last reset: 0 for
    z-scored data on a trained flow.  Synchronises with the device (gbnf_saturation_count)."""
    n = C.c_int64(0)
    _check(lib().gbnf_saturation_count(C.byref(n), 1 if reset else 0))
    return int(n.value)


def training_saturation_count(reset=False):
    """The part of ``saturation_count`` that came from TRAINING launches (forward / backward sweeps of a trainer, its weight re-pack):
    they saturate and are not repaired -- non-zero means steps with wrong gradients (gbnf_training_saturation_count).  Synchronises."""
    n = C.c_int64(0)
    _check(lib().gbnf_training_saturation_count(C.byref(n), 1 if reset else 0))
    return int(n.value)


def activation_pattern(spec):
    """The activations of a component's coupling nets, step by step (a hashable)."""
    if spec["kind"] == "glow":
        return tuple(st["net"]["act"] for st in spec["steps"])
    return tuple((st["t_net"]["act"], st["s_net"]["act"]) for st in spec["steps"])


def needs_per_step_activation(specs):
    """True when the components cannot share one uniform-activation kernel: some component mixes activations, or two
    components use different ones (the reference's `--coupling_network random`, models/glow.py:295-296)."""
    pats = {activation_pattern(s) for s in specs}
    return len(pats) > 1 or any(len(set(p)) > 1 for p in pats)


def flows_for_mixture(specs, math="default"):
    """NativeFlow handles of `specs` that are guaranteed to fit one NativeMixture."""
    per_step = needs_per_step_activation(specs)
    return [NativeFlow(s, math=math, per_step_activation=per_step) for s in specs]


def mixture_from_specs(specs, math="default"):
    """(NativeMixture, [NativeFlow]) of `specs`.  A mixture is one launch on ONE kernel variant; when the components
    would individually end up on different variants (different activations, or a geometry only the per-step-activation
    supersets cover) all of them are created for those supersets."""
    flows = flows_for_mixture(specs, math=math)
    try:
        return NativeMixture(flows), flows
    except GbnfError:
        flows = [NativeFlow(s, math=math, per_step_activation=True) for s in specs]
        return NativeMixture(flows), flows


class NativeMixture(_Handle):
    """C same-architecture components behind one launch (gbnf_mixture)."""

    _destroy = "gbnf_mixture_destroy"

    def __init__(self, flows):
        self.flows = list(flows)           # keeps the NativeFlow handles alive
        h = C.c_void_p()
        _check(lib().gbnf_mixture_create(_handle_array(self.flows), len(self.flows), C.byref(h)))
        self.handle = h
        self.d = self.flows[0].d

    @property
    def n_components(self):
        return len(self.flows)

    def numerics(self):
        """gbnf_mixture_numerics: the mixture's effective math mode and the state of its numerics guard; no sync."""
        st = NumericsStatus()
        _check(lib().gbnf_mixture_numerics(self.handle, C.byref(st)))
        return st

    def set_base(self, mean=None, std=None):
        if mean is None:
            _check(lib().gbnf_mixture_set_base(self.handle, None, None))
            return
        m = np.ascontiguousarray(np.asarray(mean, dtype=np.float32))
        s = np.ascontiguousarray(np.asarray(std, dtype=np.float32))
        if m.shape != (self.d,) or s.shape != (self.d,):
            raise GbnfError(f"base mean/std must have shape ({self.d},)")
        _check(lib().gbnf_mixture_set_base(self.handle, _fptr(m), _fptr(s)))

    def component_log_prob(self, x, c_begin=0, c_end=None, out=None):
        """ll (c_end-c_begin, n) for components [c_begin, c_end) in one launch."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        c_end = self.n_components if c_end is None else c_end
        n = x.shape[0]
        if out is None:
            out = torch.empty((c_end - c_begin, n), dtype=torch.float32, device=x.device)
        else:
            _require_device_f32(out, "out")
            if tuple(out.shape) != (c_end - c_begin, n):
                raise GbnfError("out has the wrong shape")
        _check(lib().gbnf_mixture_component_log_prob(
            self.handle, C.c_void_p(x.data_ptr() if n else 0), n, c_begin, c_end,
            C.c_void_p(out.data_ptr() if out.numel() else 0), _stream_ptr()))
        return out

    def component_forward(self, x, c_begin=0, c_end=None, want_z=True, want_ldj=True, want_ll=False):
        """(z (C',n,d), ldj (C',n), ll (C',n)) of components [c_begin, c_end) in ONE launch (gbnf_mixture_component_forward):
        the reference's per-component calls ``model(x=x, components=c)`` of one batch, all at once."""
        import torch
        _require_device_f32(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        c_end = self.n_components if c_end is None else c_end
        n, k = x.shape[0], c_end - c_begin
        z = torch.empty((k, n, self.d), dtype=torch.float32, device=x.device) if want_z else None
        ldj = torch.empty((k, n), dtype=torch.float32, device=x.device) if want_ldj else None
        ll = torch.empty((k, n), dtype=torch.float32, device=x.device) if want_ll else None
        if n and k:
            _check(lib().gbnf_mixture_component_forward(self.handle, C.c_void_p(x.data_ptr()), n, c_begin, c_end,
                                                        _ptr(z), _ptr(ldj), _ptr(ll), _stream_ptr()))
        return z, ldj, ll

    def prepared_component_log_prob(self, x, out, c_begin=0, c_end=None, col_offset=0):
        """Bind every argument once and return ``launch(stream_ptr)``: the per-call host cost is then one ctypes
        call (for latency-sensitive loops such as bench.py's pipeline).  ``out`` is a (c_end-c_begin, >= n) table;
        this batch's log-densities go to columns [col_offset, col_offset + n) (rows keep out's row stride)."""
        _require_device_f32(x, "x")
        if not out.is_cuda or out.dtype.is_floating_point is False or out.stride(1) != 1:
            raise GbnfError("out must be a float32 device table with unit column stride")
        c_end = self.n_components if c_end is None else c_end
        n = x.shape[0]
        if out.shape[0] != c_end - c_begin or out.shape[1] < col_offset + n or x.shape[1] != self.d:
            raise GbnfError("prepared_component_log_prob: shape mismatch")
        fn, h = lib().gbnf_mixture_component_log_prob_strided, self.handle
        stride = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], n)
        xp = C.c_void_p(x.data_ptr())
        op = C.c_void_p(out.data_ptr() + 4 * col_offset)
        keep = (x, out)

        def launch(stream_ptr, _keep=keep):
            rc = fn(h, xp, n, c_begin, c_end, op, stride, stream_ptr)
            if rc:
                _check(rc)
        return launch

    def prepared_group_log_prob(self, xs, out, c_begin=0, c_end=None):
        """Bound launch of ONE kernel over a group of batches: xs = list of (n,d) device tensors (same n), ``out`` a
        (c_end-c_begin, len(xs)*n) table; batch b lands in columns [b*n, (b+1)*n).  Returns ``launch(stream_ptr)``."""
        c_end = self.n_components if c_end is None else c_end
        n = xs[0].shape[0]
        for t in xs:
            _require_device_f32(t, "x")
            if tuple(t.shape) != (n, self.d):
                raise GbnfError("all batches of a group must be (n, d) with the same n")
        _require_device_f32(out, "out")
        if tuple(out.shape) != (c_end - c_begin, len(xs) * n):
            raise GbnfError("out must be (components, len(xs) * n)")
        fn, h = lib().gbnf_mixture_component_log_prob_multi, self.handle
        arr = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        nb, stride, op = len(xs), len(xs) * n, C.c_void_p(out.data_ptr())
        keep = (list(xs), out, arr)

        def launch(stream_ptr, _keep=keep):
            rc = fn(h, arr, nb, n, c_begin, c_end, op, stride, stream_ptr)
            if rc:
                _check(rc)
        return launch

    def log_prob(self, x, rho, n_used=None, ll_out=None, out=None):
        """The measured path: G (n,) = mixture log-density over components [0, n_used)."""
        import torch
        _require_device_f32(x, "x")
        _require_device_f32(rho, "rho")
        n_used = self.n_components if n_used is None else int(n_used)
        n = x.shape[0]
        if ll_out is None:
            ll_out = torch.empty((n_used, n), dtype=torch.float32, device=x.device)
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=x.device)
        if rho.numel() < n_used:
            raise GbnfError("rho shorter than n_used")
        _check(lib().gbnf_mixture_log_prob(
            self.handle, C.c_void_p(x.data_ptr() if n else 0), n, n_used, C.c_void_p(rho.data_ptr()),
            C.c_void_p(ll_out.data_ptr() if ll_out.numel() else 0),
            C.c_void_p(out.data_ptr() if n else 0), _stream_ptr()))
        return out, ll_out

    def rho_step(self, x, component, rho, step_size):
        """One iteration of ``update_rho`` for ``component`` >= 1 on the device (gbnf_mixture_rho_step): the log-densities of components
        [0, component], the reference's un-normalised recursion, grad = mean(fixed_ll - new_ll) and
        ``rho[component] = clamp(rho[component] - step_size * grad, 0.01, 100)`` written IN PLACE into ``rho`` (a contiguous float32
        device tensor; no version counter moves).  -> stats (4,) device tensor: grad, rho before, rho after, |after - before|.  The
        (component + 1, n) log-likelihood table of the call stays in ``self.rho_ll``."""
        import torch
        _require_device_f32(x, "x")
        _require_device_f32(rho, "rho")
        component = int(component)
        if x.dim() != 2 or x.shape[1] != self.d or x.shape[0] < 1:
            raise GbnfError(f"x must be (n,{self.d}) with n >= 1, got {tuple(x.shape)}")
        if rho.dim() != 1 or rho.numel() <= component:
            raise GbnfError("rho has no entry for this component")
        n = x.shape[0]
        self.rho_ll = torch.empty((component + 1, n), dtype=torch.float32, device=x.device)
        stats = torch.zeros(4, dtype=torch.float32, device=x.device)
        _check(lib().gbnf_mixture_rho_step(self.handle, C.c_void_p(x.data_ptr()), n, component, C.c_void_p(rho.data_ptr()),
                                           float(step_size), C.c_void_p(self.rho_ll.data_ptr()), C.c_void_p(stats.data_ptr()),
                                           _stream_ptr()))
        return stats

    def evaluate(self, x, component, rho, state, n_used=None, want_G=False):
        """One batch of the validation pass on the device (gbnf_mixture_evaluate): the log-densities of components [0, n_used) in ONE
        flow launch, then the running sums of ``eval_accumulate`` with ``g = component`` ADDED into ``state`` (``eval_state``); no
        host read.  -> G (n,) with ``want_G``, else None.  The (n_used, n) table of the call stays in ``self.eval_ll``: scratch kept
        on the handle while the size repeats, so the next call of that size overwrites it."""
        import torch
        _require_device_f32(x, "x")
        _require_device_f32(rho, "rho")
        _require_eval_state(state)
        n_used = self.n_components if n_used is None else int(n_used)
        if x.dim() != 2 or x.shape[1] != self.d:
            raise GbnfError(f"x must be (n,{self.d}), got {tuple(x.shape)}")
        if rho.dim() != 1 or rho.numel() < n_used:
            raise GbnfError("rho shorter than n_used")
        n = x.shape[0]
        table = getattr(self, "eval_ll", None)
        if table is None or tuple(table.shape) != (n_used, n) or table.device != x.device:
            table = self.eval_ll = torch.empty((n_used, n), dtype=torch.float32, device=x.device)
        ws = _eval_workspace(x.device, n)
        G = torch.empty(n, dtype=torch.float32, device=x.device) if want_G else None
        if not 0 <= int(component) < n_used:
            raise GbnfError(f"component = {component} outside [0, {n_used})")
        if n == 0:                              # (an empty batch adds nothing, `batches` included: there is nothing to launch)
            return G
        _check(lib().gbnf_mixture_evaluate(self.handle, _ptr(x), n, n_used, int(component), _ptr(rho), _ptr(table), _ptr(G), _ptr(state), _ptr(ws),
                                           ws.numel() * ws.element_size(), _stream_ptr()))
        return G


class Comm:
    """An RCCL communicator owned by the library (gbnf_comm): the exchange of the component-sharded group without
    torch.distributed on the data path.  ``Comm.from_torch_distributed()`` builds one for the ranks of an initialised process
    group (the 128-byte id travels through a broadcast of that group -- set-up only); ``Comm(0, 1, Comm.unique_id())`` is a
    one-rank communicator."""

    def __init__(self, rank, world, unique_id):
        if len(unique_id) != 128:
            raise GbnfError("an RCCL unique id has 128 bytes")
        buf = (C.c_uint8 * 128)(*unique_id)
        h = C.c_void_p()
        _check(lib().gbnf_comm_create(buf, int(rank), int(world), C.byref(h)))
        self.handle, self.rank, self.world = h, int(rank), int(world)

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        _check(lib().gbnf_comm_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def probe():
        """Local, non-collective: can this process build a communicator at all (librccl loadable, its symbols bound, an id
        obtainable)?  -> (ok, reason)."""
        try:
            Comm.unique_id()
            return True, ""
        except Exception as e:                 # GbnfError (dlopen / UNSUPPORTED), OSError (library missing)
            return False, f"{type(e).__name__}: {e}"

    @classmethod
    def from_torch_distributed(cls, group=None):
        """The ranks AGREE before anything that can block: every rank probes locally, the flags meet in one
        all_reduce(MIN), and only then does rank 0 broadcast the id (always: ``None`` if it could not make one) and every rank
        enter ncclCommInitRank.  A rank that cannot load RCCL therefore makes every rank raise GbnfError instead of leaving its
        peers inside a collective."""
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            return cls(0, 1, cls.unique_id())
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        if world == 1:
            return cls(0, 1, cls.unique_id())
        ok, why = cls.probe()
        # the hand-shake tensor lives where the group can reduce it: a group whose backend string mentions nccl (plain "nccl", or a
        # composite like "cpu:gloo,cuda:nccl") takes a device tensor, anything else a host tensor
        use_cuda = "nccl" in str(dist.get_backend(group)).lower() and torch.cuda.is_available()
        dev = torch.device("cuda", torch.cuda.current_device()) if use_cuda else torch.device("cpu")
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag.item()) == 0:
            raise GbnfError("no library communicator: " + (why if not ok else "another rank cannot load RCCL"))
        uid = None
        if rank == 0:
            try:
                uid = cls.unique_id()
            except Exception:
                uid = None
        box = [uid]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if box[0] is None:
            raise GbnfError("no library communicator: rank 0 could not obtain an RCCL unique id")
        return cls(rank, world, box[0])

    def close(self):
        if getattr(self, "handle", None) is not None and _lib is not None:
            _lib.gbnf_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupLaunch:
    """One group of the component-sharded mixture bound to its buffers (gbnf_mixture_group_log_prob): ``mix`` = this rank's
    components, ``comm`` = a ``Comm`` or None (one rank, no exchange), ``xs`` = the group's resident (n, d) batches,
    ``ll_local`` (C/W, S n), ``ll_full`` (C, S n), ``G`` (S n).  ``launch(stream_ptr)`` enqueues flow launch -> all-gather ->
    recursion on that stream with ONE library call; with ``graph=True`` the sequence is captured once into a HIP graph and
    ``launch`` is a hipGraphLaunch (falls back to the plain call, with ``self.graph_error`` set, when the capture is refused)."""

    def __init__(self, mix, comm, xs, n_components, rho, ll_local, ll_full, G, graph=True):
        n = xs[0].shape[0]
        for t in list(xs) + [rho, ll_local, G] + ([ll_full] if ll_full is not None else []):
            _require_device_f32(t, "tensor")
        world = comm.world if comm is not None else 1
        if n_components % world or tuple(ll_local.shape) != (n_components // world, len(xs) * n) or G.numel() != len(xs) * n:
            raise GbnfError("GroupLaunch: buffer shapes do not match the group")
        if comm is not None and (ll_full is None or tuple(ll_full.shape) != (n_components, len(xs) * n)):
            raise GbnfError("GroupLaunch: ll_full must be (C, len(xs) * n)")
        self._keep = (mix, comm, list(xs), rho, ll_local, ll_full, G)
        self._arr = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        self._args = (mix.handle, comm.handle if comm is not None else C.c_void_p(0), self._arr, len(xs), n, int(n_components),
                      _ptr(rho), _ptr(ll_local), _ptr(ll_full), _ptr(G))
        self.graph, self.graph_error = None, None
        if graph:
            h = C.c_void_p()
            rc = lib().gbnf_group_graph_create(*self._args, C.byref(h))
            if rc == 0:
                self.graph = h
            else:
                self.graph_error = lib().gbnf_last_error().decode(errors="replace")

    def launch(self, stream_ptr):
        if self.graph is not None:
            rc = lib().gbnf_group_graph_launch(self.graph, stream_ptr)
        else:
            rc = lib().gbnf_mixture_group_log_prob(*self._args, stream_ptr)
        if rc:
            _check(rc)

    def close(self):
        if getattr(self, "graph", None) is not None and _lib is not None:
            _lib.gbnf_group_graph_destroy(self.graph)
            self.graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mixture_lse(ll, rho, out=None):
    """Recursive prefix-normalised log-sum-exp of (C,n) per-component log-densities."""
    import torch
    _require_device_f32(ll, "ll")
    _require_device_f32(rho, "rho")
    if ll.dim() != 2:
        raise GbnfError("ll must be (C, n)")
    c, n = ll.shape
    if rho.numel() < c:
        raise GbnfError("rho shorter than the number of components")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=ll.device)
    _check(lib().gbnf_mixture_lse(C.c_void_p(ll.data_ptr() if n else 0), n, C.c_void_p(rho.data_ptr()), c, n,
                                  C.c_void_p(out.data_ptr() if n else 0), _stream_ptr()))
    return out


# ---- the validation pass: running sums of a loader's batches in a device state (gbnf_eval_accumulate and the calls around it)
def eval_state(device):
    """A zeroed evaluation state: ``EVAL_STATE_DOUBLES`` float64 on ``device`` (layout: ``EVAL_STATE`` / include/gbnf.h).  The
    evaluate calls only ever add to it; read it once after the last batch."""
    import torch
    return torch.zeros(EVAL_STATE_DOUBLES, dtype=torch.float64, device=device)


def _require_eval_state(state):
    import torch
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.float64 or not state.is_contiguous() \
            or state.numel() < EVAL_STATE_DOUBLES:
        raise GbnfError(f"state must be a contiguous float64 device tensor of {EVAL_STATE_DOUBLES} entries (native.eval_state)")
    return state


_eval_ws = {}      # device -> the partial-sum scratch of the accumulate calls


def _eval_workspace(device, n):
    import torch
    ws = _eval_ws[device] = _grown(_eval_ws.get(device), _query_i64(lib().gbnf_eval_workspace_bytes, n), device, torch.float64)
    return ws


def eval_accumulate(ll, rho, component, state, want_G=False, workspace=None):
    """gbnf_eval_accumulate: the sums of one batch's (n_used, n) table ``ll`` of per-component log-likelihoods (float32 on the device,
    unit column stride; the rows may be strided) ADDED into ``state``: rows, batches, sum G_ll (the recursion of ``mixture_lse``, bit
    for bit), sum g_ll (row ``component``), sum (G_ll - g_ll), sum E_ll (the rho-weighted mean of the rows), their batch means, the
    non-finite rows.  Two launches, no host read.  -> G (n,) with ``want_G``, else None.  ``workspace``: a float64 device tensor of
    gbnf_eval_workspace_bytes (default: one per device, so calls on one device must not run on two streams at once)."""
    import torch
    if not isinstance(ll, torch.Tensor) or not ll.is_cuda or ll.dtype != torch.float32 or ll.dim() != 2 or (ll.shape[1] > 1 and ll.stride(1) != 1):
        raise GbnfError("ll must be a (n_used, n) float32 device table with unit column stride")
    _require_device_f32(rho, "rho")
    _require_eval_state(state)
    n_used, n = ll.shape
    if rho.dim() != 1 or rho.numel() < n_used:
        raise GbnfError("rho shorter than the number of components")
    stride = ll.stride(0) if n_used > 1 else max(n, 1)
    ws = _eval_workspace(ll.device, n) if workspace is None else workspace
    G = torch.empty(n, dtype=torch.float32, device=ll.device) if want_G else None
    if n == 0 and 0 <= int(component) < n_used:      # (an empty table has no address to hand over; the library adds nothing for it)
        return G
    _check(lib().gbnf_eval_accumulate(_ptr(ll), stride, n_used, n, _ptr(rho), int(component), _ptr(G), _ptr(state), _ptr(ws),
                                      ws.numel() * ws.element_size(), _stream_ptr()))
    return G


def eval_accumulate_class_loss(y_logits, y, rho, c, state, n_used=None, workspace=None):
    """gbnf_eval_accumulate_class_loss: component ``c``'s share of the class loss of one batch ADDED into entries 10 - 12 of ``state``:
    with w = rho[c] / sum(rho[:n_used]),  w sum_i CE_i,  w mean_i CE_i  and  w #{argmax logits_i == argmax y_i}, where
    CE_i = logsumexp(y_logits_i) - y_logits_i[argmax y_i] in float64 (F.cross_entropy(y_logits, argmax(y)); the first largest entry
    wins both argmaxes).  y_logits, y: (n, Y) float32 on the device, 1 <= Y <= 256.  ``n_used`` defaults to ``rho.numel()``."""
    _require_device_f32(y_logits, "y_logits")
    _require_device_f32(y, "y")
    _require_device_f32(rho, "rho")
    _require_eval_state(state)
    if y_logits.dim() != 2 or y.shape != y_logits.shape:
        raise GbnfError("y_logits and y must both be (n, Y)")
    n, Y = y_logits.shape
    n_used = rho.numel() if n_used is None else int(n_used)
    if rho.dim() != 1 or rho.numel() < n_used:
        raise GbnfError("rho shorter than n_used")
    ws = _eval_workspace(y.device, n) if workspace is None else workspace
    _check(lib().gbnf_eval_accumulate_class_loss(_ptr(y_logits), _ptr(y), n, Y, _ptr(rho), n_used, int(c), _ptr(state), _ptr(ws),
                                                 ws.numel() * ws.element_size(), _stream_ptr()))


# ---- all mixture weights at once: EM over a cached (C, n) table of component log-likelihoods (gbnf_weights_em, gbnf_weights_to_rho)
def weights_state(device):
    """An evaluation state of ``weights_em``: ``WEIGHTS_STATE_DOUBLES`` float64 on ``device`` (layout: ``WEIGHTS_STATE`` / include/gbnf.h).
    The call overwrites it."""
    import torch
    return torch.zeros(WEIGHTS_STATE_DOUBLES, dtype=torch.float64, device=device)


def _require_weights_state(state):
    import torch
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.float64 or not state.is_contiguous() \
            or state.numel() < WEIGHTS_STATE_DOUBLES:
        raise GbnfError(f"state must be a contiguous float64 device tensor of {WEIGHTS_STATE_DOUBLES} entries (native.weights_state)")
    return state


_weights_ws = {}      # device -> the control words and partial sums of weights_em (grown to the largest call so far)


def weights_em(ll, rho, max_iters, tol, state=None, workspace=None):
    """gbnf_weights_em: EM for the weights of the mixture over the (C, n) table ``ll`` of per-component log-likelihoods (float32 on the
    device, unit column stride; the rows may be strided), started at ``rho[:C] / sum(rho[:C])`` and run until
    ``|L_t - L_{t-1}| <= tol`` or ``max_iters`` updates (``tol <= 0``: exactly ``max_iters``), all on the device: ``max_iters + 2``
    launches, of which those behind the stopping evaluation return at once; no host read.  -> ``state`` (``WEIGHTS_STATE``; given or
    new), overwritten.  ``rho`` is only read.  ``workspace``: a float64 device tensor of gbnf_weights_em_workspace_bytes (default:
    one per device, so calls on one device must not run on two streams at once)."""
    import torch
    if not isinstance(ll, torch.Tensor) or not ll.is_cuda or ll.dtype != torch.float32 or ll.dim() != 2 or (ll.shape[1] > 1 and ll.stride(1) != 1):
        raise GbnfError("ll must be a (C, n) float32 device table with unit column stride")
    _require_device_f32(rho, "rho")
    n_comp, n = ll.shape
    if rho.dim() != 1 or rho.numel() < n_comp:
        raise GbnfError("rho shorter than the number of components")
    state = weights_state(ll.device) if state is None else _require_weights_state(state)
    stride = ll.stride(0) if n_comp > 1 else max(n, 1)
    nb = _query_i64(lib().gbnf_weights_em_workspace_bytes, n_comp, n)
    if workspace is None:
        workspace = _weights_ws[ll.device] = _grown(_weights_ws.get(ll.device), nb, ll.device, torch.float64)
    # (an empty table has no address to hand over; no row of it is read: rho's stands in)
    llp = C.c_void_p(ll.data_ptr() if ll.numel() else rho.data_ptr())
    _check(lib().gbnf_weights_em(llp, stride, n_comp, n, C.c_void_p(rho.data_ptr()), int(max_iters), float(tol),
                                 C.c_void_p(state.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                 workspace.numel() * workspace.element_size(), _stream_ptr()))
    return state


def weights_to_rho(state, rho, rho_min=0.01, rho_max=100.0, n_components=None):
    """gbnf_weights_to_rho: ``rho[c] = clamp(w_c * sum(rho[:C]), rho_min, rho_max)`` for c < C in place, with w the weights in ``state``
    (``weights_em``); entries at and beyond C stay.  Nothing is written after a bad start; twice the number of clamped entries is
    added into ``state[7]``.  ``n_components`` defaults to ``rho.numel()``.  The caller moves rho's version counter."""
    _require_weights_state(state)
    _require_device_f32(rho, "rho")
    n_comp = rho.numel() if n_components is None else int(n_components)
    if rho.dim() != 1 or rho.numel() < n_comp:
        raise GbnfError("rho shorter than the number of components")
    _check(lib().gbnf_weights_to_rho(C.c_void_p(state.data_ptr()), n_comp, float(rho_min), float(rho_max), C.c_void_p(rho.data_ptr()),
                                     _stream_ptr()))
    return rho


def weights_table_room(table, n_components, capacity, filled, n, device):
    """The (n_components, >= filled + n) float32 device table ``fit_weights`` fills batch by batch: made at ``capacity`` columns on the
    first batch, and doubled (its ``filled`` columns copied) should a loader yield more rows than its dataset holds."""
    import torch
    if table is not None and filled + n <= table.shape[1]:
        return table
    grown = torch.empty((n_components, max(capacity, filled + n, 0 if table is None else 2 * table.shape[1])), dtype=torch.float32,
                        device=device)
    if table is not None:
        grown[:, :filled].copy_(table[:, :filled])
    return grown


def fit_weights_on_table(table, rho, n_components, max_iters, tol, write):
    """The tail of both modules' ``fit_weights``: ``weights_em`` on the filled (C, rows) table, ``weights_to_rho`` on ``rho`` with
    ``write`` (and rho's version counter moved, as the rho update does), ONE host read -> the report dict."""
    import torch
    with torch.cuda.device(table.device):
        state = weights_em(table, rho, max_iters, tol)
        if write:
            weights_to_rho(state, rho, n_components=n_components)
            # the kernel wrote rho behind autograd's back: move its version counter as the rho update does
            torch.autograd.graph.increment_version([rho])
    out = weights_report(state, n_components)
    if out.pop("bad_start"):
        raise ValueError("fit_weights: no usable row (every row holds a NaN or +inf, or is -inf under every component), or rho has a "
                         f"negative or non-finite entry or sums to 0; rows used {out['rows']}, excluded {out['excluded']}")
    out.pop("delta")
    return out


def weights_report(state, n_components):
    """The dict ``fit_weights`` returns, from ONE host read of a ``weights_em`` state."""
    s = state.tolist()
    S = WEIGHTS_STATE
    flags = int(s[S["flags"]])
    return {"nll_before": -s[S["L0"]], "nll_after": -s[S["L"]], "iters": int(s[S["iters"]]), "converged": bool(s[S["converged"]]),
            "rows": int(s[S["rows"]]), "excluded": int(s[S["excluded"]]), "weights": s[S["weights"]:S["weights"] + n_components],
            "clamped": flags // 2, "bad_start": bool(flags & 1), "delta": s[S["delta"]]}


def class_posterior(class_ll, log_prior=None, want_post=True, want_pred=False):
    """gbnf_class_posterior: class_ll (n, Y) device float32 (a table of ``NativeImageFlow.forward_classes``, or the mixture's),
    ``log_prior`` (Y,) device log-probabilities or None for uniform -> (log_px (n,), log_post (n, Y) | None, pred (n,) int32 | None):
    log_px = LSE_k(log_prior + class_ll), log_post = log_prior + class_ll - log_px, pred = the first largest entry of log_post."""
    import torch
    _require_device_f32(class_ll, "class_ll")
    if class_ll.dim() != 2:
        raise GbnfError(f"class_ll must be (n, Y), got {tuple(class_ll.shape)}")
    class_ll = class_ll.contiguous()
    n, Y = class_ll.shape
    if log_prior is not None:
        _require_device_f32(log_prior, "log_prior")
        if tuple(log_prior.shape) != (Y,):
            raise GbnfError(f"log_prior must be ({Y},), got {tuple(log_prior.shape)}")
        log_prior = log_prior.contiguous()
    log_px = torch.empty(n, dtype=torch.float32, device=class_ll.device)
    post = torch.empty((n, Y), dtype=torch.float32, device=class_ll.device) if want_post else None
    pred = torch.empty(n, dtype=torch.int32, device=class_ll.device) if want_pred else None
    if n:
        _check(lib().gbnf_class_posterior(_ptr(class_ll), _ptr(log_prior), n, Y, _ptr(log_px), _ptr(post), _ptr(pred), _stream_ptr()))
    return log_px, post, pred


def tabular_score_seed(z, r=None, base=None, want_ll=False):
    """gbnf_score_seed, the explicit tabular entry point: z (n, d) device float32, ``r`` (n,) or None for 1, ``base`` = (mean (d,),
    std (d,)) device tensors or None for N(0, I) -> (g_z = -r (z - mean) / std^2, g_ldj = r[, ll (n,) = sum_j log N(z_j; mean_j,
    std_j) with ``want_ll``; the caller adds ldj])."""
    import torch
    _require_device_f32(z, "z")
    if z.dim() != 2:
        raise GbnfError(f"z must be (n, d), got {tuple(z.shape)}")
    n, d = int(z.shape[0]), int(z.shape[1])
    if d < 1:
        raise GbnfError(f"z must be (n, d) with d >= 1, got {tuple(z.shape)}")
    mean = std = None
    if base is not None:
        mean, std = base
        for t, name in ((mean, "base mean"), (std, "base std")):
            _require_device_f32(t, name)
            if tuple(t.shape) != (d,):
                raise GbnfError(f"{name} must be ({d},), got {tuple(t.shape)}")
    if r is not None:
        _require_device_f32(r, "r")
        if tuple(r.shape) != (n,):
            raise GbnfError(f"r must be ({n},), got {tuple(r.shape)}")
    g_z = torch.empty_like(z)
    g_ldj = torch.empty(n, dtype=torch.float32, device=z.device)
    ll = torch.empty(n, dtype=torch.float32, device=z.device) if want_ll else None
    if n:
        _check(lib().gbnf_score_seed(_ptr(z), _ptr(mean), _ptr(std), _ptr(r), n, d, _ptr(g_z), _ptr(g_ldj), _ptr(ll), _stream_ptr()))
    return (g_z, g_ldj, ll) if want_ll else (g_z, g_ldj)


def score_seed(z, prior=None, r=None, base=None, want_ll=False):
    """The autograd seed of a component's log-density scaled per row by ``r`` ((n,) or None for 1), chosen by the rank of z
    (``tabular_score_seed`` is the same tabular call without the dispatch).
    Tabular, z (n, d) device float32 (gbnf_score_seed): ``base`` = (mean (d,), std (d,)) device tensors or None for N(0, I) ->
    (g_z = -r (z - mean) / std^2, g_ldj = r[, ll (n,) = sum_j log N(z_j; mean_j, std_j) with ``want_ll``; the caller adds ldj]).
    Image, z (n, Cz, Hz, Wz) (gbnf_image_score_seed): ``prior`` = (mu | logvar) as (2Cz,) -- one prior for all rows -- or (n, 2Cz) ->
    (g_z like z, g_ldj (n,)): the gradient of r * (log_normal_diag(z, mu, logvar) + ldj)."""
    import torch
    _require_device_f32(z, "z")
    if z.dim() == 2:
        if prior is not None:
            raise GbnfError("a tabular z (n, d) takes base=(mean, std), not an image prior")
        return tabular_score_seed(z, r, base, want_ll)
    if base is not None or want_ll:
        raise GbnfError("base and want_ll belong to the tabular form: z must be (n, d)")
    if prior is None:
        raise GbnfError("an image z (n, Cz, Hz, Wz) needs its prior (mu | logvar)")
    _require_device_f32(prior, "prior")
    if z.dim() != 4:
        raise GbnfError(f"z must be (n, d) or (n, Cz, Hz, Wz), got {tuple(z.shape)}")
    n, cz = int(z.shape[0]), int(z.shape[1])
    if tuple(prior.shape) == (2 * cz,):
        stride = 0
    elif tuple(prior.shape) == (n, 2 * cz):
        stride = 2 * cz
    else:
        raise GbnfError(f"prior must be ({2 * cz},) or ({n}, {2 * cz}), got {tuple(prior.shape)}")
    if r is not None:
        _require_device_f32(r, "r")
        if tuple(r.shape) != (n,):
            raise GbnfError(f"r must be ({n},), got {tuple(r.shape)}")
    g_z = torch.empty_like(z)
    g_ldj = torch.empty(n, dtype=torch.float32, device=z.device)
    if n:
        _check(lib().gbnf_image_score_seed(_ptr(z), _ptr(prior), stride, _ptr(r), n, cz, int(z.shape[2] * z.shape[3]), _ptr(g_z), _ptr(g_ldj),
                                           _stream_ptr()))
    return g_z, g_ldj


def mixture_responsibilities(ll, log_w):
    """gbnf_mixture_responsibilities: ll (C, N) device float32 per-component log-densities (image or tabular), log_w (C,) ->
    (r (C, N) = softmax_c(log_w + ll), G (N,) = logsumexp_c(log_w + ll)); a column of -inf gives G = -inf and r = 0."""
    import torch
    _require_device_f32(ll, "ll")
    _require_device_f32(log_w, "log_w")
    if ll.dim() != 2 or tuple(log_w.shape) != (ll.shape[0],) or ll.shape[0] < 1:
        raise GbnfError(f"ll must be (C, N) with C >= 1 and log_w (C,), got {tuple(ll.shape)} and {tuple(log_w.shape)}")
    c, n = ll.shape
    r = torch.empty_like(ll)
    G = torch.empty(n, dtype=torch.float32, device=ll.device)
    if n:
        _check(lib().gbnf_mixture_responsibilities(C.c_void_p(ll.data_ptr()), C.c_void_p(log_w.data_ptr()), c, n, C.c_void_p(r.data_ptr()),
                                                   C.c_void_p(G.data_ptr()), _stream_ptr()))
    return r, G


def _open_trainers(trainers, cls):
    trainers = list(trainers)
    if not trainers or any(not isinstance(t, cls) or not t.handle for t in trainers):
        raise GbnfError(f"trainers must be a non-empty sequence of open {cls.__name__}s")
    return trainers


def image_mixture_score_workspace_bytes(trainers, n):
    return _query_i64(lib().gbnf_image_mixture_score_workspace_bytes, _handle_array(trainers), len(trainers), int(n))


def image_mixture_score(trainers, log_w, x, noise=None, y=None, want_r=False, workspace=None):
    """gbnf_image_mixture_score: the score of the mixture of ``trainers`` (``NativeImageTrainer``s of components 0 .. C-1 with their
    LU factors / top prior / conditioning bound) with log-weights ``log_w`` (C,) in ONE library call -> (g_x like x, G (n,) =
    log p(x), r (C, n) | None).  ``noise`` is shared by the components and held fixed; ``y`` (n, Y) for conditioned trainers.
    ``workspace``: a contiguous device tensor to use (None: allocated here; its size is checked by the library)."""
    import torch
    trainers = _open_trainers(trainers, NativeImageTrainer)
    _require_device_f32(x, "x")
    if x.dim() != 4 or any(tuple(x.shape[1:]) != t.input_size for t in trainers):
        raise GbnfError(f"x must be (n,{trainers[0].input_size}) for every trainer, got {tuple(x.shape)}")
    n = x.shape[0]
    _check_noise(noise, x)
    _check_log_w(log_w, len(trainers))
    conditioned = [t.y_classes > 0 for t in trainers]
    if any(conditioned) and (not all(conditioned) or y is None):
        raise GbnfError("class-conditional trainers need y (n, Y), and every trainer of the call must be conditioned")
    if y is not None:
        y = trainers[0]._check_y(y, n)
    g_x = torch.empty_like(x)
    G = torch.empty(n, dtype=torch.float32, device=x.device)
    r = torch.empty((len(trainers), n), dtype=torch.float32, device=x.device) if want_r else None
    if n:
        workspace = _workspace_arg(workspace, lambda: image_mixture_score_workspace_bytes(trainers, n), x.device)
        _check(lib().gbnf_image_mixture_score(_handle_array(trainers), len(trainers), _ptr(log_w), _ptr(x), _ptr(noise), _ptr(y), n,
                                              _ptr(g_x), _ptr(G), _ptr(r), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                              _stream_ptr()))
    return g_x, G, r


def mixture_score_workspace_bytes(trainers, n):
    trainers = _open_trainers(trainers, NativeTrainer)
    return _query_i64(lib().gbnf_mixture_score_workspace_bytes, _handle_array(trainers), len(trainers), int(n))


def mixture_score(trainers, log_w, x, ll=None, base=None, want_r=False, workspace=None):
    """gbnf_mixture_score: the score of the mixture of ``trainers`` (``NativeTrainer``s of components 0 .. C-1, on running statistics)
    with log-weights ``log_w`` (C,) in ONE library call -> (g_x like x, G (n,) = log p(x), r (C, n) | None).  ``ll``: the (C, n)
    table of per-component log-densities if the caller has it (``NativeMixture.component_log_prob``: one launch for all components),
    None: one more forward per component.  ``base`` = (mean (d,), std (d,)) device tensors or None for N(0, I).  ``workspace``: a
    contiguous device tensor to use (None: allocated here; its size is checked by the library).  The call runs every trainer's
    forward on the running statistics: a ``forward(want_trace=True)`` made in batch-statistics mode before it must not be followed
    by its ``backward`` after it (the BatchNorm entries that backward reads were re-derived; ``BoostedFlow`` raises in that case)."""
    import torch
    trainers = _open_trainers(trainers, NativeTrainer)
    _require_device_f32(x, "x")
    if x.dim() != 2 or any(x.shape[1] != t.d for t in trainers):
        raise GbnfError(f"x must be (n,{trainers[0].d}) for every trainer, got {tuple(x.shape)}")
    n, nc = x.shape[0], len(trainers)
    _check_log_w(log_w, nc)
    if ll is not None:
        _require_device_f32(ll, "ll")
        if tuple(ll.shape) != (nc, n):
            raise GbnfError(f"ll must be ({nc}, {n}), got {tuple(ll.shape)}")
    mean = std = None
    if base is not None:
        mean, std = base
        for t, name in ((mean, "base mean"), (std, "base std")):
            _require_device_f32(t, name)
            if tuple(t.shape) != (x.shape[1],):
                raise GbnfError(f"{name} must be ({x.shape[1]},), got {tuple(t.shape)}")
    g_x = torch.empty_like(x)
    G = torch.empty(n, dtype=torch.float32, device=x.device)
    r = torch.empty((nc, n), dtype=torch.float32, device=x.device) if want_r else None
    if n:
        workspace = _workspace_arg(workspace, lambda: mixture_score_workspace_bytes(trainers, n), x.device)
        _check(lib().gbnf_mixture_score(_handle_array(trainers), nc, _ptr(log_w), _ptr(mean), _ptr(std), _ptr(ll), _ptr(x), n, _ptr(g_x),
                                        _ptr(G), _ptr(r), _ptr(workspace), workspace.numel() * workspace.element_size(), _stream_ptr()))
    return g_x, G, r


def mixture_step_workspace_bytes(trainers, n):
    trainers = _open_trainers(trainers, NativeTrainer)
    return _query_i64(lib().gbnf_mixture_step_workspace_bytes, _handle_array(trainers), len(trainers), int(n))


def mixture_nll_step(trainers, states, log_w, x, *, lr, weight_decay=0.0, max_grad_norm=0.0, betas=(0.9, 0.999), eps=1e-8, want_G=False,
                     want_r=False, workspace=None):
    """gbnf_mixture_nll_step: ONE joint step of every component on the mixture NLL  -mean_i LSE_c(log_w_c + ll_c(x_i))  in one library
    call: C traced forwards -> responsibilities -> per component the seed (r_c / n) z_c, -r_c / n, its backward and gradient norm ->
    one clip coefficient over all components -> C optimiser updates on the live tensors, no host read in between.  ``trainers``:
    ``NativeTrainer``s of components 0 .. C-1 on running statistics; ``states``: their ``OptState``s (one kind), each advanced by one
    step; ``log_w`` (C,) device, held fixed; ``lr``: a float or a sequence of C floats (0: that component's parameters stay bit for
    bit, its moments move).  -> (stats (4 + 2 C,) device tensor: nll, total gradient norm, clip coefficient, 0, the C mean
    responsibilities, the C component gradient norms; the C flat unclipped gradients; G (n,) | None; r (C, n) | None).
    ``workspace``: a contiguous device tensor to use (None: allocated here; its size is checked by the library).  The parameters
    change behind autograd's back: no version counter moves (``BoostedFlow.mixture_training_step`` takes care of that)."""
    import torch
    trainers = _open_trainers(trainers, NativeTrainer)
    nc = len(trainers)
    states = list(states)
    if len(states) != nc or any(not isinstance(s, OptState) for s in states):
        raise GbnfError(f"states must be {nc} OptStates, one per trainer")
    lrs = [float(lr)] * nc if isinstance(lr, (int, float)) else [float(v) for v in lr]
    if len(lrs) != nc:
        raise GbnfError(f"lr must be a float or {nc} floats, got {len(lrs)}")
    _require_device_f32(x, "x")
    if x.dim() != 2 or x.shape[0] < 1 or any(x.shape[1] != t.d for t in trainers):
        raise GbnfError(f"x must be (n,{trainers[0].d}) with n >= 1 for every trainer, got {tuple(x.shape)}")
    n = x.shape[0]
    _check_log_w(log_w, nc)
    if len({s.kind for s in states}) != 1:
        raise GbnfError("states must be of one optimiser kind")
    hypers = (_OptHyper * nc)()
    for c, (t, s) in enumerate(zip(trainers, states)):
        s.check(t)
        hypers[c] = t._hyper(s, lr=lrs[c], weight_decay=weight_decay, max_grad_norm=max_grad_norm, betas=betas, eps=eps)
    if workspace is None:        # (in line, without _workspace_arg's closure: this is the per-step path)
        workspace = torch.empty((mixture_step_workspace_bytes(trainers, n) + 3) // 4, dtype=torch.float32, device=x.device)
    else:
        _check_workspace(workspace)
    flats = [torch.empty(t.grad_floats, dtype=torch.float32, device=x.device) for t in trainers]
    stats = torch.zeros(4 + 2 * nc, dtype=torch.float32, device=x.device)
    G = torch.empty(n, dtype=torch.float32, device=x.device) if want_G else None
    r = torch.empty((nc, n), dtype=torch.float32, device=x.device) if want_r else None
    _check(lib().gbnf_mixture_nll_step(_handle_array(trainers), nc, _ptr(log_w), _ptr(x), n, _addr_array(flats),
                                       _addr_array([s.exp_avg for s in states]), _addr_array([s.exp_avg_sq for s in states]), hypers,
                                       _ptr(stats), _ptr(G), _ptr(r), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                       _stream_ptr()))
    for s in states:
        s.step += 1
    return stats, flats, G, r


def prepared_mixture_lse(ll, rho, out):
    """Bound form of mixture_lse: returns ``launch(stream_ptr)``."""
    _require_device_f32(ll, "ll")
    _require_device_f32(rho, "rho")
    _require_device_f32(out, "out")
    c, n = ll.shape
    if rho.numel() < c or out.numel() != n:
        raise GbnfError("prepared_mixture_lse: shape mismatch")
    fn = lib().gbnf_mixture_lse
    lp, rp, op = C.c_void_p(ll.data_ptr()), C.c_void_p(rho.data_ptr()), C.c_void_p(out.data_ptr())
    keep = (ll, rho, out)

    def launch(stream_ptr, _keep=keep):
        rc = fn(lp, n, rp, c, n, op, stream_ptr)
        if rc:
            _check(rc)
    return launch


def actnorm_init(z, scale=1.0):
    """ActNorm data-dependent initialisation statistics of a device batch z (n,d) -> (bias (d,), logs (d,))."""
    import torch
    _require_device_f32(z, "z")
    if z.dim() != 2 or z.shape[0] < 1:
        raise GbnfError("z must be (n,d) with n >= 1")
    n, d = z.shape
    bias = torch.empty(d, dtype=torch.float32, device=z.device)
    logs = torch.empty(d, dtype=torch.float32, device=z.device)
    _check(lib().gbnf_actnorm_init(C.c_void_p(z.data_ptr()), n, d, float(scale), C.c_void_p(bias.data_ptr()),
                                   C.c_void_p(logs.data_ptr()), _stream_ptr()))
    return bias, logs


def boosting_weights(G, beta=1.0):
    """Boosting sample weights from the fixed components' mixture log-density G (n,) on the device."""
    import torch
    _require_device_f32(G, "G")
    if G.dim() != 1 or G.numel() < 1:
        raise GbnfError("G must be (n,) with n >= 1")
    w = torch.empty_like(G)
    _check(lib().gbnf_boosting_weights(C.c_void_p(G.data_ptr()), G.numel(), float(beta), C.c_void_p(w.data_ptr()),
                                       _stream_ptr()))
    return w


def resample_rows(w, u):
    """Multinomial resampling with replacement by inverse CDF (gbnf_resample_rows): ``w`` (n,) weights and ``u`` (m,) uniforms in [0,1),
    both float32 on the device -> rows (m,) int64, rows[i] = the smallest j with u[i] * sum(w) < cumsum(max(w, 0))[j] in float64."""
    import torch
    _require_device_f32(w, "w")
    _require_device_f32(u, "u")
    if w.dim() != 1 or w.numel() < 1 or u.dim() != 1 or u.numel() < 1:
        raise GbnfError("w must be (n,) and u (m,) with n, m >= 1")
    nb = _query_i64(lib().gbnf_resample_workspace_bytes, w.numel())
    cdf = torch.empty(nb // 8, dtype=torch.float64, device=w.device)
    rows = torch.empty(u.numel(), dtype=torch.int64, device=w.device)
    _check(lib().gbnf_resample_rows(_ptr(w), w.numel(), _ptr(u), u.numel(), _ptr(rows), _ptr(cdf), nb, _stream_ptr()))
    return rows


_sample_ws = {}        # device -> workspace of mixture_partition / mixture_sample (grown to the largest call so far)


def _sample_workspace(n_flows, n, d, device):
    import torch
    nb = _query_i64(lib().gbnf_mixture_sample_workspace_bytes, int(n_flows), int(n), int(d))
    ws = _sample_ws.get(str(device))
    if ws is None or ws.numel() * 4 < nb:
        ws = _sample_ws[str(device)] = torch.empty(nb // 4, dtype=torch.float32, device=device)
    return ws, nb


def mixture_partition(rho, u, n_used=None, z=None):
    """The first phase of drawing from the mixture (gbnf_mixture_sample_begin): a component per row from ``rho[0:n_used]`` and the uniforms
    ``u`` (n,) by the rule of ``resample_rows``, the rows partitioned by component -> (comp (n,) int32, order (n,) int64, counts (n_used,)
    int64, workspace), all on the device and nothing read back.  ``order`` lists the rows of component 0 in ascending index, then those
    of component 1, ...; with ``z`` (n,d) the workspace holds its rows in that order, segment by segment, for ``mixture_sample``."""
    import torch
    _require_device_f32(rho, "rho")
    _require_device_f32(u, "u")
    n_used = rho.numel() if n_used is None else int(n_used)
    if rho.dim() != 1 or not 1 <= n_used <= rho.numel():
        raise GbnfError(f"rho must be (C,) with 1 <= n_used <= C, got {tuple(rho.shape)} and n_used = {n_used}")
    if u.dim() != 1 or u.numel() < 1:
        raise GbnfError("u must be (n,) with n >= 1")
    n, d = u.numel(), 1
    if z is not None:
        _require_device_f32(z, "z")
        if z.dim() != 2 or z.shape[0] != n or z.shape[1] < 1:
            raise GbnfError(f"z must be ({n},d), got {tuple(z.shape)}")
        d = z.shape[1]
    ws, nb = _sample_workspace(n_used, n, d, u.device)
    comp = torch.empty(n, dtype=torch.int32, device=u.device)
    order = torch.empty(n, dtype=torch.int64, device=u.device)
    counts = torch.empty(n_used, dtype=torch.int64, device=u.device)
    _check(lib().gbnf_mixture_sample_begin(C.c_void_p(rho.data_ptr()), n_used, C.c_void_p(u.data_ptr()),
                                           C.c_void_p(z.data_ptr() if z is not None else 0), n, d, C.c_void_p(comp.data_ptr()),
                                           C.c_void_p(order.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()), nb,
                                           _stream_ptr()))
    return comp, order, counts, ws


def mixture_sample(flows, rho, u, z, n_used=None, want_ldj=True, out=None):
    """Rows of the boosted MIXTURE from latent rows: row i goes backwards through the component drawn for it from ``rho[0:n_used]`` by
    ``u[i]`` (the rule of ``resample_rows``) -> (x (n,d), log|det dx/dz| (n,) | None, comp (n,) int32).  ``flows``: the components'
    ``NativeFlow`` handles, at least n_used of them; ``rho`` (C,), ``u`` (n,), ``z`` (n,d): float32 on the device.  ``out``: the x buffer
    (it may be ``z`` itself).  gbnf_mixture_sample_begin, ONE host read of the n_used segment sizes (where the reference has the
    ``.item()`` of its draw), gbnf_mixture_sample_finish: every component's rows are one ``gbnf_flow_inverse`` call."""
    import torch
    n_used = len(flows) if n_used is None else int(n_used)
    if not 1 <= n_used <= len(flows):
        raise GbnfError(f"n_used = {n_used} outside [1, {len(flows)}]")
    if z is None:
        raise GbnfError("z must be (n,d)")
    comp, order, counts, ws = mixture_partition(rho, u, n_used, z)
    n, d = z.shape
    if any(f.d != d for f in flows[:n_used]):
        raise GbnfError(f"every flow must have d = {d}")
    x = torch.empty_like(z) if out is None else _require_device_f32(out, "out")
    if tuple(x.shape) != (n, d):
        raise GbnfError(f"out must be ({n},{d}), got {tuple(x.shape)}")
    ldj = torch.empty(n, dtype=torch.float32, device=z.device) if want_ldj else None
    handles = _handle_array(flows[:n_used])
    host = (C.c_int64 * n_used)(*counts.cpu().tolist())
    _check(lib().gbnf_mixture_sample_finish(handles, n_used, host, C.c_void_p(order.data_ptr()), n, C.c_void_p(x.data_ptr()),
                                            C.c_void_p(ldj.data_ptr() if ldj is not None else 0), C.c_void_p(ws.data_ptr()),
                                            ws.numel() * 4, _stream_ptr()))
    return x, ldj, comp
