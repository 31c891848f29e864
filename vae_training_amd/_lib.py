"""ctypes binding of include/vaek.h (the drop-in boundary).  Loads the in-tree libvaek.so."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VAEK_LIB_PATH") or os.path.join(_HERE, "csrc", "libvaek.so")      # override: A/B builds, diagnostics
VAEK_MAX_HIDDEN = 8
VAEK_F32, VAEK_BF16 = 0, 1
VAEK_ACT_NONE, VAEK_ACT_RELU = 0, 1


class VaekError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libvaek error {code}: {msg}")
        self.code = code


class VaekConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("batch", C.c_int32), ("data_dim", C.c_int32), ("latent_dim", C.c_int32),
        ("n_enc_hidden", C.c_int32), ("enc_hidden", C.c_int32 * VAEK_MAX_HIDDEN),
        ("n_dec_hidden", C.c_int32), ("dec_hidden", C.c_int32 * VAEK_MAX_HIDDEN),
        ("sigmoid_decoder", C.c_int32), ("tunable_eps", C.c_int32), ("eps_cli", C.c_float),
        ("dtype", C.c_int32), ("device", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32),
        ("global_batch", C.c_int64), ("force_generic", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class VaekReplicas(C.Structure):
    """vaek_replicas of include/vaek.h: the per-replica description of vaek_train_loop_gen_replicas and
    vaek_train_step_gen_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("state_stride", C.c_int64), ("grads_stride", C.c_int64),
        ("seeds", C.c_void_p), ("lrs", C.c_void_p), ("a_stride", C.c_int64), ("loss_hist", C.c_void_p), ("loss_hist_cap", C.c_int64),
    ]


class VaekTrajectory(C.Structure):
    """vaek_trajectory of include/vaek.h: the trajectory ring of vaek_train_loop_gen_traj and vaek_train_loop_gen_replicas_traj
    (`buf` is a device pointer; strides and cap count floats and records)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("every", C.c_int32), ("buf", C.c_void_p), ("cap", C.c_int64), ("record_stride", C.c_int64),
        ("replica_stride", C.c_int64),
    ]


class VaekStatsEvent(C.Structure):
    """vaek_stats_event of include/vaek.h: the per-replica description of vaek_stats_event_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32), ("state_stride", C.c_int64),
        ("x_seeds", C.c_void_p), ("x_steps", C.c_void_p), ("z_seeds", C.c_void_p), ("z_steps", C.c_void_p), ("sample_eps", C.c_void_p),
        ("a_stride", C.c_int64), ("out", C.c_void_p), ("out_stride", C.c_int64),
    ]


class VaekLogLikelihood(C.Structure):
    """vaek_log_likelihood of include/vaek.h: the per-replica description of vaek_log_likelihood_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("rows", C.c_int32), ("samples", C.c_int32), ("state_stride", C.c_int64),
        ("x_seeds", C.c_void_p), ("x_steps", C.c_void_p), ("z_seeds", C.c_void_p), ("z_steps", C.c_void_p), ("a_stride", C.c_int64),
        ("out", C.c_void_p), ("out_stride", C.c_int64), ("x", C.c_void_p), ("x_stride", C.c_int64),
    ]


class VaekSpectrumEvent(C.Structure):
    """vaek_spectrum_event of include/vaek.h: vaek_stats_event's fields with a double* out (device pointers)."""
    _fields_ = list(VaekStatsEvent._fields_)


class VaekExactLogLikelihood(C.Structure):
    """vaek_exact_log_likelihood of include/vaek.h: the per-replica description of vaek_exact_log_likelihood_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32), ("state_stride", C.c_int64),
        ("x_seeds", C.c_void_p), ("x_steps", C.c_void_p), ("a_stride", C.c_int64), ("out", C.c_void_p), ("out_stride", C.c_int64),
        ("x", C.c_void_p), ("x_stride", C.c_int64), ("row_out", C.c_void_p), ("row_stride", C.c_int64),
    ]


class VaekDecoderJacobian(C.Structure):
    """vaek_decoder_jacobian of include/vaek.h: the per-replica description of vaek_mlp3_decoder_jacobian_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32), ("state_stride", C.c_int64),
        ("z_seeds", C.c_void_p), ("z_steps", C.c_void_p), ("z", C.c_void_p), ("z_stride", C.c_int64), ("rank_tol", C.c_double),
        ("out", C.c_void_p), ("out_stride", C.c_int64), ("row_out", C.c_void_p), ("row_out_stride", C.c_int64),
    ]


class VaekElboHvp(C.Structure):
    """vaek_elbo_hvp of include/vaek.h: the per-replica description of vaek_elbo_hvp_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("rows", C.c_int32), ("nvec", C.c_int32), ("state_stride", C.c_int64),
        ("x_seeds", C.c_void_p), ("x_steps", C.c_void_p), ("a_stride", C.c_int64), ("x", C.c_void_p), ("x_stride", C.c_int64),
        ("v", C.c_void_p), ("v_stride", C.c_int64), ("hv", C.c_void_p), ("hv_stride", C.c_int64), ("grad", C.c_void_p),
        ("grad_stride", C.c_int64), ("out", C.c_void_p), ("out_stride", C.c_int64),
    ]


class VaekElboHessian(C.Structure):
    """vaek_elbo_hessian of include/vaek.h: the per-replica description of vaek_elbo_hessian_lanczos_replicas (device pointers)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n", C.c_int32), ("rows", C.c_int32), ("steps", C.c_int32), ("state_stride", C.c_int64),
        ("x_seeds", C.c_void_p), ("x_steps", C.c_void_p), ("a_stride", C.c_int64), ("x", C.c_void_p), ("x_stride", C.c_int64),
        ("v0", C.c_void_p), ("v0_stride", C.c_int64), ("basis", C.c_void_p), ("basis_stride", C.c_int64), ("out", C.c_void_p),
        ("out_stride", C.c_int64),
    ]


class VaekSampledElboHvp(C.Structure):
    """vaek_sampled_elbo_hvp of include/vaek.h: vaek_elbo_hvp's fields, then the samples and their source (device pointers)."""
    _fields_ = list(VaekElboHvp._fields_) + [
        ("samples", C.c_int32), ("reserved", C.c_int32), ("z_seeds", C.c_void_p), ("z_steps", C.c_void_p), ("xi", C.c_void_p),
        ("xi_stride", C.c_int64),
    ]


class VaekSampledElboHessian(C.Structure):
    """vaek_sampled_elbo_hessian of include/vaek.h: vaek_elbo_hessian's fields, then the samples and their source (device pointers)."""
    _fields_ = list(VaekElboHessian._fields_) + [
        ("samples", C.c_int32), ("reserved", C.c_int32), ("z_seeds", C.c_void_p), ("z_steps", C.c_void_p), ("xi", C.c_void_p),
        ("xi_stride", C.c_int64),
    ]


ELBO_HESSIAN_RECORD_HEAD = 12      # doubles of a Lanczos record in front of the four blocks of 32: theta, rho, alpha, beta
ELBO_HESSIAN_MAX_STEPS = 32
DECODER_JACOBIAN_RECORD_HEAD = 8   # doubles of a decoder-Jacobian model record in front of the L mean eigenvalues and the L mean diagonals
EXACT_LOGLIK_RECORD_HEAD = 10      # doubles of an exact log-likelihood record in front of the D eigenvalues of K^T K
STATS_RECORD_HEAD = 8     # floats of a stats record in front of the epsilon_p copy: loss, Dkl, mse, eps, two score values, 0, 0


def trajectory_slot(t, every, cap):
    """The slot rule of vaek_trajectory: the ring slot of the record of Adam step t (1-based), or None where step t is not recorded."""
    if t < 1 or t % every:
        return None
    return (t // every - 1) % cap


_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); exactly the symbols include/vaek.h declares
SIGNATURES = {
    "vaek_version": (C.c_int, []),
    "vaek_last_error": (C.c_char_p, []),
    "vaek_ctx_create": (C.c_int, [C.POINTER(VaekConfig), C.POINTER(_vp)]),
    "vaek_ctx_destroy": (C.c_int, [_vp]),
    "vaek_param_count": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_grad_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_leaf_count": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_leaf_info": (C.c_int, [_vp, _i32, C.c_char_p, _i32, C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32)]),
    "vaek_workspace_bytes": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "vaek_uses_fused_path": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_train_step_path": (C.c_int, [_vp, C.c_char_p, _i32]),
    "vaek_dense_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "vaek_dense_bwd_dx": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vaek_dense_bwd_dw": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "vaek_elbo_fwd_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp]),
    "vaek_elbo_fwd_bwd_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp]),
    "vaek_adam_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _i32, _vp, _f32, _vp]),
    "vaek_train_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp]),
    "vaek_train_step_grads_only": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vaek_train_step_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp]),
    "vaek_bucket_count": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_bucket_info": (C.c_int, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "vaek_train_step_grads_bucketed": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vaek_loss_eval": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vaek_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp, _vp, _i32, _vp, _vp]),
    "vaek_comm_buffer_bytes": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "vaek_comm_create": (C.c_int, [_vp, _vp]),
    "vaek_comm_init": (C.c_int, [_vp, _vp]),
    "vaek_comm_status": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_comm_destroy": (C.c_int, [_vp]),
    "vaek_comm_allreduce": (C.c_int, [_vp, _vp, _i64, _vp]),
    "vaek_make_batch": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _i32, _i64, C.c_uint64, _vp,
                                  C.c_uint32, C.c_uint32, _vp]),
    "vaek_make_batch_next": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _i32, _i64, C.c_uint64, _vp,
                                       _i32, C.c_uint32, _vp]),
    "vaek_train_step_gen": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _vp, _i32, _i32, _i32, _f32,
                                      _vp, _vp, _vp, _i64, C.c_uint64, _vp, _i32, C.c_uint32, _vp]),
    "vaek_supports_train_steps": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_train_steps": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp, _vp]),
    "vaek_train_steps_status": (C.c_int, [_vp, _vp, C.POINTER(_i32)]),
    "vaek_supports_train_steps_gen": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_train_steps_moment_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_train_steps_moments": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vaek_train_steps_update": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp]),
    "vaek_train_steps_gen": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _f32, C.c_int64, C.c_uint64, C.c_uint32, _i32,
                                       _f32, _vp, _vp]),
    "vaek_supports_train_loop_gen": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_train_loop_gen": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _f32, C.c_int64, C.c_uint64, C.c_uint32, _i32,
                                      _f32, _vp, _vp]),
    "vaek_train_loop_steps_per_launch": (C.c_int, []),
    "vaek_train_loop_max_replicas": (C.c_int, []),
    "vaek_train_loop_replicas_workspace_bytes": (C.c_int, [_vp, _i32, C.POINTER(C.c_size_t)]),
    "vaek_train_loop_gen_replicas": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(VaekReplicas), _i32, _vp, _i32, _i32, _i32, _f32,
                                               C.c_int64, C.c_uint32, _i32, _f32, _vp, _vp]),
    "vaek_trajectory_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_train_loop_gen_traj": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _f32, C.c_int64, C.c_uint64, C.c_uint32, _i32,
                                           _f32, _vp, _vp, C.POINTER(VaekTrajectory)]),
    "vaek_train_loop_gen_replicas_traj": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(VaekReplicas), _i32, _vp, _i32, _i32, _i32, _f32,
                                                    C.c_int64, C.c_uint32, _i32, _f32, _vp, _vp, C.POINTER(VaekTrajectory)]),
    "vaek_supports_stats_event": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_stats_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_stats_event_max_rows": (C.c_int, []),
    "vaek_stats_event_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekStatsEvent), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32, C.c_uint32, _vp]),
    "vaek_supports_log_likelihood": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_log_likelihood_record_len": (C.c_int, []),
    "vaek_log_likelihood_max_rows": (C.c_int, []),
    "vaek_log_likelihood_max_samples": (C.c_int, []),
    "vaek_log_likelihood_workspace_bytes": (C.c_int, [_vp, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_log_likelihood_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekLogLikelihood), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32, C.c_uint32,
                                               _vp, _vp]),
    "vaek_supports_mlp3_log_likelihood": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_mlp3_log_likelihood_max_columns": (C.c_int, []),
    "vaek_mlp3_log_likelihood_workspace_bytes": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_mlp3_log_likelihood_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekLogLikelihood), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32,
                                                    C.c_uint32, _vp, _vp]),
    "vaek_supports_mlp3_stats_event": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_mlp3_stats_event_workspace_bytes": (C.c_int, [_vp, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_mlp3_stats_event_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekStatsEvent), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32, C.c_uint32,
                                                 _vp, _vp]),
    "vaek_supports_cov_spectrum": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_cov_spectrum_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_cov_spectrum_max_sets": (C.c_int, []),
    "vaek_cov_spectrum_max_sweeps": (C.c_int, []),
    "vaek_cov_spectrum_rows": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _vp, _i64, _vp]),
    "vaek_supports_spectrum_event": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_spectrum_event_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekSpectrumEvent), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32, C.c_uint32,
                                               _vp]),
    "vaek_cov_eigen_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_cov_eigen_rows": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _vp, _i64, _vp]),
    "vaek_eigen_event_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekSpectrumEvent), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32, C.c_uint32,
                                            _vp]),
    "vaek_subspace_record_len": (C.c_int, [_i32]),
    "vaek_subspace_angles": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "vaek_supports_exact_log_likelihood": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_exact_log_likelihood_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_exact_log_likelihood_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekExactLogLikelihood), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32,
                                                     _vp]),
    "vaek_supports_elbo_hessian": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_elbo_hvp_max_vectors": (C.c_int, []),
    "vaek_elbo_hvp_record_len": (C.c_int, []),
    "vaek_elbo_hessian_max_steps": (C.c_int, []),
    "vaek_elbo_hessian_record_len": (C.c_int, []),
    "vaek_elbo_hessian_basis_doubles": (C.c_int, [_vp, _i32, C.POINTER(_i64)]),
    "vaek_elbo_hvp_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekElboHvp), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32, _vp]),
    "vaek_elbo_hessian_lanczos_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekElboHessian), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32,
                                                     _vp]),
    "vaek_supports_sampled_elbo_hessian": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_sampled_elbo_hessian_max_columns": (C.c_int, []),
    "vaek_sampled_elbo_hessian_record_len": (C.c_int, []),
    "vaek_sampled_elbo_hessian_workspace_bytes": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_sampled_elbo_hvp_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekSampledElboHvp), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32,
                                                 C.c_uint32, _vp, _vp]),
    "vaek_sampled_elbo_hessian_lanczos_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekSampledElboHessian), _i32, _vp, _i32, _i32, _i32, _f32,
                                                             C.c_uint32, C.c_uint32, _vp, _vp]),
    "vaek_supports_mlp3_sampled_elbo_hessian": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "vaek_mlp3_sampled_elbo_hessian_max_columns": (C.c_int, []),
    "vaek_mlp3_sampled_elbo_hessian_workspace_bytes": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_mlp3_sampled_elbo_hvp_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekSampledElboHvp), _i32, _vp, _i32, _i32, _i32, _f32, C.c_uint32,
                                                      C.c_uint32, _vp, _vp]),
    "vaek_mlp3_sampled_elbo_hessian_lanczos_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekSampledElboHessian), _i32, _vp, _i32, _i32, _i32,
                                                                  _f32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "vaek_supports_mlp3_decoder_jacobian": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_decoder_jacobian_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_decoder_jacobian_row_record_len": (C.c_int, [_vp, C.POINTER(_i64)]),
    "vaek_mlp3_decoder_jacobian_max_columns": (C.c_int, []),
    "vaek_mlp3_decoder_jacobian_workspace_bytes": (C.c_int, [_vp, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_mlp3_decoder_jacobian_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekDecoderJacobian), C.c_uint32, _vp, _vp]),
    "vaek_supports_linear_decoder_jacobian": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_linear_decoder_jacobian_max_rows": (C.c_int, []),
    "vaek_linear_decoder_jacobian_workspace_bytes": (C.c_int, [_vp, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_linear_decoder_jacobian_replicas": (C.c_int, [_vp, _vp, C.POINTER(VaekDecoderJacobian), C.c_uint32, _vp, _vp]),
    "vaek_supports_train_step_replicas": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vaek_train_step_max_replicas": (C.c_int, []),
    "vaek_train_step_replicas_workspace_bytes": (C.c_int, [_vp, _i32, C.POINTER(C.c_size_t)]),
    "vaek_train_step_gen_replicas": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(VaekReplicas), _vp, _vp, _vp, _f32, _vp, _i32, _vp,
                                               _i32, _i32, _i32, _f32, _vp, _vp, _vp, _i64, _vp, _i32, C.c_uint32, _vp]),
    "vaek_conv2d_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vaek_to_bf16": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "vaek_conv2d_forward_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_conv2d_bias_grad": (C.c_int, [_vp, _vp, _vp, C.c_int64, _i32, _vp]),
    "vaek_conv2d_bias_grad_bf16": (C.c_int, [_vp, _vp, _vp, C.c_int64, _i32, _vp]),
    "vaek_dense_fwd_reparam": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "vaek_reparam_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.c_int64, _vp, _vp]),
    "vaek_conv2d_transpose_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vaek_conv2d_weight_grad_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "vaek_conv2d_weight_grad": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vaek_rng_fill": (C.c_int, [_vp, _vp, _vp, _i64, C.c_uint64, C.c_uint32, C.c_uint32, _vp]),
    "vaek_set_loss_history": (C.c_int, [_vp, _vp, _i64]),
    "vaek_microbench_copy": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "vaek_microbench_launch": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vaek_microbench_mfma": (C.c_int, [_vp, _i32, _i32, _i32, _vp, C.POINTER(C.c_double), _vp]),
    "vaek_profile_begin": (C.c_int, [_vp, _i32]),
    "vaek_profile_report": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
}

_lib = None


def load():
    """Load libvaek.so (once).  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. vae_training_amd has no CPU/PyTorch fallback.")
    # torch first: libvaek shares device pointers and streams with PyTorch-ROCm, so both must use
    # the one HIP runtime torch ships (same SONAME libamdhip64.so.7 -- whoever loads first wins)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise VaekError(rc, load().vaek_last_error().decode("utf-8", "replace"))
