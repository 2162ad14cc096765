"""ctypes binding of libdronenav.so (include/dronenav.h).  No torch types cross this boundary.

There is no CPU fallback: if the library is missing the import of the product fails loudly
(`DroneNavLibraryError`) and tells the user how to build it.
"""
import ctypes as C
import os

from . import build as _build

MAX_WAYPOINTS = 64
MAX_TRACKS = 64
OBS_DIM = 13
ACT_DIM = 4
ABI_VERSION = 10
GROUND_CONTACT_AUTO = 2

DN_OK = 0
STATUS_NAMES = {0: "DN_OK", -1: "DN_ERR_INVALID_ARGUMENT", -2: "DN_ERR_HIP", -3: "DN_ERR_OUT_OF_MEMORY",
                -4: "DN_ERR_NO_DEVICE", -5: "DN_ERR_BAD_STATE"}


class DroneNavError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class DroneNavLibraryError(ImportError):
    pass


class DnConfig(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int64), ("device_id", C.c_int32), ("num_waypoints", C.c_int32),
        ("waypoints", C.c_double * (MAX_WAYPOINTS * 3)), ("spawn", C.c_double * 3), ("aviary_dim", C.c_double * 6),
        ("threshold", C.c_double), ("max_steps", C.c_int32), ("circle", C.c_int32), ("cylinder", C.c_int32),
        ("include_distance", C.c_int32), ("normalize_actions", C.c_int32), ("normalize_obs", C.c_int32),
        ("ground_contact", C.c_int32), ("compute_f32", C.c_int32), ("act_noise_sigma", C.c_float),
        ("obs_noise_sigma", C.c_float), ("seed", C.c_uint64), ("env_id_offset", C.c_int64),
        ("clip_rew", C.c_int32), ("norm_rew", C.c_int32), ("physics", C.c_int32), ("action_type", C.c_int32),
        ("random_spawn", C.c_int32), ("zero_damping", C.c_int32),
    ]


class DnEnvState(C.Structure):
    _fields_ = [
        ("pos", C.c_float * 3), ("quat", C.c_float * 4), ("vel", C.c_float * 3), ("ang_v", C.c_float * 3),
        ("prev_vel", C.c_float * 3), ("prev_ang_v", C.c_float * 3), ("cur_pos", C.c_float * 3),
        ("d", C.c_float), ("d_prev", C.c_float), ("idx", C.c_int32), ("steps", C.c_int32), ("just_found", C.c_int32),
        ("ep_ret", C.c_float), ("ep_len", C.c_int32),
        ("rms_mean", C.c_double * OBS_DIM), ("rms_var", C.c_double * OBS_DIM), ("rms_count", C.c_double),
        ("rr_returns", C.c_double), ("rr_mean", C.c_double), ("rr_var", C.c_double), ("rr_count", C.c_double),
        ("last_rpm", C.c_float * 4), ("pid", C.c_double * 9), ("ep_ret_lo", C.c_float), ("rms_m2", C.c_double * OBS_DIM),
    ]


class DnMlpNet(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("w2", C.c_void_p), ("w3", C.c_void_p), ("wh", C.c_void_p),
                ("b1", C.c_void_p), ("b2", C.c_void_p), ("b3", C.c_void_p), ("bh", C.c_void_p),
                ("out", C.c_void_p), ("out_dim", C.c_int32), ("grade", C.c_int32), ("arch", C.c_int32),
                ("reserved_", C.c_int32)]


class DnStats(C.Structure):
    _fields_ = [("env_steps", C.c_int64), ("episodes", C.c_int64), ("truncated", C.c_int64), ("completed", C.c_int64),
                ("sum_ep_len", C.c_int64), ("sum_found_targets", C.c_int64), ("sum_ep_return", C.c_double)]


class DnDynamicsConfig(C.Structure):
    _fields_ = [("mass", C.c_float * 2), ("inertia", C.c_float * 2), ("kf", C.c_float * 2), ("km", C.c_float * 2),
                ("resample", C.c_int32), ("reserved", C.c_int32)]


class DnWindConfig(C.Structure):
    _fields_ = [("speed", C.c_float * 2), ("azimuth", C.c_float * 2), ("vertical", C.c_float * 2), ("gust_sigma", C.c_float * 2),
                ("gust_tau", C.c_float), ("coeff", C.c_float * 2), ("resample", C.c_int32), ("reserved", C.c_int32)]


class DnActuatorConfig(C.Structure):
    _fields_ = [("latency", C.c_int32 * 2), ("motor_tau", C.c_float * 2), ("fill", C.c_float * 4), ("resample", C.c_int32),
                ("reserved", C.c_int32)]


class DnSensorConfig(C.Structure):
    _fields_ = [("latency", C.c_int32 * 2), ("bias_amp", C.c_float * 13), ("resample", C.c_int32), ("reserved", C.c_int32)]


class DnPrivilegedConfig(C.Structure):
    _fields_ = [("groups", C.c_int32), ("reserved", C.c_int32)]


class DnGoalConfig(C.Structure):
    _fields_ = [("frame", C.c_int32), ("reserved", C.c_int32)]


class DnHistoryConfig(C.Structure):
    _fields_ = [("frames", C.c_int32), ("actions", C.c_int32), ("extra_dim", C.c_int32), ("reserved", C.c_int32)]


class DnRownormConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("clip", C.c_float), ("epsilon", C.c_double)]


class DnRetnormConfig(C.Structure):
    _fields_ = [("gamma", C.c_double), ("epsilon", C.c_double), ("clip", C.c_float), ("reserved", C.c_int32)]


class DnMinibatchField(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_int32), ("normalize", C.c_int32)]


class DnMinibatchConfig(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("epoch", C.c_uint64), ("epsilon", C.c_double), ("num_fields", C.c_int32), ("reserved", C.c_int32)]


MINIBATCH_MAX_FIELDS = 8


class DnPpoLossConfig(C.Structure):
    _fields_ = [("clip_range", C.c_double), ("clip_range_vf", C.c_double), ("ent_coef", C.c_double), ("vf_coef", C.c_double),
                ("act_dim", C.c_int32), ("reserved", C.c_int32)]


PPO_MAX_ACT = 8


class DnAdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("count", C.c_int64)]


class DnAdamConfig(C.Structure):
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double),
                ("n_tensors", C.c_int32), ("flags", C.c_int32)]


ADAM_MAX_TENSORS = 32
ADAM_ZERO_GRADS = 1


class DnReplayConfig(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("draw", C.c_uint64), ("buffer_size", C.c_int64), ("n_envs", C.c_int64), ("valid", C.c_int64),
                ("skip", C.c_int64), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32)]


class DnReplaySource(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("next_obs", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
                ("timeouts", C.c_void_p)]


REPLAY_PLAIN, REPLAY_RING = 0, 1
REPLAY_MAX_OBS, REPLAY_MAX_ACT = 64, 8


class DnSacConfig(C.Structure):
    _fields_ = [("gamma", C.c_double), ("target_entropy", C.c_double), ("ent_coef", C.c_double), ("log_std_min", C.c_double),
                ("log_std_max", C.c_double), ("act_dim", C.c_int32), ("n_critics", C.c_int32), ("reserved", C.c_int64)]


SAC_MAX_ACT, SAC_MAX_CRITICS = 8, 4


class DnMlpTrainLayer(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("d_weight", C.c_void_p), ("d_bias", C.c_void_p), ("in_dim", C.c_int32),
                ("out_dim", C.c_int32)]


class DnMlpTrainConfig(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("activation", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


# DN_MLP_TRAIN_MAX_LAYERS, DN_MLP_ACT_TANH, DN_MLP_TRAIN_ACCUMULATE, DN_MLP_TRAIN_NO_PARAM_GRADS, DN_MLP_TRAIN_CHUNK (tests/test_mlp_train_cpu.py
# holds them to the header)
TRAIN_MAX_LAYERS, TRAIN_ACT_TANH = 4, 0
TRAIN_ACCUMULATE, TRAIN_NO_PARAM_GRADS = 1, 2
TRAIN_CHUNK = 1024


class DnSacTrainConfig(C.Structure):
    _fields_ = [("n_nets", C.c_int32), ("n_layers", C.c_int32), ("head_parts", C.c_int32), ("activation", C.c_int32), ("in0", C.c_int32),
                ("in1", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


# DN_MLP_ACT_RELU, DN_SAC_TRAIN_MAX_NETS, DN_SAC_TRAIN_MAX_PARTS (tests/test_sac_train_cpu.py holds them to the header)
TRAIN_ACT_RELU = 1
TRAIN_MAX_NETS, TRAIN_MAX_PARTS = 4, 2


class DnLstmConfig(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("hidden", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class DnLstmParams(C.Structure):
    _fields_ = [("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p), ("d_w_ih", C.c_void_p),
                ("d_w_hh", C.c_void_p), ("d_b_ih", C.c_void_p), ("d_b_hh", C.c_void_p)]


# the bounds of dn_lstm_* as the header's comment states them (tests/test_lstm_cpu.py holds them to the refusals)
RNN_MAX_IN, RNN_MAX_HIDDEN, RNN_MAX_STEPS, RNN_MAX_ROWS = 64, 512, 1024, 1 << 24


class DnTrackBankConfig(C.Structure):
    _fields_ = [("num_tracks", C.c_int32), ("num_waypoints", C.c_int32 * MAX_TRACKS), ("waypoints", C.c_double * (MAX_WAYPOINTS * 3)),
                ("weight", C.c_float * MAX_TRACKS), ("resample", C.c_int32), ("reserved", C.c_int32)]


# every entry point declared in include/dronenav.h: name -> (restype, argtypes)
_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
PROTOTYPES = {
    "dn_abi_version": (_I32, []),
    "dn_last_error": (C.c_char_p, []),
    "dn_device_count": (_I32, []),
    "dn_config_default": (None, [C.POINTER(DnConfig)]),
    "dn_create": (_I32, [C.POINTER(DnConfig), C.POINTER(_VP)]),
    "dn_destroy": (_I32, [_VP]),
    "dn_num_envs": (_I64, [_VP]),
    "dn_get_config": (_I32, [_VP, C.POINTER(DnConfig)]),
    "dn_get_num_cus": (_I32, [_VP]),
    "dn_get_exact_flags": (_I32, [_VP]),
    "dn_resolve_ground_contact": (_I32, [C.POINTER(DnConfig)]),
    "dn_reset": (_I32, [_VP, _VP, _VP]),
    "dn_step": (_I32, [_VP] * 12),
    "dn_step_many": (_I32, [_VP, _I64] + [_VP] * 11),
    "dn_eval_kinematics": (_I32, [_VP] * 11),
    "dn_compact_done": (_I32, [_VP, _I64, _VP, _VP, _I32, _VP]),
    "dn_pack_done": (_I32, [_VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP]),
    "dn_stream_copy": (_I32, [_VP, _VP, _I64, _I32, _VP]),
    "dn_get_state": (_I32, [_VP, _VP, _I64]),
    "dn_set_state": (_I32, [_VP, _VP, _I64]),
    "dn_get_stats": (_I32, [_VP, C.POINTER(DnStats), _VP]),
    "dn_reset_stats": (_I32, [_VP, _VP]),
    "dn_get_kernel_waves": (_I32, [_VP, _I32]),
    "dn_get_step_count": (_I32, [_VP, C.POINTER(C.c_uint64)]),
    "dn_set_step_count": (_I32, [_VP, C.c_uint64]),
    "dn_preprocess_action": (_I32, [_VP, _I64, _I32, _VP, _VP, _VP, _I32, _VP]),
    "dn_policy_sample": (_I32, [_VP, _VP, C.POINTER(C.c_float), C.c_uint64, _I32, _VP, _VP, _VP, _VP]),
    "dn_squashed_sample": (_I32, [_VP, _VP, C.c_uint64, _I32, _VP, _VP, _VP]),
    "dn_step_squashed": (_I32, [_VP, _VP, C.c_uint64, _I32] + [_VP] * 12),
    "dn_add_bootstrap": (_I32, [_VP, _VP, _VP, C.c_double, _I64, _I32, _VP]),
    "dn_step_sampled": (_I32, [_VP, _VP, C.POINTER(C.c_float), C.c_uint64, _I32] + [_VP] * 12),
    "dn_mlp_forward": (_I32, [_VP, _I32, _VP, _VP, _I64, _I32, _I32, _VP]),
    "dn_mlp_step_sampled": (_I32, [_VP, _VP, _I32, _VP, _I32, C.POINTER(C.c_float), C.c_uint64, _I32] + [_VP] * 12),
    "dn_gae": (_I32, [_VP] * 5 + [_I64, _I64, C.c_double, C.c_double, _VP, _VP, _I32, _VP]),
    "dn_history_width": (_I32, [C.POINTER(DnHistoryConfig)]),
    "dn_stack_history": (_I32, [C.POINTER(DnHistoryConfig), _I64, _I64] + [_VP] * 9 + [_I32, _VP]),
    "dn_rownorm_state_doubles": (_I64, [_I32]),
    "dn_rownorm_scratch_bytes": (_I64, [_I64, _I64, _I32]),
    "dn_rownorm_init": (_I32, [C.POINTER(DnRownormConfig), _VP, _I32, _VP]),
    "dn_rownorm": (_I32, [C.POINTER(DnRownormConfig), _VP, _I64, _I64, _VP, _VP, _I32, _VP, _I64, _I32, _VP]),
    "dn_retnorm_scratch_bytes": (_I64, [_I64, _I64]),
    "dn_retnorm_init": (_I32, [_VP, _VP, _I64, _I32, _VP]),
    "dn_retnorm": (_I32, [C.POINTER(DnRetnormConfig), _VP, _VP, _I64, _I64, _VP, _VP, _VP, _I32, _VP, _I64, _I32, _VP]),
    "dn_minibatch_scratch_bytes": (_I64, [_I64]),
    "dn_minibatch_permutation": (_I32, [C.c_uint64, C.c_uint64, _I64, _I64, _I64, _VP]),
    "dn_minibatch": (_I32, [C.POINTER(DnMinibatchConfig), C.POINTER(DnMinibatchField), _I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _I64, _I32,
                            _VP]),
    "dn_ppo_loss_scratch_bytes": (_I64, [_I64, _I32]),
    "dn_ppo_loss": (_I32, [C.POINTER(DnPpoLossConfig), _I64] + [_VP] * 15 + [_I64, _I32, _VP]),
    "dn_adam_scratch_bytes": (_I64, [C.POINTER(C.c_int64), _I32]),
    "dn_adam_step": (_I32, [C.POINTER(DnAdamConfig), C.POINTER(DnAdamTensor), _VP, _VP, _VP, _VP, _I64, _I32, _VP]),
    "dn_replay_indices": (_I32, [C.c_uint64, C.c_uint64, _I64, _I64, _I64, _I64, _I64, _VP]),
    "dn_replay_sample": (_I32, [C.POINTER(DnReplayConfig), C.POINTER(DnReplaySource), _I64] + [_VP] * 8 + [_I32, _VP]),
    "dn_sac_loss_scratch_bytes": (_I64, [_I64, _I32]),
    "dn_sac_policy": (_I32, [C.POINTER(DnSacConfig), _I64] + [_VP] * 5 + [_I32, _VP]),
    "dn_sac_policy_backward": (_I32, [C.POINTER(DnSacConfig), _I64] + [_VP] * 7 + [_I32, _VP]),
    "dn_sac_critic_loss": (_I32, [C.POINTER(DnSacConfig), _I64] + [_VP] * 11 + [_I64, _I32, _VP]),
    "dn_sac_actor_loss": (_I32, [C.POINTER(DnSacConfig), _I64] + [_VP] * 10 + [_I64, _I32, _VP]),
    "dn_mlp_train_scratch_bytes": (_I64, [C.POINTER(DnMlpTrainConfig), C.POINTER(DnMlpTrainLayer), _I64]),
    "dn_mlp_train_forward": (_I32, [C.POINTER(DnMlpTrainConfig), C.POINTER(DnMlpTrainLayer), _VP, _I64, _VP, _VP, _I64, _I32, _VP]),
    "dn_mlp_train_backward": (_I32, [C.POINTER(DnMlpTrainConfig), C.POINTER(DnMlpTrainLayer), _VP, _VP, _I64, _VP, _VP, _I64, _I32, _VP]),
    "dn_sac_train_scratch_bytes": (_I64, [C.POINTER(DnSacTrainConfig), C.POINTER(DnMlpTrainLayer), _I64]),
    "dn_sac_train_forward": (_I32, [C.POINTER(DnSacTrainConfig), C.POINTER(DnMlpTrainLayer), _VP, _VP, _I64, C.POINTER(_VP), _VP, _I64, _I32, _VP]),
    "dn_sac_train_backward": (_I32, [C.POINTER(DnSacTrainConfig), C.POINTER(DnMlpTrainLayer), _VP, _VP, C.POINTER(_VP), _I64, _VP, _VP, _VP, _I64,
                                     _I32, _VP]),
    "dn_polyak_update": (_I32, [_I32, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_I64), C.c_double, _I32, _VP]),
    "dn_lstm_scratch_bytes": (_I64, [C.POINTER(DnLstmConfig), _I64, _I64]),
    "dn_lstm_forward": (_I32, [C.POINTER(DnLstmConfig), C.POINTER(DnLstmParams), _VP, _VP, _VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _I64, _I32,
                               _VP]),
    "dn_lstm_backward": (_I32, [C.POINTER(DnLstmConfig), C.POINTER(DnLstmParams), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _VP, _VP, _I64, _I32,
                                _VP]),
    "dn_set_launch_events":(_I32, [_VP, _VP, _VP]),
    "dn_state_bytes": (_I64, [_I64, _I32]),
    "dn_enable_dynamics": (_I32, [_VP, C.POINTER(DnDynamicsConfig)]),
    "dn_set_dynamics": (_I32, [_VP, _VP, _VP]),
    "dn_get_dynamics": (_I32, [_VP, _VP, _VP]),
    "dn_get_dynamics_config": (_I32, [_VP, C.POINTER(DnDynamicsConfig)]),
    "dn_enable_wind": (_I32, [_VP, C.POINTER(DnWindConfig)]),
    "dn_set_wind": (_I32, [_VP, _VP, _VP, _VP]),
    "dn_get_wind": (_I32, [_VP, _VP, _VP, _VP]),
    "dn_get_wind_config": (_I32, [_VP, C.POINTER(DnWindConfig)]),
    "dn_enable_actuator": (_I32, [_VP, C.POINTER(DnActuatorConfig)]),
    "dn_set_actuator": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "dn_get_actuator": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "dn_get_actuator_config": (_I32, [_VP, C.POINTER(DnActuatorConfig)]),
    "dn_enable_sensor": (_I32, [_VP, C.POINTER(DnSensorConfig)]),
    "dn_set_sensor": (_I32, [_VP, _VP, _VP, _VP, _VP]),
    "dn_get_sensor": (_I32, [_VP, _VP, _VP, _VP, _VP]),
    "dn_get_sensor_config": (_I32, [_VP, C.POINTER(DnSensorConfig)]),
    "dn_enable_privileged": (_I32, [_VP, C.POINTER(DnPrivilegedConfig)]),
    "dn_get_privileged_config": (_I32, [_VP, C.POINTER(DnPrivilegedConfig)]),
    "dn_bind_privileged": (_I32, [_VP, _VP, _VP, _I64]),
    "dn_enable_goal": (_I32, [_VP, C.POINTER(DnGoalConfig)]),
    "dn_get_goal_config": (_I32, [_VP, C.POINTER(DnGoalConfig)]),
    "dn_bind_goal": (_I32, [_VP, _VP, _VP, _I64]),
    "dn_enable_tracks": (_I32, [_VP, C.POINTER(DnTrackBankConfig)]),
    "dn_set_tracks": (_I32, [_VP, _VP, _VP]),
    "dn_get_tracks": (_I32, [_VP, _VP, _VP, _VP]),
    "dn_get_track_stats": (_I32, [_VP, _VP, _I32]),
    "dn_get_track_bank_config": (_I32, [_VP, C.POINTER(DnTrackBankConfig)]),
}

_lib = None


def _truthy(name):
    """An on / off environment switch, spelt as dn_create accepts it (anything else is left for dn_create to refuse)."""
    return os.environ.get(name, "").strip().lower() in ("1", "true", "on", "yes")


def library_path():
    # DN_LIB_PATH: an alternative build of the same ABI (A/B measurements of kernel variants).  DN_EXACT_NORM=1: the build with the
    # normaliser's float64 output stage (libdronenav_exact.so, include/dronenav.h DN_EXACT_FLAG_NORM).  Default = the in-tree library.
    if os.environ.get("DN_LIB_PATH"):
        return os.environ["DN_LIB_PATH"]
    return _build.LIB_PATH_EXACT if _truthy("DN_EXACT_NORM") else _build.LIB_PATH


def load():
    """Load libdronenav.so (built in-tree by build.build_library / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise DroneNavLibraryError(
            f"{path} is missing: run `python __graft_entry__.py` (or drl-dronenavigation_amd/build.py) to compile "
            "the HIP kernels with hipcc.  This package has no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  The device pointers
    # handed across the C ABI come from torch's allocator, so both must share ONE HIP runtime instance:
    # import torch first, and the dynamic loader resolves our NEEDED libamdhip64.so.7 to the copy torch
    # already mapped.  (Pure-C users link against the system runtime as usual.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = C.CDLL(path)
    except OSError as exc:
        raise DroneNavLibraryError(f"cannot load {path}: {exc}") from exc
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise DroneNavLibraryError(f"{path} does not export {name}") from exc
        fn.restype = res
        fn.argtypes = args
    if lib.dn_abi_version() != ABI_VERSION:
        raise DroneNavLibraryError(f"{path}: ABI {lib.dn_abi_version()} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(status):
    if status != DN_OK:
        raise DroneNavError(status, load().dn_last_error().decode("utf-8", "replace"))
