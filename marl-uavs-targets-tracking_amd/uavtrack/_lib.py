"""ctypes binding of include/uavtrack.h.  Loads libuavtrack.so from this directory and
fails loudly if it is missing -- there is no Python or CPU stand-in for the kernels."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# UAVTRACK_LIB points at another build of the same ABI (A/B timing of kernel variants)
LIB_PATH = os.environ.get("UAVTRACK_LIB") or os.path.join(_HERE, "libuavtrack.so")

ABI_VERSION = 1
OBS_DIM = 12
MAX_CLIMB = 8

c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)


class UavtrackConfig(C.Structure):
    """Mirror of `struct uavtrack_config` (include/uavtrack.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_envs", C.c_int32), ("n_uav", C.c_int32), ("m_targets", C.c_int32),
        ("dim", C.c_int32), ("na", C.c_int32), ("nc", C.c_int32),
        ("norm_n_uav", C.c_int32), ("norm_m_targets", C.c_int32),
        ("reward_mode", C.c_int32), ("horizon", C.c_int32), ("device_id", C.c_int32),
        ("env_offset", C.c_int64),
        ("x_max", C.c_double), ("y_max", C.c_double), ("z_max", C.c_double),
        ("dt", C.c_double), ("u_v_max", C.c_double), ("u_h_max", C.c_double), ("u_g_max", C.c_double),
        ("dc", C.c_double), ("dp", C.c_double), ("t_v_max", C.c_double),
        ("alpha", C.c_double), ("beta", C.c_double), ("gamma", C.c_double),
        ("cooperative", C.c_double),
    ]


class HostStep(C.Structure):
    """Mirror of `struct uavtrack_host_step` (include/uavtrack.h): host pointers into the library's pinned block."""
    _fields_ = [(k, C.c_void_p) for k in ("obs", "reward", "terms", "raw", "covered", "done",
                                          "ux", "uy", "uz", "uh", "ua", "tx", "ty", "tz", "th", "step_count")]


class LearnerConfig(C.Structure):
    """Mirror of `struct uavtrack_learner_config` (include/uavtrack.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("hidden", C.c_int32), ("n_actions", C.c_int32),
        ("loss", C.c_int32), ("pad_", C.c_int32), ("max_batch", C.c_int64),
        ("gamma", C.c_double), ("actor_lr", C.c_double), ("critic_lr", C.c_double),
    ]


class PmiTrainerConfig(C.Structure):
    """Mirror of `struct uavtrack_pmi_trainer_config` (include/uavtrack.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("hidden", C.c_int32), ("pad_", C.c_int32),
        ("max_batch", C.c_int64), ("lr", C.c_double),
    ]


class ReplayConfig(C.Structure):
    """Mirror of `struct uavtrack_replay_config` (include/uavtrack.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("max_capacity", C.c_int64), ("max_batch", C.c_int64),
        ("seed", C.c_uint64),
    ]


class ReplayRing(C.Structure):
    """Mirror of `struct uavtrack_replay_ring` (include/uavtrack.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("states", "actions", "rewards", "next_states", "priorities")] + [
        ("capacity", C.c_int64), ("pos", C.c_int64), ("count", C.c_int64)]


class EpisodeStatsConfig(C.Structure):
    """Mirror of `struct uavtrack_episode_stats_config` (include/uavtrack.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("device_id", C.c_int32), ("n_envs", C.c_int64), ("n_uav", C.c_int32),
        ("pad_", C.c_int32), ("env_offset", C.c_int64), ("max_steps", C.c_int64), ("log_capacity", C.c_int64),
    ]


class EpisodeRecord(C.Structure):
    """Mirror of `struct uavtrack_episode_record` (include/uavtrack.h): 64 bytes."""
    _fields_ = [
        ("ret", C.c_double), ("tracking", C.c_double), ("boundary", C.c_double), ("duplicate", C.c_double),
        ("average_covered", C.c_double), ("max_covered", C.c_double), ("env", C.c_int64), ("steps", C.c_int32),
        ("ordinal", C.c_int32),
    ]


class PmiTensors(C.Structure):
    """Mirror of `struct uavtrack_pmi_tensors` (include/uavtrack.h): 26 device pointers in PMI_STATE_KEYS order."""
    _fields_ = [("t", C.c_void_p * 26)]


class PmiSource(C.Structure):
    """Mirror of `struct uavtrack_pmi_source` (include/uavtrack.h)."""
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_int64)]


# the float entries of the reference PMINetwork's state_dict, its order (= struct uavtrack_pmi_tensors)
PMI_STATE_KEYS = tuple(f"{m}.{k}" for lin, bn in (("fc_comm", "bn_comm"), ("fc_obs", "bn_obs"),
                                                   ("fc_boundary_state", "bn_boundary_state"), ("fc1", "bn1"))
                       for m, k in ((lin, "weight"), (lin, "bias"), (bn, "weight"), (bn, "bias"),
                                    (bn, "running_mean"), (bn, "running_var"))) + ("fc2.weight", "fc2.bias")
PMI_TRAIN_TENSORS = 18                                    # PMINetwork.parameters()
PMI_MAX_SOURCES = 64                                      # UAVTRACK_PMI_MAX_SOURCES
PMI_BN_LAYERS = 4                                         # BatchNorm1d layers (num_batches_tracked entries)
LOSS_FORMS = ("reference", "per_sample")                  # enum uavtrack_actor_loss
TARGET_OFF, TARGET_POLYAK, TARGET_PERIODIC = 0, 1, 2       # enum uavtrack_target_mode
ADVANTAGE_RAW, ADVANTAGE_BATCH, ADVANTAGE_GIVEN = 0, 1, 2   # enum uavtrack_advantage_mode
LEARNER_ROW_TAIL = 8                                     # words behind the P gradient sums of a gradient row
LEARNER_MAX_ROWS = 64                                     # UAVTRACK_LEARNER_MAX_ROWS
REPLAY_MAX_NSTEP = 64                                     # UAVTRACK_REPLAY_MAX_NSTEP
LEARNER_TENSORS = 8                                       # parameter tensors: actor fc1.w fc1.b fc2.w fc2.b, critic likewise
ACTOR_SAMPLE, ACTOR_ARGMAX = 0, 1   # enum in include/uavtrack.h
PROF_CLASSES = ("rollout", "scorer", "mix", "ep_sums")   # UAVTRACK_PROF_* in include/uavtrack.h
PMI_SCHEMES = ("auto", "f16x3", "bf16x6", "fp32")         # enum uavtrack_pmi_scheme

# name -> (restype, argtypes); every symbol declared in include/uavtrack.h
SIGNATURES = {
    "uavtrack_version": (C.c_int, []),
    "uavtrack_last_error": (C.c_char_p, []),
    "uavtrack_create": (C.c_int, [C.POINTER(UavtrackConfig), C.POINTER(C.c_void_p)]),
    "uavtrack_destroy": (C.c_int, [C.c_void_p]),
    "uavtrack_reset": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "uavtrack_set_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 10 + [C.c_void_p]),
    "uavtrack_get_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 10 + [C.c_void_p]),
    "uavtrack_set_episodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_get_episodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_set_pmi_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    "uavtrack_set_pmi_scheme": (C.c_int, [C.c_void_p, C.c_int32]),
    "uavtrack_pmi_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_publish_pmi_weights": (C.c_int, [C.c_void_p, C.POINTER(PmiTensors), C.c_int32, C.c_void_p]),
    "uavtrack_pmi_publish_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_pmi_blob_floats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "uavtrack_get_pmi_blob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_pmi_inference": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "uavtrack_step": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6 + [C.c_void_p]),
    "uavtrack_step_accumulate": (C.c_int, [C.c_void_p] + [C.c_void_p] * 7 + [C.c_void_p]),
    "uavtrack_step_many": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]),
    "uavtrack_step_many_autoreset": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64] + [C.c_void_p] * 7 + [C.c_void_p]),
    "uavtrack_run_greedy": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64] + [C.c_void_p] * 7 + [C.c_void_p]),
    "uavtrack_greedy_actions": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "uavtrack_set_actor_weights": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    "uavtrack_publish_actor_weights": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    "uavtrack_get_actor_blob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_actor_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_run_actor": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32] + [C.c_void_p] * 8 + [C.c_void_p]),
    "uavtrack_run_actor_autoreset": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32] + [C.c_void_p] * 8
                                     + [C.c_void_p]),
    "uavtrack_run_greedy_autoreset": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 7 + [C.c_void_p]),
    "uavtrack_set_start_obs_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "uavtrack_set_target_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "uavtrack_set_raw_reward_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "uavtrack_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HostStep), C.c_void_p]),
    "uavtrack_pmi_pairs_scored": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "uavtrack_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "uavtrack_get_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_kernel_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "uavtrack_launch_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "uavtrack_variant_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "uavtrack_learner_create": (C.c_int, [C.POINTER(LearnerConfig), C.POINTER(C.c_void_p)]),
    "uavtrack_learner_destroy": (C.c_int, [C.c_void_p]),
    "uavtrack_learner_num_params": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "uavtrack_learner_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "uavtrack_learner_set_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_learner_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_learner_publish_actor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_learner_set_optimizer_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "uavtrack_learner_get_optimizer_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "uavtrack_learner_update": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 6),
    "uavtrack_learner_update_weighted": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                         + [C.c_void_p] * 7),
    "uavtrack_learner_row_floats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "uavtrack_learner_grad": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 4),
    "uavtrack_learner_grad_weighted": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                       + [C.c_void_p] * 5),
    "uavtrack_learner_update_discounted": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                           + [C.c_void_p] * 8),
    "uavtrack_learner_grad_discounted": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                         + [C.c_void_p] * 6),
    "uavtrack_learner_update_clipped": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                        + [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 6),
    "uavtrack_learner_grad_clipped": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                      + [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 4),
    "uavtrack_learner_update_stored": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                       + [C.c_void_p] * 5 + [C.c_double] + [C.c_void_p] * 6),
    "uavtrack_learner_grad_stored": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                     + [C.c_void_p] * 5 + [C.c_double] + [C.c_void_p] * 4),
    "uavtrack_learner_values": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_learner_set_target": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int64, C.c_void_p]),
    "uavtrack_learner_get_target": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "uavtrack_learner_sync_target": (C.c_int, [C.c_void_p, C.c_void_p]),
    "uavtrack_learner_set_target_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_learner_get_target_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_learner_values_target": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_learner_log_probs": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 3),
    "uavtrack_learner_log_probs_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                    C.c_void_p, C.c_void_p]),
    "uavtrack_learner_ratio_weights": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p,
                                                 C.c_double] + [C.c_void_p] * 4),
    "uavtrack_learner_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_learner_write_priorities": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 3),
    "uavtrack_learner_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_learner_set_regularisation": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "uavtrack_learner_get_regularisation": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "uavtrack_learner_set_diagnostics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_learner_set_advantage": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    "uavtrack_learner_get_advantage": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                 C.POINTER(C.c_void_p)]),
    "uavtrack_learner_set_advantage_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "uavtrack_learner_set_kl_stop": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "uavtrack_learner_get_kl_stop": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "uavtrack_learner_kl_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "uavtrack_pmi_trainer_create": (C.c_int, [C.POINTER(PmiTrainerConfig), C.POINTER(C.c_void_p)]),
    "uavtrack_pmi_trainer_destroy": (C.c_int, [C.c_void_p]),
    "uavtrack_pmi_trainer_num_params": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "uavtrack_pmi_trainer_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "uavtrack_pmi_trainer_set_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_pmi_trainer_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "uavtrack_pmi_trainer_set_optimizer_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "uavtrack_pmi_trainer_get_optimizer_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "uavtrack_pmi_trainer_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "uavtrack_pmi_trainer_publish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_pmi_trainer_train_many": (C.c_int, [C.c_void_p, C.POINTER(PmiSource), C.c_int32, C.c_int64, C.c_void_p,
                                                   C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "uavtrack_pmi_trainer_select": (C.c_int, [C.c_void_p, C.POINTER(PmiSource), C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "uavtrack_pmi_trainer_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_replay_create": (C.c_int, [C.POINTER(ReplayConfig), C.POINTER(C.c_void_p)]),
    "uavtrack_replay_destroy": (C.c_int, [C.c_void_p]),
    "uavtrack_replay_add": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64] + [C.c_void_p] * 5),
    "uavtrack_replay_add_rollout": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64, C.c_int64] + [C.c_void_p] * 5),
    "uavtrack_replay_add_rollout_episodes": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64, C.c_int64, C.c_int64]
                                             + [C.c_void_p] * 7),
    "uavtrack_replay_add_rollout_nstep": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_void_p, C.c_int64, C.c_int64,
                                                    C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_double, C.c_void_p]),
    "uavtrack_replay_add_rollout_lambda": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_void_p, C.c_int64, C.c_int64,
                                                     C.c_int64] + [C.c_void_p] * 7 + [C.c_double, C.c_double, C.c_void_p]),
    "uavtrack_replay_add_rollout_gae": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_int64, C.c_int64] + [C.c_void_p] * 9
                                        + [C.c_double, C.c_double, C.c_void_p]),
    "uavtrack_replay_sample": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64, C.c_double, C.c_double,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_replay_sample_annealed": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64, C.c_double, C.c_double,
                                                  C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_replay_sample_uniform": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64, C.c_void_p, C.c_void_p]),
    "uavtrack_replay_sample_sweep": (C.c_int, [C.c_void_p, C.POINTER(ReplayRing), C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "uavtrack_replay_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_episode_stats_create": (C.c_int, [C.POINTER(EpisodeStatsConfig), C.POINTER(C.c_void_p)]),
    "uavtrack_episode_stats_destroy": (C.c_int, [C.c_void_p]),
    "uavtrack_episode_stats_add": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_void_p]),
    "uavtrack_episode_stats_close": (C.c_int, [C.c_void_p, C.c_void_p]),
    "uavtrack_episode_stats_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), C.c_void_p]),
    "uavtrack_episode_stats_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` or "
                f"`make -C marl-uavs-targets-tracking_amd/csrc`.  uavtrack has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("UAVTRACK_LIB_OLDER_OK") and not hasattr(lib, name):
                continue              # A/B timing against an older build of the library (tools/sweep.py --lib)
            fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.uavtrack_version() != ABI_VERSION:
            raise RuntimeError(f"libuavtrack ABI {lib.uavtrack_version()} != binding {ABI_VERSION}")
        _lib = lib
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().uavtrack_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what or 'uavtrack'} failed: {msg}")


def ptr(t):
    """A tensor's device address as a void * argument (None for NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def tensor_arg(t, dtype, n: int, device, message: str):
    """t as a pointer argument may take it: None, or a contiguous `dtype` tensor of n elements on `device`; else
    ValueError(message).  Returns t."""
    if t is not None and (t.numel() != n or t.dtype != dtype or not t.is_contiguous() or t.device != device):
        raise ValueError(message)
    return t


def host_ptr(a):
    """A numpy array's address as a void * argument."""
    return a.ctypes.data_as(C.c_void_p)
