"""Loader for libpgx.so, the HIP/gfx950 implementation of the env step (C-ABI in include/pgx.h).

The product path has no CPU fallback: if the shared library is missing or does
not export the full ABI, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

from .abi import PGX_E_INVALID  # noqa: F401 (re-exported for the C-ABI tests)
from .abi import (PgxAcConfig, PgxAcIo, PgxAcWeights, PgxActorConfig, PgxActorIo, PgxActorWeights, PgxConfig, PgxMonitorConfig, PgxMonitorIo, PgxMonitorTotals, PgxNormConfig, PgxNormIo, PgxQcConfig, PgxQcIo, PgxQcWeights, PgxReplayBatch,
                  PgxReplayConfig, PgxReplayStep, PgxReplayViews, PgxRolloutBatch, PgxRolloutConfig, PgxRolloutIo,
                  PgxRolloutViews, PgxSdeActorConfig, PgxSdeActorIo, PgxSdeActorWeights, PgxStateView, PgxStepOut,
                  PgxTransition)

LIB_PATH = os.environ.get("PGX_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libpgx.so")

EXPORTS = [
    "pgx_version", "pgx_last_error", "pgx_obs_dim", "pgx_action_dim", "pgx_dev_model_bytes", "pgx_create", "pgx_destroy",
    "pgx_get_state", "pgx_reset", "pgx_step", "pgx_step_kernel", "pgx_sample_actions", "pgx_compute_reward",
    "pgx_state_bytes", "pgx_save_state", "pgx_restore_state", "pgx_snapshot", "pgx_restore", "pgx_release",
    "pgx_set_rng_streams", "pgx_get_rng_streams",
    "pgx_replay_create", "pgx_replay_destroy", "pgx_replay_add", "pgx_replay_size", "pgx_replay_sample",
    "pgx_replay_episode_arrays", "pgx_replay_row_dim", "pgx_replay_row_stride",
    "pgx_replay_set_last", "pgx_replay_collect", "pgx_replay_truncate_last_trajectory", "pgx_replay_state",
    "pgx_replay_arrays",
    "pgx_norm_create", "pgx_norm_destroy", "pgx_norm_step", "pgx_norm_reset", "pgx_norm_rows", "pgx_norm_apply",
    "pgx_norm_set_training", "pgx_norm_set_keys", "pgx_norm_get_stats", "pgx_norm_set_stats",
    "pgx_monitor_create", "pgx_monitor_destroy", "pgx_monitor_step", "pgx_monitor_reset", "pgx_monitor_clear",
    "pgx_monitor_set_targets", "pgx_monitor_get_totals", "pgx_monitor_read", "pgx_monitor_get_env_state",
    "pgx_rollout_row_dim", "pgx_rollout_row_stride", "pgx_rollout_create", "pgx_rollout_destroy", "pgx_rollout_add",
    "pgx_rollout_compute_returns_and_advantage", "pgx_rollout_permutation", "pgx_rollout_gather", "pgx_rollout_reset",
    "pgx_rollout_set_last", "pgx_rollout_state", "pgx_rollout_arrays",
    "pgx_actor_create", "pgx_actor_destroy", "pgx_actor_set_weights", "pgx_actor_forward", "pgx_actor_state",
    "pgx_actor_set_state", "pgx_actor_forward_host",
    "pgx_ac_create", "pgx_ac_destroy", "pgx_ac_set_weights", "pgx_ac_forward", "pgx_ac_values", "pgx_ac_state",
    "pgx_ac_set_state", "pgx_ac_forward_host",
    "pgx_sde_actor_create", "pgx_sde_actor_destroy", "pgx_sde_actor_set_weights", "pgx_sde_actor_reset_noise",
    "pgx_sde_actor_forward", "pgx_sde_actor_state", "pgx_sde_actor_set_state", "pgx_sde_actor_get_matrices",
    "pgx_sde_actor_set_matrices", "pgx_sde_actor_get_std", "pgx_sde_actor_forward_host",
    "pgx_qc_create", "pgx_qc_destroy", "pgx_qc_set_weights", "pgx_qc_get_weights", "pgx_qc_forward", "pgx_qc_target",
    "pgx_qc_polyak", "pgx_qc_sync_target", "pgx_qc_forward_host", "pgx_qc_target_host",
]


class PgxError(RuntimeError):
    """A libpgx call returned a negative status (message from pgx_last_error)."""


_libs = {}


def load(path: str = None):
    """Load libpgx.so (or another build of the same ABI, e.g. libpgx_rtmodel.so) once per path;
    raise loudly if it is absent (build with __graft_entry__.build())."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise PgxError(f"libpgx.so not found at {path}: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise PgxError(f"libpgx.so does not export {name}")
    lib.pgx_version.restype = C.c_char_p
    lib.pgx_last_error.restype = C.c_char_p
    lib.pgx_obs_dim.argtypes = [C.POINTER(PgxConfig)]
    lib.pgx_action_dim.argtypes = [C.POINTER(PgxConfig)]
    lib.pgx_dev_model_bytes.argtypes = [C.POINTER(PgxConfig), C.c_void_p, C.c_int64]
    lib.pgx_create.argtypes = [C.POINTER(PgxConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_destroy.argtypes = [C.c_void_p]
    lib.pgx_destroy.restype = None
    lib.pgx_get_state.argtypes = [C.c_void_p, C.POINTER(PgxStateView)]
    lib.pgx_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PgxStepOut), C.c_void_p]
    lib.pgx_step.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PgxStepOut), C.c_void_p]
    if hasattr(lib, "pgx_step_kernel"):   # (A/B runs load older builds with EXPORTS filtered)
        lib.pgx_step_kernel.argtypes = [C.c_void_p]
        lib.pgx_step_kernel.restype = C.c_char_p
    lib.pgx_sample_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pgx_compute_reward.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                       C.c_void_p]
    lib.pgx_state_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.pgx_save_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_restore_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_snapshot.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    lib.pgx_restore.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.pgx_release.argtypes = [C.c_void_p, C.c_int32]
    lib.pgx_set_rng_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_get_rng_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_replay_create.argtypes = [C.POINTER(PgxReplayConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_replay_row_dim.argtypes = [C.POINTER(PgxReplayConfig)]
    lib.pgx_replay_row_stride.argtypes = [C.POINTER(PgxReplayConfig)]
    lib.pgx_replay_destroy.argtypes = [C.c_void_p]
    lib.pgx_replay_destroy.restype = None
    lib.pgx_replay_add.argtypes = [C.c_void_p, C.POINTER(PgxTransition), C.c_void_p]
    lib.pgx_replay_size.argtypes = [C.c_void_p]
    lib.pgx_replay_size.restype = C.c_int64
    lib.pgx_replay_sample.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(PgxReplayBatch), C.c_void_p]
    lib.pgx_replay_episode_arrays.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_void_p)]
    lib.pgx_replay_set_last.argtypes = [C.c_void_p] * 5
    lib.pgx_replay_collect.argtypes = [C.c_void_p, C.POINTER(PgxReplayStep), C.c_void_p]
    lib.pgx_replay_truncate_last_trajectory.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.pgx_replay_state.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                     C.c_int32, C.c_void_p]
    lib.pgx_replay_arrays.argtypes = [C.c_void_p, C.POINTER(PgxReplayViews)]
    lib.pgx_norm_create.argtypes = [C.POINTER(PgxNormConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_norm_destroy.argtypes = [C.c_void_p]
    lib.pgx_norm_destroy.restype = None
    lib.pgx_norm_step.argtypes = [C.c_void_p, C.POINTER(PgxNormIo), C.c_void_p]
    lib.pgx_norm_reset.argtypes = [C.c_void_p, C.POINTER(PgxNormIo), C.c_void_p]
    lib.pgx_norm_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    lib.pgx_norm_apply.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.pgx_norm_set_training.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.pgx_norm_set_keys.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.pgx_norm_get_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_norm_set_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_monitor_create.argtypes = [C.POINTER(PgxMonitorConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_monitor_destroy.argtypes = [C.c_void_p]
    lib.pgx_monitor_destroy.restype = None
    lib.pgx_monitor_step.argtypes = [C.c_void_p, C.POINTER(PgxMonitorIo), C.c_void_p]
    lib.pgx_monitor_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_monitor_clear.argtypes = [C.c_void_p, C.c_void_p]
    lib.pgx_monitor_set_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_monitor_get_totals.argtypes = [C.c_void_p, C.POINTER(PgxMonitorTotals), C.c_void_p]
    lib.pgx_monitor_read.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.POINTER(C.c_int32), C.c_void_p]
    lib.pgx_monitor_get_env_state.argtypes = [C.c_void_p] * 6
    lib.pgx_rollout_row_dim.argtypes = [C.POINTER(PgxRolloutConfig)]
    lib.pgx_rollout_row_stride.argtypes = [C.POINTER(PgxRolloutConfig)]
    lib.pgx_rollout_create.argtypes = [C.POINTER(PgxRolloutConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_rollout_destroy.argtypes = [C.c_void_p]
    lib.pgx_rollout_destroy.restype = None
    lib.pgx_rollout_add.argtypes = [C.c_void_p, C.POINTER(PgxRolloutIo), C.c_void_p]
    lib.pgx_rollout_compute_returns_and_advantage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pgx_rollout_permutation.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.pgx_rollout_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(PgxRolloutBatch), C.c_void_p]
    lib.pgx_rollout_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.pgx_rollout_set_last.argtypes = [C.c_void_p] * 6
    lib.pgx_rollout_state.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int32, C.c_void_p]
    lib.pgx_rollout_arrays.argtypes = [C.c_void_p, C.POINTER(PgxRolloutViews)]
    lib.pgx_actor_create.argtypes = [C.POINTER(PgxActorConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_actor_destroy.argtypes = [C.c_void_p]
    lib.pgx_actor_destroy.restype = None
    lib.pgx_actor_set_weights.argtypes = [C.c_void_p, C.POINTER(PgxActorWeights), C.c_void_p]
    lib.pgx_actor_forward.argtypes = [C.c_void_p, C.POINTER(PgxActorIo), C.c_int32, C.c_void_p]
    lib.pgx_actor_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    lib.pgx_actor_set_state.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pgx_actor_forward_host.argtypes = [C.POINTER(PgxActorConfig), C.POINTER(PgxActorWeights), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pgx_ac_create.argtypes = [C.POINTER(PgxAcConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_ac_destroy.argtypes = [C.c_void_p]
    lib.pgx_ac_destroy.restype = None
    lib.pgx_ac_set_weights.argtypes = [C.c_void_p, C.POINTER(PgxAcWeights), C.c_void_p]
    lib.pgx_ac_forward.argtypes = [C.c_void_p, C.POINTER(PgxAcIo), C.c_int32, C.c_void_p]
    lib.pgx_ac_values.argtypes = [C.c_void_p] * 7
    lib.pgx_ac_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    lib.pgx_ac_set_state.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pgx_ac_forward_host.argtypes = [C.POINTER(PgxAcConfig), C.POINTER(PgxAcWeights), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pgx_sde_actor_create.argtypes = [C.POINTER(PgxSdeActorConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_sde_actor_destroy.argtypes = [C.c_void_p]
    lib.pgx_sde_actor_destroy.restype = None
    lib.pgx_sde_actor_set_weights.argtypes = [C.c_void_p, C.POINTER(PgxSdeActorWeights), C.c_void_p]
    lib.pgx_sde_actor_reset_noise.argtypes = [C.c_void_p] * 4
    lib.pgx_sde_actor_forward.argtypes = [C.c_void_p, C.POINTER(PgxSdeActorIo), C.c_int32, C.c_void_p]
    lib.pgx_sde_actor_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    lib.pgx_sde_actor_set_state.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pgx_sde_actor_get_matrices.argtypes = [C.c_void_p] * 3
    lib.pgx_sde_actor_set_matrices.argtypes = [C.c_void_p] * 3
    lib.pgx_sde_actor_get_std.argtypes = [C.c_void_p] * 3
    lib.pgx_sde_actor_forward_host.argtypes = [C.POINTER(PgxSdeActorConfig), C.POINTER(PgxSdeActorWeights)] + \
        [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3
    lib.pgx_qc_create.argtypes = [C.POINTER(PgxQcConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pgx_qc_destroy.argtypes = [C.c_void_p]
    lib.pgx_qc_destroy.restype = None
    lib.pgx_qc_set_weights.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PgxQcWeights), C.c_void_p]
    lib.pgx_qc_get_weights.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PgxQcWeights), C.c_void_p]
    lib.pgx_qc_forward.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PgxQcIo), C.c_int32, C.c_void_p]
    lib.pgx_qc_target.argtypes = [C.c_void_p, C.POINTER(PgxQcIo), C.c_int32, C.c_int32, C.c_void_p]
    lib.pgx_qc_polyak.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    lib.pgx_qc_sync_target.argtypes = [C.c_void_p, C.c_void_p]
    lib.pgx_qc_forward_host.argtypes = [C.POINTER(PgxQcConfig), C.POINTER(PgxQcWeights), C.POINTER(PgxQcIo), C.c_int32]
    lib.pgx_qc_target_host.argtypes = [C.POINTER(PgxQcConfig), C.POINTER(PgxQcWeights), C.POINTER(PgxQcIo), C.c_int32,
                                       C.c_int32]
    _libs[path] = lib
    return lib


def check(rc: int, what: str, lib=None) -> None:
    if rc != 0:
        msg = (lib or load()).pgx_last_error().decode(errors="replace")
        raise PgxError(f"{what} failed ({rc}): {msg}")
