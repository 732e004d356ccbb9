"""Loader for libpgx.so, the HIP/gfx950 implementation of the env step (C-ABI in include/pgx.h).

The product path has no CPU fallback: if the shared library is missing or does
not export the full ABI, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Tuple

from . import abi
from .abi import PGX_E_INVALID  # noqa: F401 (re-exported for the C-ABI tests)

LIB_PATH = os.environ.get("PGX_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libpgx.so")

INT = "int"   # a restype to leave alone: ctypes' default, C int
P, I32, I64, U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
ptr = C.POINTER


def _int(*argtypes) -> Tuple[list, Any]:
    return list(argtypes), INT


# Every entry point of include/pgx.h: name -> (argtypes, restype), by unit.
SIGNATURES: Dict[str, Tuple[list, Any]] = {
    "pgx_version": ([], C.c_char_p),
    "pgx_last_error": ([], C.c_char_p),
    "pgx_obs_dim": _int(ptr(abi.PgxConfig)),
    "pgx_action_dim": _int(ptr(abi.PgxConfig)),
    "pgx_dev_model_bytes": _int(ptr(abi.PgxConfig), P, I64),
    "pgx_create": _int(ptr(abi.PgxConfig), C.c_int, ptr(P)),
    "pgx_destroy": ([P], None),
    "pgx_get_state": _int(P, ptr(abi.PgxStateView)),
    "pgx_reset": _int(P, P, P, P, ptr(abi.PgxStepOut), P),
    "pgx_step": _int(P, P, ptr(abi.PgxStepOut), P),
    "pgx_step_kernel": ([P], C.c_char_p),
    "pgx_sample_actions": _int(P, P, U64, P),
    "pgx_compute_reward": _int(P, P, I64, I32, C.c_double, P, P),
    "pgx_state_bytes": _int(P, ptr(I64)),
    "pgx_save_state": _int(P, P, P),
    "pgx_restore_state": _int(P, P, P),
    "pgx_snapshot": _int(P, ptr(I32), P),
    "pgx_restore": _int(P, I32, P),
    "pgx_release": _int(P, I32),
    "pgx_set_rng_streams": _int(P, P, P),
    "pgx_get_rng_streams": _int(P, P, P),

    "pgx_replay_create": _int(ptr(abi.PgxReplayConfig), C.c_int, ptr(P)),
    "pgx_replay_destroy": ([P], None),
    "pgx_replay_add": _int(P, ptr(abi.PgxTransition), P),
    "pgx_replay_size": ([P], I64),
    "pgx_replay_sample": _int(P, I64, U64, ptr(abi.PgxReplayBatch), P),
    "pgx_replay_episode_arrays": _int(P, ptr(P), ptr(P), ptr(P)),
    "pgx_replay_row_dim": _int(ptr(abi.PgxReplayConfig)),
    "pgx_replay_row_stride": _int(ptr(abi.PgxReplayConfig)),
    "pgx_replay_set_last": _int(*[P] * 5),
    "pgx_replay_collect": _int(P, ptr(abi.PgxReplayStep), P),
    "pgx_replay_truncate_last_trajectory": _int(P, I32, P),
    "pgx_replay_state": _int(P, ptr(I64), ptr(I32), ptr(C.c_uint32), I32, P),
    "pgx_replay_arrays": _int(P, ptr(abi.PgxReplayViews)),

    "pgx_norm_create": _int(ptr(abi.PgxNormConfig), C.c_int, ptr(P)),
    "pgx_norm_destroy": ([P], None),
    "pgx_norm_step": _int(P, ptr(abi.PgxNormIo), P),
    "pgx_norm_reset": _int(P, ptr(abi.PgxNormIo), P),
    "pgx_norm_rows": _int(P, P, I64, I32, I32, P),
    "pgx_norm_apply": _int(P, I32, I32, P, P, I64, P),
    "pgx_norm_set_training": _int(P, I32, P),
    "pgx_norm_set_keys": _int(P, I32, I32),
    "pgx_norm_get_stats": _int(*[P] * 6),
    "pgx_norm_set_stats": _int(*[P] * 6),

    "pgx_monitor_create": _int(ptr(abi.PgxMonitorConfig), C.c_int, ptr(P)),
    "pgx_monitor_destroy": ([P], None),
    "pgx_monitor_step": _int(P, ptr(abi.PgxMonitorIo), P),
    "pgx_monitor_reset": _int(P, P, P),
    "pgx_monitor_clear": _int(P, P),
    "pgx_monitor_set_targets": _int(P, P, P),
    "pgx_monitor_get_totals": _int(P, ptr(abi.PgxMonitorTotals), P),
    "pgx_monitor_read": _int(P, I32, *[P] * 6, ptr(I32), P),
    "pgx_monitor_get_env_state": _int(*[P] * 6),

    "pgx_rollout_row_dim": _int(ptr(abi.PgxRolloutConfig)),
    "pgx_rollout_row_stride": _int(ptr(abi.PgxRolloutConfig)),
    "pgx_rollout_create": _int(ptr(abi.PgxRolloutConfig), C.c_int, ptr(P)),
    "pgx_rollout_destroy": ([P], None),
    "pgx_rollout_add": _int(P, ptr(abi.PgxRolloutIo), P),
    "pgx_rollout_compute_returns_and_advantage": _int(P, P, P, P),
    "pgx_rollout_permutation": _int(P, U64, P, P),
    "pgx_rollout_gather": _int(P, P, I64, ptr(abi.PgxRolloutBatch), P),
    "pgx_rollout_reset": _int(P, P),
    "pgx_rollout_set_last": _int(*[P] * 6),
    "pgx_rollout_state": _int(P, ptr(I32), ptr(C.c_uint32), I32, P),
    "pgx_rollout_arrays": _int(P, ptr(abi.PgxRolloutViews)),

    "pgx_actor_create": _int(ptr(abi.PgxActorConfig), C.c_int, ptr(P)),
    "pgx_actor_destroy": ([P], None),
    "pgx_actor_set_weights": _int(P, ptr(abi.PgxActorWeights), P),
    "pgx_actor_forward": _int(P, ptr(abi.PgxActorIo), I32, P),
    "pgx_actor_state": _int(P, ptr(U64), P),
    "pgx_actor_set_state": _int(P, U64, P),
    "pgx_actor_forward_host": _int(ptr(abi.PgxActorConfig), ptr(abi.PgxActorWeights), P, P, P, I32, P, P),
    "pgx_actor_action_log_prob": _int(P, ptr(abi.PgxActorLpIo), I32, P),
    "pgx_actor_lp_state": _int(P, ptr(U64), P),
    "pgx_actor_lp_set_state": _int(P, U64, P),
    "pgx_actor_log_prob_host": _int(ptr(abi.PgxActorConfig), ptr(abi.PgxActorWeights), ptr(abi.PgxActorLpIo), I32),

    "pgx_ac_create": _int(ptr(abi.PgxAcConfig), C.c_int, ptr(P)),
    "pgx_ac_destroy": ([P], None),
    "pgx_ac_set_weights": _int(P, ptr(abi.PgxAcWeights), P),
    "pgx_ac_forward": _int(P, ptr(abi.PgxAcIo), I32, P),
    "pgx_ac_values": _int(*[P] * 7),
    "pgx_ac_state": _int(P, ptr(U64), P),
    "pgx_ac_set_state": _int(P, U64, P),
    "pgx_ac_forward_host": _int(ptr(abi.PgxAcConfig), ptr(abi.PgxAcWeights), P, P, P, I32, P, P),

    "pgx_sde_actor_create": _int(ptr(abi.PgxSdeActorConfig), C.c_int, ptr(P)),
    "pgx_sde_actor_destroy": ([P], None),
    "pgx_sde_actor_set_weights": _int(P, ptr(abi.PgxSdeActorWeights), P),
    "pgx_sde_actor_reset_noise": _int(*[P] * 4),
    "pgx_sde_actor_forward": _int(P, ptr(abi.PgxSdeActorIo), I32, P),
    "pgx_sde_actor_state": _int(P, ptr(U64), P),
    "pgx_sde_actor_set_state": _int(P, U64, P),
    "pgx_sde_actor_get_matrices": _int(P, P, P),
    "pgx_sde_actor_set_matrices": _int(P, P, P),
    "pgx_sde_actor_get_std": _int(P, P, P),
    "pgx_sde_actor_forward_host": _int(ptr(abi.PgxSdeActorConfig), ptr(abi.PgxSdeActorWeights), P, P, P, P, I32,
                                       P, P, P),
    "pgx_sde_actor_action_log_prob": _int(P, ptr(abi.PgxSdeActorLpIo), I32, P),
    "pgx_sde_actor_reset_batch_noise": _int(P, P, P),
    "pgx_sde_actor_get_batch_matrix": _int(P, P, P),
    "pgx_sde_actor_set_batch_matrix": _int(P, P, P),
    "pgx_sde_actor_batch_state": _int(P, ptr(U64), P),
    "pgx_sde_actor_batch_set_state": _int(P, U64, P),
    "pgx_sde_actor_log_prob_host": _int(ptr(abi.PgxSdeActorConfig), ptr(abi.PgxSdeActorWeights), P, P,
                                        ptr(abi.PgxSdeActorLpIo), I32),

    "pgx_qc_create": _int(ptr(abi.PgxQcConfig), C.c_int, ptr(P)),
    "pgx_qc_destroy": ([P], None),
    "pgx_qc_set_weights": _int(P, I32, ptr(abi.PgxQcWeights), P),
    "pgx_qc_get_weights": _int(P, I32, ptr(abi.PgxQcWeights), P),
    "pgx_qc_forward": _int(P, I32, ptr(abi.PgxQcIo), I32, P),
    "pgx_qc_target": _int(P, ptr(abi.PgxQcIo), I32, I32, P),
    "pgx_qc_polyak": _int(P, C.c_double, P),
    "pgx_qc_sync_target": _int(P, P),
    "pgx_qc_forward_host": _int(ptr(abi.PgxQcConfig), ptr(abi.PgxQcWeights), ptr(abi.PgxQcIo), I32),
    "pgx_qc_target_host": _int(ptr(abi.PgxQcConfig), ptr(abi.PgxQcWeights), ptr(abi.PgxQcIo), I32, I32),
    "pgx_qc_grad_workspace_floats": ([ptr(abi.PgxQcConfig), I32], I64),
    "pgx_qc_init_training": _int(P, C.c_double, C.c_double, C.c_double),
    "pgx_qc_critic_grad": _int(P, ptr(abi.PgxQcGradIo), I32, I32, P),
    "pgx_qc_get_grads": _int(P, ptr(abi.PgxQcWeights), P),
    "pgx_qc_adam_step": _int(P, P, P),
    "pgx_qc_get_opt_state": _int(P, ptr(abi.PgxQcWeights), ptr(abi.PgxQcWeights), ptr(U64), P),
    "pgx_qc_set_opt_state": _int(P, ptr(abi.PgxQcWeights), ptr(abi.PgxQcWeights), U64, P),
    "pgx_qc_critic_grad_host": _int(ptr(abi.PgxQcConfig), ptr(abi.PgxQcWeights), ptr(abi.PgxQcGradIo), I32, I32,
                                    ptr(abi.PgxQcWeights)),
    "pgx_qc_adam_step_host": _int(ptr(abi.PgxQcConfig), *[ptr(abi.PgxQcWeights)] * 4, ptr(U64), *[C.c_double] * 4),
}

# what load() requires of a library: a list the A/B tools filter before they load an older build
EXPORTS = list(SIGNATURES)


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
        fn = getattr(lib, name)
        fn.argtypes, restype = SIGNATURES[name]
        if restype is not INT:
            fn.restype = restype
    _libs[path] = lib
    return lib


def check(rc: int, what: str, lib=None) -> None:
    if rc != 0:
        msg = (lib or load()).pgx_last_error().decode(errors="replace")
        raise PgxError(f"{what} failed ({rc}): {msg}")
