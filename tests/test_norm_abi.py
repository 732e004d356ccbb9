"""The VecNormalize C-ABI (include/pgx.h, pgx_norm_*) without a GPU: the ctypes mirrors against the
header's layout through gcc, the exported entry points, pgx_norm_create's argument checks (made
before any device call), and the numpy restatement of RunningMeanStd the GPU tests compare against."""
import ctypes as C
import os

import numpy as np
import pytest

from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NORM_EXPORTS = ["pgx_norm_create", "pgx_norm_destroy", "pgx_norm_step", "pgx_norm_reset", "pgx_norm_rows",
                "pgx_norm_apply", "pgx_norm_set_training", "pgx_norm_set_keys", "pgx_norm_get_stats",
                "pgx_norm_set_stats"]


# ---------------------------------------------------------------- the restatement
class RunningMeanStd:
    """SB3 RunningMeanStd(epsilon=1e-4) in numpy fp64, written from the rules of include/pgx.h."""

    def __init__(self, shape=()):
        self.mean, self.var, self.count = np.zeros(shape, np.float64), np.ones(shape, np.float64), 1e-4

    def update(self, batch):
        x = np.asarray(batch).astype(np.float64)
        batch_mean, batch_var, n = np.mean(x, axis=0), np.var(x, axis=0), x.shape[0]
        delta = batch_mean - self.mean
        tot = self.count + n
        new_mean = self.mean + delta * n / tot
        m2 = self.var * self.count + batch_var * n + np.square(delta) * self.count * n / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


def test_struct_layout_matches_header():
    """ctypes mirrors of pgx_norm_config / pgx_norm_io == the header's sizeof / offsetof (gcc, as C)."""
    structs = {"pgx_norm_config": abi.PgxNormConfig, "pgx_norm_io": abi.PgxNormIo}
    header_layout(structs)
    hdr = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert "#define PGX_NORM_KEY_ALL 7" in hdr and abi.NORM_KEY_ALL == 7
    assert "#define PGX_NORM_REWARD 3" in hdr and abi.NORM_REWARD == 3
    assert [abi.NORM_KEY_BITS[k] for k in abi.NORM_KEYS] == [1, 2, 4]


def test_library_exports_the_entry_points():
    assert_exported(NORM_EXPORTS)


@pytest.mark.parametrize("field,value", [("n_envs", 0), ("n_envs", -3), ("obs_dim", 0), ("obs_dim", -1),
                                         ("epsilon", -1e-8), ("obs_dim", 250), ("key_mask", 8),
                                         ("clip_obs", 0.0)])
def test_create_rejects_bad_config_without_a_device(field, value):
    """PGX_E_INVALID comes from the argument check, before any HIP call: this runs without a GPU
    (a HIP failure would be PGX_E_HIP)."""
    lib = _native.load()
    cfg = abi.PgxNormConfig(64, 6, abi.NORM_KEY_ALL, 1, 10.0, 10.0, 0.99, 1e-8)
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.pgx_norm_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_norm_create" in msg
    assert field.split("_")[0].encode() in msg   # the message names the field
    # the null-handle checks of the other entry points
    assert lib.pgx_norm_step(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_norm_set_keys(None, 7, 1) == abi.PGX_E_INVALID


def test_python_surface_is_exported():
    import inspect

    import panda_gym_amd as pg

    sig = inspect.signature(pg.VecNormalize.__init__).parameters
    assert list(sig)[1:] == ["venv", "training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma",
                             "epsilon", "norm_obs_keys"]
    assert [sig[k].default for k in list(sig)[2:]] == [True, True, True, 10.0, 10.0, 0.99, 1e-8, None]
    for name in ("reset_tensors", "step_tensors", "capture_steps", "reset", "seed", "step_async", "step_wait", "step",
                 "normalize_obs", "normalize_reward", "unnormalize_obs", "unnormalize_reward", "get_original_obs",
                 "get_original_reward", "obs_rms", "ret_rms", "returns", "training", "norm_obs", "norm_reward",
                 "save", "load"):
        assert hasattr(pg.VecNormalize, name), name
    from panda_gym_amd.normalize import key_mask

    assert key_mask(None) == 7 and key_mask(["observation"]) == 1 and key_mask(["desired_goal", "achieved_goal"]) == 6
    with pytest.raises(ValueError, match="norm_obs_keys"):
        key_mask(["goal"])
    assert "env" in inspect.signature(pg.HerReplayBuffer.sample_into).parameters


def test_restatement_two_updates_equal_hand_merged_moments():
    """The reference the GPU tests use, pinned: two updates of known small arrays equal the moments
    of (prior, batch 1, batch 2) merged by hand -- the prior is `count` = 1e-4 pseudo-samples of
    mean 0 and variance 1 -- to 1e-15."""
    b1 = np.array([[1.0, -2.0], [3.0, 0.5], [2.0, 4.0]], dtype=np.float32)
    b2 = np.array([[0.25, 8.0], [-1.5, 1.0]], dtype=np.float32)
    rms = RunningMeanStd((2,))
    rms.update(b1)
    rms.update(b2)
    # by hand: one weighted population of the prior (weight w0 = 1e-4, mean 0, variance 1) and the
    # five rows, about its own mean m: mean = sum(x) / W, M2 = w0 * (1 + m^2) + sum((x - m)^2)
    rows = np.concatenate([b1, b2]).astype(np.float64)
    w0 = 1e-4
    W = 5 + w0
    mean = rows.sum(axis=0) / W
    var = (w0 * (1.0 + np.square(mean)) + np.square(rows - mean).sum(axis=0)) / W
    assert rms.count == pytest.approx(W, rel=1e-15, abs=0)
    np.testing.assert_allclose(rms.mean, mean, rtol=1e-15, atol=0)
    np.testing.assert_allclose(rms.var, var, rtol=1e-15, atol=0)
    assert rms.mean[0] == pytest.approx(4.75 / W, rel=1e-15, abs=0)   # column 0's sum in closed form
