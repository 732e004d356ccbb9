"""The non-finite guard's ABI surface without a GPU: the constants and struct members of
include/pgx.h mirrored in abi.py, the guard off by default, and the constructor's mode check."""
import ctypes as C
import inspect
import os
import re

import pytest

import panda_gym_amd as pg
from panda_gym_amd import abi
from panda_gym_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(ROOT, "include", "pgx.h")) as f:
        return f.read()


def test_error_bits_match_header():
    hdr = _header()
    assert abi.ERR_NONFINITE == int(re.search(r"#define PGX_ERR_NONFINITE (\d+)u", hdr).group(1)) == 2
    assert abi.ERR_AO_OBSTACLE == int(re.search(r"#define PGX_ERR_AO_OBSTACLE (\d+)u", hdr).group(1)) == 1
    assert abi.ERR_NONFINITE & abi.ERR_AO_OBSTACLE == 0


def test_config_field_takes_the_pad_slot():
    """pgx_config.nonfinite_guard sits where pad1 sat: between no_auto_reset and seed, the struct
    no larger (the header's own layout is test_model_and_abi's)."""
    hdr = _header()
    cfg = hdr[hdr.index("typedef struct pgx_config {"):hdr.index("} pgx_config;")]
    assert "pad1" not in cfg and re.search(r"int32_t nonfinite_guard;", cfg)
    f = abi.PgxConfig
    assert not hasattr(f, "pad1")
    assert f.nonfinite_guard.offset == f.no_auto_reset.offset + 4 and f.nonfinite_guard.size == 4
    assert f.seed.offset == f.nonfinite_guard.offset + 4


def test_step_out_gains_a_last_member():
    hdr = _header()
    out = hdr[hdr.index("typedef struct pgx_step_out {"):hdr.index("} pgx_step_out;")]
    members = re.findall(r"^\s+(?:float|uint8_t)\* (\w+);", out, re.M)
    assert members[-1] == "nonfinite" and members[-2] == "task_truncated"
    names = [n for n, _ in abi.PgxStepOut._fields_]
    assert names == ["obs", "achieved_goal", "desired_goal", "reward", "success", "terminated", "truncated",
                     "terminal_obs", "terminal_achieved_goal", "terminal_desired_goal", "task_truncated",
                     "nonfinite"]
    assert abi.PgxStepOut.nonfinite.offset == C.sizeof(abi.PgxStepOut) - C.sizeof(C.c_void_p)
    assert abi.PgxStepOut().nonfinite is None   # NULL unless a caller sets it: skipped


@pytest.mark.parametrize("env_id", ["PandaReach-v3", "PandaPush-v3", "PandaReachAO-v3"])
def test_make_config_leaves_the_guard_off(env_id):
    model = abi.make_model(load_model("panda_custom0"), ee_link=11)
    params = abi.default_sim_params()
    cfg = abi.make_config(pg.envs.spec(env_id), 64, model, params, seed=1)
    assert cfg.nonfinite_guard == 0


def test_constructor_signature_and_mode_check():
    """nonfinite="off" is the default of both env classes, and an unknown mode is a ValueError raised
    before anything touches a device (this test runs without one)."""
    for cls in (pg.PandaVecEnv, pg.PandaEnv):
        assert inspect.signature(cls.__init__).parameters["nonfinite"].default == "off"
    assert pg.envs.NONFINITE_MODES == ("off", "reset", "raise")
    for bad in ("on", "Reset", "", None, 1):
        with pytest.raises(ValueError, match="nonfinite"):
            pg.PandaVecEnv("PandaReach-v3", num_envs=4, device="cuda:0", nonfinite=bad)
        with pytest.raises(ValueError, match="nonfinite"):
            pg.PandaEnv("PandaReach-v3", device="cuda:0", nonfinite=bad)
