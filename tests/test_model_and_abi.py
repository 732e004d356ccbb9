"""Model tables (URDF -> Bullet multibody) and the C-ABI boundary, on CPU (no GPU calls)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from abi_checks import header_layout
from panda_gym_amd import abi
from panda_gym_amd.model import bullet_quicksort_equal_keys, forward_kinematics, load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_link_order_matches_reference_indices():
    """custom_0 links 0-6 panda_link1..7, 9 panda_ee, 11 panda_rightfinger (ee_link, panda.py:68)."""
    m = load_model("panda_custom0")
    assert m.link_names[:7] == [f"panda_link{i}" for i in range(1, 8)]
    assert m.link_names[9] == "panda_ee" and m.link_names[11] == "panda_rightfinger"
    assert m.n_dofs == 7 and all(t == 4 for t in m.jtype[7:])


def test_neutral_ee_position():
    """EE = COM of panda_rightfinger at the neutral pose (panda.py:67), base (-0.6, 0, 0)."""
    m = load_model("panda_custom0")
    fk = forward_kinematics(m, [0, -0.3, 0, -2.2, 0, 2.0, math.pi / 4], base_pos=(-0.6, 0, 0))
    assert np.allclose(fk["C"][11], [-0.11845, 0.01, 0.4375], atol=1e-4)


def test_inertia_is_bullet_aabb_rule():
    """No URDF_USE_INERTIA_FROM_FILE: inertia from the collision AABB, not the URDF <inertia> 0.1."""
    m = load_model("panda_custom0")
    assert all(abs(I[0] - 0.1) > 1e-3 for I, ms in zip(m.inertia, m.mass) if ms > 0)
    # finger links have mass but no collision: empty-compound AABB (2 * margin)
    assert 0 < m.inertia[11][0] < 1e-6


def test_quicksort_permutation_equal_keys():
    assert bullet_quicksort_equal_keys([0, 1]) == [1, 0]
    p = bullet_quicksort_equal_keys(list(range(14)))
    assert sorted(p) == list(range(14))


def test_row_header_matches_model():
    m = load_model("panda_custom0")
    kinds, dofs = m.row_table()
    hdr = open(os.path.join(ROOT, "panda-gym_amd", "csrc", "pgx_rows.h")).read()
    codes = [int(x) for x in re.search(r"\{([0-9, ]+)\}", hdr).group(1).split(",")]
    assert codes == [int(k) << 4 | int(d) for k, d in zip(kinds, dofs)]


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "pgx.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\*?\s+\*?(pgx_[a-z_0-9]+)\s*\(", hdr, re.M)))


def test_libpgx_exports_every_declared_symbol():
    from panda_gym_amd import _native

    lib = _native.load()
    decl = _declared_functions()
    assert len(decl) >= 14
    for name in decl:
        assert hasattr(lib, name), name
    assert set(decl) == set(_native.EXPORTS)
    assert lib.pgx_version().startswith(b"pgx")


def _declarations():
    """(return type, name, [parameter declarations]) of every function include/pgx.h declares."""
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?[a-z_0-9]+\*?)\s+\*?(pgx_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", hdr,
                                        re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out.append((" ".join(ret.split()), name, [] if params == ["void"] else params))
    return out


def test_signature_table_matches_the_header():
    """_native.SIGNATURES against the declarations of include/pgx.h, without a library: the number of
    parameters; a scalar parameter has the ctypes type of its C type; a pointer or a handle has c_void_p
    or a POINTER(...); the restype is None for void, c_char_p for const char*, c_int64 for int64_t and
    ctypes' default for int."""
    from panda_gym_amd import _native

    scalars = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    restypes = {"void": None, "const char*": C.c_char_p, "int64_t": C.c_int64, "int": _native.INT}
    decl = _declarations()
    assert sorted(d[1] for d in decl) == _declared_functions()   # (every declaration was parsed)
    assert set(_native.SIGNATURES) == {d[1] for d in decl} and _native.EXPORTS == list(_native.SIGNATURES)
    for ret, name, params in decl:
        argtypes, restype = _native.SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for a, p in zip(argtypes, params):
            ctype = [w for w in p.split()[:-1] if w != "const"]
            if "*" in p or ctype[-1].endswith("_handle"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert ctype[-1] in scalars and a is scalars[ctype[-1]], (name, p)
                assert C.sizeof(a) == {"int": 4, "int32_t": 4}.get(ctype[-1], 8), (name, p)
        assert ret in restypes and restype is restypes[ret], (name, ret)


def test_host_only_calls_without_gpu():
    from panda_gym_amd import _native

    lib = _native.load()
    cfg = abi.make_config(abi.EnvSpec(), 8, abi.make_model(load_model("panda_custom0")), abi.default_sim_params())
    assert lib.pgx_obs_dim(C.byref(cfg)) == 6 and lib.pgx_action_dim(C.byref(cfg)) == 3
    cfg.task = 7                                                 # Slide/Flip/Stack: out of scope
    h = C.c_void_p()
    assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) < 0      # unsupported task fails loudly
    assert b"task" in lib.pgx_last_error()
    cfg.task, cfg.contacts = abi.TASK_PUSH, 0
    assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) < 0      # an object needs the contact solver
    assert b"contacts" in lib.pgx_last_error()
    cfg.contacts, cfg.lanes_per_env = abi.CONTACTS_FULL, 1   # the full manifold budget: 16 lanes only
    assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) == -3
    assert b"16-lane" in lib.pgx_last_error()
    cfg.contacts = 3
    assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) < 0
    assert lib.pgx_step(None, None, None, None) < 0


def test_compiled_default_model_is_current():
    """The constant block the kernels are compiled with (pgx_default_model.h) is the one pgx_create
    folds today for the default parameters; other parameters are refused before any HIP call."""
    from panda_gym_amd import _native
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_default_model

    txt, _ = gen_default_model.render()
    assert txt == open(gen_default_model.OUT).read(), "run python tools/gen_default_model.py"
    lib = _native.load()
    params = abi.default_sim_params()
    params.dt *= 2
    cfg = abi.make_config(abi.EnvSpec(), 8, abi.make_model(load_model("panda_custom0")), params)
    h = C.c_void_p()
    assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) == -3   # PGX_E_UNSUPPORTED
    assert b"compiled for" in lib.pgx_last_error()
    # the scene's table box is part of the block too (round 6): another table, centre or plane top
    for field, k, v in (("table_center", 2, -0.25), ("table_half", 0, 0.6), ("plane_z", None, -0.5)):
        cfg = abi.make_config(abi.EnvSpec(), 8, abi.make_model(load_model("panda_custom0")), abi.default_sim_params())
        if k is None:
            setattr(cfg, field, v)
        else:
            getattr(cfg, field)[k] = v
        assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) == -3, field
        assert b"compiled for" in lib.pgx_last_error()
    # the substep count is a runtime loop bound, not part of the block
    params = abi.default_sim_params(n_substeps=1)
    cfg = abi.make_config(abi.EnvSpec(), 8, abi.make_model(load_model("panda_custom0")), params)
    rc = lib.pgx_create(C.byref(cfg), 0, C.byref(h))
    assert rc != -3 or b"compiled for" not in lib.pgx_last_error()
    if rc == 0:
        lib.pgx_destroy(h)


def test_default_library_refuses_other_joint_forces():
    """pgx_config.joint_forces (PandaVecEnv(joint_forces=...)) reaches the constant block as the
    motor rows' impulse bound, joint_forces x dt: the default library refuses other values before
    any HIP call and names the block's word, as for every other compiled parameter."""
    from panda_gym_amd import _native

    lib = _native.load()
    h = C.c_void_p()
    words = []
    for d, f in ((0, 0.0), (6, 6.0)):   # a limp first joint; another force on the last arm joint
        cfg = abi.make_config(abi.EnvSpec(), 8, abi.make_model(load_model("panda_custom0")), abi.default_sim_params())
        assert cfg.joint_forces[d] == abi.JOINT_FORCES[d] != f
        cfg.joint_forces[d] = f
        assert lib.pgx_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_UNSUPPORTED
        msg = lib.pgx_last_error().decode()
        assert "compiled for" in msg
        words.append(int(re.search(r"constant block word (\d+)", msg).group(1)))
    assert words[1] == words[0] + 6, words   # max_impulse[0], max_impulse[6]


def test_constants_match_header():
    hdr = open(os.path.join(ROOT, "include", "pgx.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", hdr).group(1))

    from oracle import oracle as orc

    for name in ("OBJECT_POINTS", "ROBOT_POINTS", "ROBOT_POINTS_ARM", "ROBOT_POINTS_ONE_LANE", "MANIFOLD_POOL",
                 "MANIFOLD_POOL_AO", "MANIFOLD_POINT", "PCG64_WORDS"):
        assert getattr(abi, name) == define("PGX_" + name), name
    assert orc.OBJECT_POINTS == abi.OBJECT_POINTS and orc.ROBOT_MAX >= abi.ROBOT_POINTS
    for name in ("PGX_E_INVALID", "PGX_E_HIP", "PGX_E_UNSUPPORTED", "PGX_E_NOMEM"):
        assert getattr(abi, name) == int(re.search(rf"#define {name} (-\d+)", hdr).group(1)), name
    assert abi.AO_OBSTACLES == define("PGX_AO_OBSTACLES") and abi.MAX_CAPSULES == define("PGX_MAX_CAPSULES")


def test_struct_layout_matches_c():
    """ctypes mirror == C layout of include/pgx.h (sizeof, and offsetof of every field, via gcc)."""
    header_layout({"pgx_model": abi.PgxModel, "pgx_sim_params": abi.PgxSimParams, "pgx_config": abi.PgxConfig,
                   "pgx_step_out": abi.PgxStepOut, "pgx_state_view": abi.PgxStateView,
                   "pgx_replay_config": abi.PgxReplayConfig, "pgx_transition": abi.PgxTransition,
                   "pgx_replay_batch": abi.PgxReplayBatch})
