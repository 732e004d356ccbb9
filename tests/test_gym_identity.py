"""Class identity at the Python boundary (RobotTaskEnv(gym.Env) with spaces.Dict of spaces.Box,
core.py:4-7, 255, 274-280; SB3 make_vec_env / VecEnv consumers, setup_training.py:43-47): where
gymnasium and stable-baselines3 import, PandaEnv is a gymnasium.Env, PandaVecEnv an SB3 VecEnv (no
abstract method left), the spaces are gymnasium's and the env ids are in gymnasium's registry;
without them the stand-ins are unchanged.  Neither package is installed here, so the test imports
the package under minimal stub modules (tests/gym_stubs.py) in a fresh interpreter."""
import json
import os
import subprocess
import sys

import pytest

from gym_stubs import write_stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
import inspect, json
import gymnasium, gymnasium.spaces as S
from stable_baselines3.common.vec_env import VecEnv
import panda_gym_amd as pg
from panda_gym_amd import envs
obs, act = envs.make_spaces(6, 3)
pg.register_envs(50)
pg.register_envs(50)   # a second call registers nothing twice
reg = gymnasium.registry["PandaReach-v3"]
out = {
    "vec_is_vecenv": issubclass(envs.PandaVecEnv, VecEnv),
    "vec_abstract": sorted(getattr(envs.PandaVecEnv, "__abstractmethods__", ())),
    "env_is_gym": issubclass(envs.PandaEnv, gymnasium.Env),
    "obs_is_dict": isinstance(obs, S.Dict),
    "obs_keys": sorted(obs.spaces),
    "obs_boxes": all(isinstance(obs.spaces[k], S.Box) for k in obs.spaces),
    "obs_shape": list(obs.spaces["observation"].shape),
    "obs_bounds": [float(obs.spaces["observation"].low[0]), float(obs.spaces["observation"].high[0])],
    "act_is_box": isinstance(act, S.Box),
    "act_bounds": [float(act.low[0]), float(act.high[0]), str(act.dtype)],
    "registered": sorted(k for k in gymnasium.registry if k.startswith("Panda")),
    "reach_entry": reg["entry_point"], "reach_kwargs": reg["kwargs"], "reach_steps": reg["max_episode_steps"],
}
if GPU:
    venv = pg.PandaVecEnv("PandaReach-v3", num_envs=8, device="cuda:0", seed=3)
    o = venv.reset()
    _, r, d, infos = venv.step(venv.action_space.low[None, :].repeat(8, 0) * 0.0)
    out.update(vec_instance=isinstance(venv, VecEnv), reset_infos=len(venv.reset_infos),
               render_mode=venv.render_mode, wrapped=venv.env_is_wrapped(object), n_infos=len(infos),
               obs_shape_vec=list(o["observation"].shape))
    venv.close()
    env = pg.make("PandaReach-v3")
    ob, info = env.reset(seed=1)
    out.update(env_instance=isinstance(env, gymnasium.Env), env_obs=sorted(ob), env_space=isinstance(env.observation_space, S.Dict))
    env.close()
print("PROBE " + json.dumps(out))
'''


def run_probe(tmp_path, gpu: bool) -> dict:
    stubs = write_stubs(str(tmp_path / "stubs"))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([stubs, ROOT] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-c", f"GPU = {gpu}\n" + PROBE], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1]
    return json.loads(line[len("PROBE "):])


def check_classes(out: dict) -> None:
    assert out["vec_is_vecenv"] and out["vec_abstract"] == [], out
    assert out["env_is_gym"], out
    assert out["obs_is_dict"] and out["obs_boxes"] and out["act_is_box"], out
    assert out["obs_keys"] == ["achieved_goal", "desired_goal", "observation"]
    assert out["obs_shape"] == [6] and out["obs_bounds"] == [-10.0, 10.0]
    assert out["act_bounds"] == [-1.0, 1.0, "float32"]
    assert "PandaReach-v3" in out["registered"] and "PandaPickAndPlaceJointsDense-v3" in out["registered"]
    assert "PandaReachAO-v3" in out["registered"]
    assert out["reach_entry"] == "panda_gym_amd.envs:PandaEnv" and out["reach_kwargs"] == {"env_id": "PandaReach-v3"}
    assert out["reach_steps"] == 50


def test_classes_are_gymnasium_and_sb3_where_importable(tmp_path):
    check_classes(run_probe(tmp_path, gpu=False))


def test_stand_ins_without_gymnasium_and_sb3():
    from panda_gym_amd import envs
    if envs._gym is not None or envs._sb3_vec is not None:
        pytest.skip("gymnasium / stable-baselines3 are installed")
    from panda_gym_amd._handle import Handle

    # (the handle base, then the stand-in for SB3's VecEnv)
    assert envs.PandaVecEnv.__bases__ == (Handle, object) and envs.PandaEnv.__bases__ == (object,)
    assert Handle.__bases__ == (object,)
    obs, act = envs.make_spaces(18, 3)
    assert isinstance(obs, envs.DictSpace) and isinstance(act, envs.Box)
    assert obs["observation"].shape == (18,) and act.shape == (3,) and act.dtype == "float32"
    assert float(obs["desired_goal"].low[0]) == -10.0 and float(act.high[0]) == 1.0


@pytest.mark.gpu
def test_instances_under_gymnasium_and_sb3(tmp_path):
    """The same under the stubs with live objects on the GPU: SB3's VecEnv constructor ran (reset_infos,
    render_mode), the SB3 step protocol answers, make() returns a gymnasium.Env."""
    out = run_probe(tmp_path, gpu=True)
    check_classes(out)
    assert out["vec_instance"] and out["reset_infos"] == 8 and out["render_mode"] is None
    assert out["wrapped"] == [False] * 8 and out["n_infos"] == 8 and out["obs_shape_vec"] == [8, 6]
    assert out["env_instance"] and out["env_space"]
    assert out["env_obs"] == ["achieved_goal", "desired_goal", "observation"]
