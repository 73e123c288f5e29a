#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/mpe_reference_cases.npz by stepping the REFERENCE's multi-agent particle
environment for the ``simple_reference`` scenario (onpolicy/envs/mpe: core.py physics and communication state,
environment.py MultiDiscrete action decoding, scenarios/simple_reference.py goals / reward / observation) from seeded
initial states with seeded one-hot MultiDiscrete actions: one 25-step episode per seed.  Needs the reference tree
(oracle/ref_import.py); gym and seaborn are stubbed for the import as in oracle/make_golden_mpe.py.

    python tools/make_golden_mpe_reference.py

Per case ``ref<i>_``: post-reset pos0 / vel0 / landmarks / goals / obs0, per step actions (one-hot [T, 2, 15]) and
action_idx ([T, 2, 2]), obs, rewards (shared), individual rewards, dones, pos, comm; obs_dim, share_obs_dim,
action_dims.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402
from make_golden_mpe import _stub_modules  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEEDS = (3, 17, 2024)
T = 25


def main():
    _stub_modules()
    ref_import.load_reference()
    envs = types.ModuleType("onpolicy.envs")     # (skip onpolicy/envs/__init__.py: absl flags for SMAC)
    envs.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "onpolicy", "envs")]
    sys.modules["onpolicy.envs"] = envs
    from onpolicy.envs.mpe.MPE_env import MPEEnv          # the reference's
    out = {}
    for ci, seed in enumerate(SEEDS):
        args = types.SimpleNamespace(scenario_name="simple_reference", num_agents=2, num_landmarks=3, episode_length=T)
        env = MPEEnv(args)
        env.seed(seed)
        obs0 = np.array(env.reset())
        w = env.world
        key = "ref%d_" % ci
        dims = env.action_space[0].high - env.action_space[0].low + 1
        out[key + "pos0"] = np.array([a.state.p_pos for a in w.agents])
        out[key + "vel0"] = np.array([a.state.p_vel for a in w.agents])
        out[key + "landmarks"] = np.array([l.state.p_pos for l in w.landmarks])
        out[key + "goals"] = np.array([w.landmarks.index(a.goal_b) for a in w.agents], dtype=np.int64)
        out[key + "obs0"] = obs0
        rng = np.random.default_rng(seed)
        rec = {k: [] for k in ("actions", "action_idx", "obs", "rewards", "individual_rewards", "dones", "pos", "comm")}
        for _ in range(T):
            idx = np.stack([rng.integers(0, int(d), 2) for d in dims], -1)                  # [agents, heads]
            onehot = np.concatenate([np.eye(int(d))[idx[:, k]] for k, d in enumerate(dims)], -1)
            obs, rew, done, info = env.step(list(onehot))
            rec["actions"].append(onehot)
            rec["action_idx"].append(idx)
            rec["obs"].append(np.array(obs))
            rec["rewards"].append(np.array(rew, dtype=np.float64))
            rec["individual_rewards"].append(np.array([i["individual_reward"] for i in info], dtype=np.float64))
            rec["dones"].append(np.array(done))
            rec["pos"].append(np.array([a.state.p_pos for a in w.agents]))
            rec["comm"].append(np.array([a.state.c for a in w.agents]))
        for k, v in rec.items():
            out[key + k] = np.array(v)
        out[key + "obs_dim"] = np.array(env.observation_space[0].shape)
        out[key + "share_obs_dim"] = np.array(env.share_observation_space[0].shape)
        out[key + "action_dims"] = np.array(dims, dtype=np.int64)
    path = os.path.join(GOLD, "mpe_reference_cases.npz")
    np.savez_compressed(path, **out)
    print("mpe_reference_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))
    print("case 0: goals", out["ref0_goals"], "obs", out["ref0_obs"].shape, "rewards[0]", out["ref0_rewards"][0].ravel())


if __name__ == "__main__":
    main()
