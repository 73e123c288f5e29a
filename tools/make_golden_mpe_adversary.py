#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/mpe_adversary_cases.npz by stepping the REFERENCE's multi-agent particle
environment for the ``simple_adversary`` scenario (onpolicy/envs/mpe: core.py physics, environment.py action decoding and
per-agent rewards, scenarios/simple_adversary.py goal / reward / observation) from seeded initial states: one 25-step
episode per case.  Needs the reference tree (oracle/ref_import.py); gym and seaborn are stubbed for the import as in
oracle/make_golden_mpe.py.

    python tools/make_golden_mpe_adversary.py

Free-play cases take seeded random one-hot actions.  The ``cover`` case puts good agent 1 at the goal + (0.3, 0.2) after
the reset and steers it onto the goal, while the adversary is steered away from it: the good agents' reward, d_0 - min
d_g, is positive there.  The ``found`` case puts the adversary on the goal and lets it rest: d_0 = 0 and the good agents'
reward is negative.  The tool asserts both signs, and that in some case the good agent nearest to the goal changes.

Per case ``adv<i>_``: dims (A, L), post-reset pos0 / vel0 / landmarks / goal / obs0_<agent>, per step action_idx
[T, A], obs_<agent> [T, D_agent], rewards [T, A, 1], individual_rewards [T, A], dones [T, A], pos and vel [T, A, 2];
obs_dims, share_obs_dim, action_dims.
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
T = 25
# (agents, seed, kind)
CASES = ((3, 3, "free"), (3, 17, "free"), (2, 2024, "free"), (5, 5, "free"), (3, 11, "cover"), (3, 23, "found"))


def _towards(x, target):
    """The movement index that takes ``x`` towards ``target`` along the axis on which it is further away."""
    dx, dy = target - x
    if abs(dx) >= abs(dy):
        return 1 if dx > 0 else 2
    return 3 if dy > 0 else 4


def main():
    _stub_modules()
    ref_import.load_reference()
    envs = types.ModuleType("onpolicy.envs")     # (skip onpolicy/envs/__init__.py: absl flags for SMAC)
    envs.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "onpolicy", "envs")]
    sys.modules["onpolicy.envs"] = envs
    from onpolicy.envs.mpe.MPE_env import MPEEnv          # the reference's
    out = {}
    changes_hands = 0
    for ci, (A, seed, kind) in enumerate(CASES):
        # (num_landmarks: the scenario ignores it and builds A - 1)
        args = types.SimpleNamespace(scenario_name="simple_adversary", num_agents=A, num_landmarks=3, episode_length=T)
        env = MPEEnv(args)
        env.seed(seed)
        obs0 = env.reset()
        w = env.world
        goal = w.agents[0].goal_a
        if kind == "cover":
            w.agents[1].state.p_pos = goal.state.p_pos + np.array([0.3, 0.2])
        if kind == "found":
            w.agents[0].state.p_pos = goal.state.p_pos.copy()
        if kind != "free":
            obs0 = [env._get_obs(agent) for agent in w.agents]
        key = "adv%d_" % ci
        L = len(w.landmarks)
        dims = [int(sp.n) for sp in env.action_space]                   # Discrete(5) each
        out[key + "dims"] = np.array([A, L], dtype=np.int64)
        out[key + "pos0"] = np.array([a.state.p_pos for a in w.agents])
        out[key + "vel0"] = np.array([a.state.p_vel for a in w.agents])
        out[key + "landmarks"] = np.array([l.state.p_pos for l in w.landmarks])
        out[key + "goal"] = np.array(w.landmarks.index(goal), dtype=np.int64)
        for i in range(A):
            out[key + "obs0_%d" % i] = np.array(obs0[i], dtype=np.float64)
        rng = np.random.default_rng(seed)
        rec = {k: [] for k in ["action_idx", "rewards", "individual_rewards", "dones", "pos", "vel"]
               + ["obs_%d" % i for i in range(A)]}
        nearest = []
        for _ in range(T):
            idx = np.array([rng.integers(0, d) for d in dims], dtype=np.int64)              # [agents]
            if kind == "cover":         # the adversary away from the goal, agent 1 onto it
                away = 2 * w.agents[0].state.p_pos - goal.state.p_pos
                idx[0] = _towards(w.agents[0].state.p_pos, away)
                idx[1] = _towards(w.agents[1].state.p_pos, goal.state.p_pos)
            if kind == "found":         # the adversary rests on the goal
                idx[0] = 0
            obs, rew, done, info = env.step([np.eye(d)[i] for d, i in zip(dims, idx)])
            rec["action_idx"].append(idx)
            for i in range(A):
                rec["obs_%d" % i].append(np.array(obs[i], dtype=np.float64))
            rec["rewards"].append(np.array(rew, dtype=np.float64))
            rec["individual_rewards"].append(np.array([i["individual_reward"] for i in info], dtype=np.float64))
            rec["dones"].append(np.array(done))
            rec["pos"].append(np.array([a.state.p_pos for a in w.agents]))
            rec["vel"].append(np.array([a.state.p_vel for a in w.agents]))
            d = np.sqrt(((rec["pos"][-1] - goal.state.p_pos) ** 2).sum(-1))
            nearest.append(1 + int(d[1:].argmin()))
        for k, v in rec.items():
            out[key + k] = np.array(v)
        good = out[key + "rewards"][:, 1, 0]
        if kind == "cover":
            assert (good[5:] > 0).all(), good
        if kind == "found":
            assert (good < 0).all() and (out[key + "rewards"][:, 0, 0] == 0).all(), out[key + "rewards"][..., 0]
        changes_hands += len(set(nearest)) > 1
        out[key + "obs_dims"] = np.array([sp.shape[0] for sp in env.observation_space], dtype=np.int64)
        out[key + "share_obs_dim"] = np.array(env.share_observation_space[0].shape)
        out[key + "action_dims"] = np.array(dims, dtype=np.int64)
        print("case %d (%s): A=%d L=%d goal %d obs_dims %s nearest good agent %s rewards[0] %s rewards[-1] %s" % (
            ci, kind, A, L, out[key + "goal"], out[key + "obs_dims"], sorted(set(nearest)),
            out[key + "rewards"][0].ravel(), out[key + "rewards"][-1].ravel()))
    assert changes_hands >= 1, "no case in which the nearest good agent changes"
    path = os.path.join(GOLD, "mpe_adversary_cases.npz")
    np.savez_compressed(path, **out)
    print("mpe_adversary_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
