#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/mpe_push_cases.npz by stepping the REFERENCE's multi-agent particle
environment for the ``simple_push`` scenario (onpolicy/envs/mpe: core.py physics and contact forces, environment.py
action decoding and per-agent rewards, scenarios/simple_push.py goal / reward / observation) from seeded initial states:
one 25-step episode per case.  Needs the reference tree (oracle/ref_import.py); gym and seaborn are stubbed for the
import as in oracle/make_golden_mpe.py.

    python tools/make_golden_mpe_push.py

Free-play cases take seeded random one-hot actions.  Random play never brings agents of radius 0.05 into contact, so the
contact cases place agent 1 at agent 0 + (0.06, 0.01) after the reset (and, with three agents, agent 2 next to agent 1)
and drive the pair into each other; the tool asserts that each of them has at least 3 steps that start with a pair closer
than 0.1, so that the contact force acts in them.

Per case ``push<i>_``: dims (A, L), post-reset pos0 / vel0 / landmarks / goal / obs0_<agent>, per step action_idx
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
# (agents, landmarks, seed, contact)
CASES = ((2, 2, 3, False), (2, 2, 17, False), (3, 2, 2024, False), (4, 1, 5, False), (2, 2, 11, True), (3, 2, 23, True))
CONTACT_STEPS = 3           # at least this many steps of a contact case start with a pair closer than 0.1


def _closest_pair(pos):
    d = np.sqrt(((pos[:, None] - pos[None]) ** 2).sum(-1))
    return float(d[~np.eye(len(pos), dtype=bool)].min())


def main():
    _stub_modules()
    ref_import.load_reference()
    envs = types.ModuleType("onpolicy.envs")     # (skip onpolicy/envs/__init__.py: absl flags for SMAC)
    envs.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "onpolicy", "envs")]
    sys.modules["onpolicy.envs"] = envs
    from onpolicy.envs.mpe.MPE_env import MPEEnv          # the reference's
    out = {}
    for ci, (A, L, seed, contact) in enumerate(CASES):
        args = types.SimpleNamespace(scenario_name="simple_push", num_agents=A, num_landmarks=L, episode_length=T)
        env = MPEEnv(args)
        env.seed(seed)
        obs0 = env.reset()
        w = env.world
        if contact:
            w.agents[1].state.p_pos = w.agents[0].state.p_pos + np.array([0.06, 0.01])
            if A > 2:
                w.agents[2].state.p_pos = w.agents[1].state.p_pos + np.array([0.01, 0.07])
            obs0 = [env._get_obs(agent) for agent in w.agents]
        key = "push%d_" % ci
        dims = [int(sp.n) for sp in env.action_space]                   # Discrete(5) each
        out[key + "dims"] = np.array([A, L], dtype=np.int64)
        out[key + "pos0"] = np.array([a.state.p_pos for a in w.agents])
        out[key + "vel0"] = np.array([a.state.p_vel for a in w.agents])
        out[key + "landmarks"] = np.array([l.state.p_pos for l in w.landmarks])
        out[key + "goal"] = np.array(w.landmarks.index(w.agents[0].goal_a), dtype=np.int64)
        for i in range(A):
            out[key + "obs0_%d" % i] = np.array(obs0[i], dtype=np.float64)
        rng = np.random.default_rng(seed)
        rec = {k: [] for k in ["action_idx", "rewards", "individual_rewards", "dones", "pos", "vel"]
               + ["obs_%d" % i for i in range(A)]}
        touching = 0
        for _ in range(T):
            idx = np.array([rng.integers(0, d) for d in dims], dtype=np.int64)              # [agents]
            if contact:                 # agent 0 to the right, agent 1 to the left: into each other; a third one downwards
                idx[0], idx[1] = 1, 2
                if A > 2:
                    idx[2] = 4
            touching += _closest_pair(np.array([a.state.p_pos for a in w.agents])) < 0.1      # the contact force acts
            obs, rew, done, info = env.step([np.eye(d)[i] for d, i in zip(dims, idx)])
            rec["action_idx"].append(idx)
            for i in range(A):
                rec["obs_%d" % i].append(np.array(obs[i], dtype=np.float64))
            rec["rewards"].append(np.array(rew, dtype=np.float64))
            rec["individual_rewards"].append(np.array([i["individual_reward"] for i in info], dtype=np.float64))
            rec["dones"].append(np.array(done))
            rec["pos"].append(np.array([a.state.p_pos for a in w.agents]))
            rec["vel"].append(np.array([a.state.p_vel for a in w.agents]))
        assert touching >= CONTACT_STEPS if contact else True, (ci, touching)
        for k, v in rec.items():
            out[key + k] = np.array(v)
        out[key + "obs_dims"] = np.array([sp.shape[0] for sp in env.observation_space], dtype=np.int64)
        out[key + "share_obs_dim"] = np.array(env.share_observation_space[0].shape)
        out[key + "action_dims"] = np.array(dims, dtype=np.int64)
        print("case %d: A=%d L=%d goal %d obs_dims %s steps in contact %d rewards[0] %s" % (
            ci, A, L, out[key + "goal"], out[key + "obs_dims"], touching, out[key + "rewards"][0].ravel()))
    path = os.path.join(GOLD, "mpe_push_cases.npz")
    np.savez_compressed(path, **out)
    print("mpe_push_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
