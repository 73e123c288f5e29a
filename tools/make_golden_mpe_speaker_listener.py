#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/mpe_speaker_listener_cases.npz by stepping the REFERENCE's multi-agent
particle environment for the ``simple_speaker_listener`` scenario (onpolicy/envs/mpe: core.py physics and communication
state, environment.py action decoding, scenarios/simple_speaker_listener.py goal / reward / observation) from seeded
initial states with seeded one-hot actions: one 25-step episode per seed.  Needs the reference tree
(oracle/ref_import.py); gym and seaborn are stubbed for the import as in oracle/make_golden_mpe.py.

    python tools/make_golden_mpe_speaker_listener.py

Per case ``spk<i>_``: post-reset pos0 / vel0 / landmarks / goal / obs0_speaker / obs0_listener, per step action_idx
([T, 2]: the speaker's symbol, the listener's movement), obs_speaker [T, 3], obs_listener [T, 11], rewards (shared),
individual rewards, dones, pos, comm (the speaker's state.c); obs_dims, share_obs_dim, action_dims.
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
        args = types.SimpleNamespace(scenario_name="simple_speaker_listener", num_agents=2, num_landmarks=3,
                                     episode_length=T)
        env = MPEEnv(args)
        env.seed(seed)
        obs0 = env.reset()
        w = env.world
        key = "spk%d_" % ci
        dims = [int(sp.n) for sp in env.action_space]                   # Discrete(3), Discrete(5)
        out[key + "pos0"] = np.array([a.state.p_pos for a in w.agents])
        out[key + "vel0"] = np.array([a.state.p_vel for a in w.agents])
        out[key + "landmarks"] = np.array([l.state.p_pos for l in w.landmarks])
        out[key + "goal"] = np.array(w.landmarks.index(w.agents[0].goal_b), dtype=np.int64)
        out[key + "obs0_speaker"] = np.array(obs0[0], dtype=np.float64)
        out[key + "obs0_listener"] = np.array(obs0[1], dtype=np.float64)
        rng = np.random.default_rng(seed)
        rec = {k: [] for k in ("action_idx", "obs_speaker", "obs_listener", "rewards", "individual_rewards", "dones",
                               "pos", "comm")}
        for _ in range(T):
            idx = np.array([rng.integers(0, d) for d in dims], dtype=np.int64)              # [agents]
            obs, rew, done, info = env.step([np.eye(d)[i] for d, i in zip(dims, idx)])
            rec["action_idx"].append(idx)
            rec["obs_speaker"].append(np.array(obs[0], dtype=np.float64))
            rec["obs_listener"].append(np.array(obs[1], dtype=np.float64))
            rec["rewards"].append(np.array(rew, dtype=np.float64))
            rec["individual_rewards"].append(np.array([i["individual_reward"] for i in info], dtype=np.float64))
            rec["dones"].append(np.array(done))
            rec["pos"].append(np.array([a.state.p_pos for a in w.agents]))
            rec["comm"].append(np.array(w.agents[0].state.c, dtype=np.float64))
        for k, v in rec.items():
            out[key + k] = np.array(v)
        out[key + "obs_dims"] = np.array([sp.shape[0] for sp in env.observation_space], dtype=np.int64)
        out[key + "share_obs_dim"] = np.array(env.share_observation_space[0].shape)
        out[key + "action_dims"] = np.array(dims, dtype=np.int64)
    path = os.path.join(GOLD, "mpe_speaker_listener_cases.npz")
    np.savez_compressed(path, **out)
    print("mpe_speaker_listener_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))
    for k in sorted(out):
        if k.startswith("spk0_"):
            print(k, out[k].shape, out[k].dtype)
    print("case 0: goal", out["spk0_goal"], "rewards[0]", out["spk0_rewards"][0].ravel(), "pos[-1]", out["spk0_pos"][-1])


if __name__ == "__main__":
    main()
