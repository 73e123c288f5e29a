#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/mpe_tag_cases.npz by stepping the REFERENCE's multi-agent particle
environment for the ``simple_tag`` scenario (onpolicy/envs/mpe: core.py physics with top speeds and contact forces between
agents and between agents and landmarks, environment.py action decoding and per-agent rewards, scenarios/simple_tag.py
constants / reward / observation) from seeded initial states: one 25-step episode per case.  Needs the reference tree
(oracle/ref_import.py); gym and seaborn are stubbed for the import as in oracle/make_golden_mpe.py.

    python tools/make_golden_mpe_tag.py

Free-play cases take seeded random one-hot actions: they clamp the speed in most steps, now and then touch a landmark
and seldom produce a catch.  The designed cases place the entities after the reset and script some agents (the others
keep their random actions); each carries an assertion below:

  catch     an adversary 0.1 from a good agent, each driven at the other along x: at least CONTACT_STEPS steps begin with
            the pair closer than 0.125, and at least one step pays +10 / -10
  landmark  an adversary 0.22 from a landmark's centre, driven into it: at least CONTACT_STEPS steps begin with it closer
            than 0.275
  bound     a good agent at x = 0.85 driven outward, through the ramp of the boundary penalty (0.9, 1.0) into its exp
            branch, and a second good agent at y = 2.3, where the penalty is capped at 10

No (good agent, adversary) distance of any recorded step lies within THRESHOLD_MARGIN of 0.125, so whether a pair
touches is never a rounding question in a replay.

Per case ``tag<i>_``: dims (A, L), num_adversaries, post-reset pos0 / vel0 / landmarks / obs0_<agent>, per step
action_idx [T, A], obs_<agent> [T, D_agent], rewards [T, A, 1], individual_rewards [T, A], dones [T, A], pos and vel
[T, A, 2]; obs_dims, share_obs_dim, action_dims.
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
# (adversaries, good agents, landmarks, seed, design)
CASES = ((3, 1, 2, 3, None), (2, 2, 2, 2024, None), (1, 1, 1, 5, None),
         (3, 1, 2, 11, "catch"), (2, 2, 2, 23, "landmark"), (1, 2, 1, 29, "bound"))
CONTACT_STEPS = 3           # at least this many steps of a contact case start with the pair inside its dist_min
THRESHOLD_MARGIN = 1e-6
CATCH = 0.05 + 0.075        # a good agent's radius + an adversary's
LANDMARK = 0.2


def _design(design, w, adv):
    """Places the entities of a designed case; -> {agent: scripted action index, or a function that returns it}."""
    agents, landmarks = w.agents, w.landmarks
    if design == "catch":           # adversary 0 and the good agent face each other, everything else out of the way
        for l, x in zip(landmarks, (-0.7, 0.7)):
            l.state.p_pos = np.array([x, -0.7])
        agents[0].state.p_pos = np.array([-0.05, 0.3])
        agents[adv].state.p_pos = np.array([0.05, 0.3])
        agents[1].state.p_pos = np.array([-0.6, 0.8])
        agents[2].state.p_pos = np.array([0.6, 0.8])
        # each of the pair drives at the other along x, on whichever side it is: they cross and turn around
        def at(me, other):
            return lambda: 1 if agents[other].state.p_pos[0] > agents[me].state.p_pos[0] else 2
        return {0: at(0, adv), adv: at(adv, 0)}
    if design == "landmark":        # adversary 0 to the right of landmark 0, driven to the left
        landmarks[0].state.p_pos = np.array([-0.3, 0.1])
        landmarks[1].state.p_pos = np.array([0.6, -0.6])
        agents[0].state.p_pos = landmarks[0].state.p_pos + np.array([0.22, 0.0])
        agents[1].state.p_pos = np.array([0.7, 0.7])
        agents[2].state.p_pos = np.array([-0.8, -0.7])
        agents[3].state.p_pos = np.array([0.1, -0.8])
        return {0: 2}
    assert design == "bound"        # good agent 1 leaves to the right, good agent 2 is far above the screen
    landmarks[0].state.p_pos = np.array([-0.5, -0.5])
    agents[0].state.p_pos = np.array([-0.6, 0.5])
    agents[1].state.p_pos = np.array([0.85, 0.0])
    agents[2].state.p_pos = np.array([0.0, 2.3])
    return {1: 1, 2: 3}


def bound(x):
    return 0.0 if x < 0.9 else (x - 0.9) * 10 if x < 1.0 else min(np.exp(2 * x - 2), 10)


def main():
    _stub_modules()
    ref_import.load_reference()
    envs = types.ModuleType("onpolicy.envs")     # (skip onpolicy/envs/__init__.py: absl flags for SMAC)
    envs.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "onpolicy", "envs")]
    sys.modules["onpolicy.envs"] = envs
    from onpolicy.envs.mpe.MPE_env import MPEEnv          # the reference's
    out = {}
    for ci, (adv, good, L, seed, design) in enumerate(CASES):
        A = adv + good
        args = types.SimpleNamespace(scenario_name="simple_tag", num_agents=A, num_adversaries=adv,
                                     num_good_agents=good, num_landmarks=L, episode_length=T)
        env = MPEEnv(args)
        env.seed(seed)
        obs0 = env.reset()
        w = env.world
        scripted = {}
        if design:
            scripted = _design(design, w, adv)
            obs0 = [env._get_obs(agent) for agent in w.agents]
        key = "tag%d_" % ci
        dims = [int(sp.n) for sp in env.action_space]                   # Discrete(5) each
        out[key + "dims"] = np.array([A, L], dtype=np.int64)
        out[key + "num_adversaries"] = np.array(adv, dtype=np.int64)
        out[key + "pos0"] = np.array([a.state.p_pos for a in w.agents])
        out[key + "vel0"] = np.array([a.state.p_vel for a in w.agents])
        out[key + "landmarks"] = np.array([l.state.p_pos for l in w.landmarks])
        for i in range(A):
            out[key + "obs0_%d" % i] = np.array(obs0[i], dtype=np.float64)
        rng = np.random.default_rng(seed)
        rec = {k: [] for k in ["action_idx", "rewards", "individual_rewards", "dones", "pos", "vel"]
               + ["obs_%d" % i for i in range(A)]}
        pair_steps = landmark_steps = catches = clamped = touched = 0
        margin = np.inf
        ramp = exp = capped = False

        def pair_dist():
            pos = np.array([a.state.p_pos for a in w.agents])
            return np.sqrt(((pos[adv:, None] - pos[None, :adv]) ** 2).sum(-1))          # [good, adversaries]
        margin = min(margin, float(np.abs(pair_dist() - CATCH).min()))
        for _ in range(T):
            idx = np.array([rng.integers(0, d) for d in dims], dtype=np.int64)              # [agents]
            for i, move in scripted.items():
                idx[i] = move() if callable(move) else move
            pos = np.array([a.state.p_pos for a in w.agents])
            land = np.array([l.state.p_pos for l in w.landmarks])
            to_land = np.sqrt(((pos[:, None] - land[None]) ** 2).sum(-1))                   # [agents, landmarks]
            size = np.array([a.size for a in w.agents])
            pair_steps += pair_dist()[0, 0] < CATCH
            landmark_steps += to_land[0, 0] < size[0] + LANDMARK
            touched += bool((to_land < size[:, None] + LANDMARK).any())
            obs, rew, done, info = env.step([np.eye(d)[i] for d, i in zip(dims, idx)])
            rec["action_idx"].append(idx)
            for i in range(A):
                rec["obs_%d" % i].append(np.array(obs[i], dtype=np.float64))
            rec["rewards"].append(np.array(rew, dtype=np.float64))
            rec["individual_rewards"].append(np.array([i["individual_reward"] for i in info], dtype=np.float64))
            rec["dones"].append(np.array(done))
            rec["pos"].append(np.array([a.state.p_pos for a in w.agents]))
            rec["vel"].append(np.array([a.state.p_vel for a in w.agents]))
            d = pair_dist()
            margin = min(margin, float(np.abs(d - CATCH).min()))
            hits = int((d < CATCH).sum())
            catches += hits
            if hits:
                assert rec["rewards"][-1][0, 0] == 10 * hits and rec["rewards"][-1][adv:, 0].min() <= -10
            speed = np.sqrt((rec["vel"][-1] ** 2).sum(-1))
            clamped += bool((np.abs(speed - np.array([a.max_speed for a in w.agents])) < 1e-12).any())
            for a in w.agents[adv:]:
                for x in np.abs(a.state.p_pos):
                    ramp, exp, capped = ramp or 0.9 < x < 1.0, exp or (x >= 1.0 and bound(x) < 10), capped or bound(x) == 10
        assert margin > THRESHOLD_MARGIN, (ci, margin)
        if design == "catch":
            assert pair_steps >= CONTACT_STEPS and catches >= 1, (ci, pair_steps, catches)
        if design == "landmark":
            assert landmark_steps >= CONTACT_STEPS, (ci, landmark_steps)
        if design == "bound":
            assert ramp and exp and capped, (ci, ramp, exp, capped)
        for k, v in rec.items():
            out[key + k] = np.array(v)
        out[key + "obs_dims"] = np.array([sp.shape[0] for sp in env.observation_space], dtype=np.int64)
        out[key + "share_obs_dim"] = np.array(env.share_observation_space[0].shape)
        out[key + "action_dims"] = np.array(dims, dtype=np.int64)
        print("case %d (%s): adv=%d good=%d L=%d obs_dims %s catches %d steps clamped %d touching a landmark %d "
              "pair / landmark contact steps %d / %d margin %.3g" % (
                  ci, design or "free play", adv, good, L, out[key + "obs_dims"], catches, clamped, touched, pair_steps,
                  landmark_steps, margin))
    path = os.path.join(GOLD, "mpe_tag_cases.npz")
    np.savez_compressed(path, **out)
    print("mpe_tag_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
