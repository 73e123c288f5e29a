#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/mpe_world_comm_cases.npz by stepping the REFERENCE's multi-agent particle
environment for the ``simple_world_comm`` scenario (onpolicy/envs/mpe: core.py physics with top speeds, contact forces and
the communication state, environment.py MultiDiscrete / Discrete action decoding and per-agent rewards,
scenarios/simple_world_comm.py constants / reward / observation with its forests) from seeded initial states: one 25-step
episode per case.  Needs the reference tree (oracle/ref_import.py); gym and seaborn are stubbed for the import as in
oracle/make_golden_mpe.py.

    python tools/make_golden_mpe_world_comm.py

Every agent takes seeded random actions, the leader (agent 0) a movement and a word: its action is the 9-wide
concatenation of two one-hots.  The free-play cases run at (adversaries, good agents, obstacles) = (4, 2, 1), (2, 1, 2)
and (1, 1, 1).  The designed cases place the entities after the reset and script some agents (the others keep their
random actions); each carries an assertion below:

  forest    good agent Nadv at rest inside forest 0, adversary 1 (not the leader) in the open, driven into the forest and
            out at its far side, where forest 1 waits: some steps hide the good agent from adversary 1 and not from the
            leader, later steps show it; in some step the observer is in a forest and the other in the open, in some step
            the two are in different forests
  food      a good agent driven across a food: at least 3 steps pay the +2
  catch     an adversary 0.1 from a good agent, each driven at the other along x: at least one step pays +5 to every
            adversary and -5 to the good agent
  speak     the leader's word cycles 0, 1, 2, 3: every adversary's last four columns show it in the same step, obs0's last
            four columns are zero
  bound     a good agent at x = 0.85 driven outward, through the ramp of the boundary penalty (0.9, 1.0) into its exp
            branch, and a second good agent at y = 2.3, where the penalty is capped at 10; paid doubled

Over every recorded step of every case (the post-reset state included) no agent-forest distance lies within
THRESHOLD_MARGIN of its threshold (0.375 / 0.345), no good-food distance within it of 0.075 and no good-adversary distance
within it of 0.12, so whether a pair touches, eats or hides is never a rounding question in a replay.

Per case ``wc<i>_``: dims (A, L: obstacles), num_adversaries, post-reset pos0 / vel0 / landmarks [L + 4, 2] /
obs0_<agent>, per step action_idx [T, A + 1] (the leader's movement, its word, the others' movements), obs_<agent>
[T, D_agent], rewards [T, A, 1], individual_rewards [T, A], dones [T, A], pos and vel [T, A, 2], comm [T, 4]; obs_dims,
share_obs_dim, action_dims (the width of every agent's one-hot action).
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
# (adversaries, good agents, obstacles, seed, design)
CASES = ((4, 2, 1, 3, None), (2, 1, 2, 2024, None), (1, 1, 1, 5, None),
         (2, 1, 1, 11, "forest"), (1, 2, 1, 23, "food"), (3, 1, 2, 29, "catch"), (3, 1, 1, 31, "speak"),
         (1, 2, 1, 37, "bound"))
THRESHOLD_MARGIN = 1e-6
SIZE = (0.075, 0.045)       # adversary, good agent
CATCH = SIZE[1] + SIZE[0]
FOOD = SIZE[1] + 0.03
FOREST = 0.3
FAR = np.array([5.0, 5.0])


def _design(design, w, adv, L):
    """Places the entities of a designed case; -> {action column: scripted index, or a function that returns it}.
    Columns: 0 the leader's movement, 1 its word, i + 1 agent i's movement."""
    agents, landmarks = w.agents, w.landmarks
    obstacles, food, forests = landmarks[:L], landmarks[L:L + 2], landmarks[L + 2:]
    for k, l in enumerate(obstacles):           # out of everybody's way unless the case says otherwise
        l.state.p_pos = np.array([-0.8 + 0.3 * k, -0.85])
    if design == "forest":
        # forests 0.62 apart along x: their discs overlap for nobody (0.375 + 0.375 > 0.62 only between 0.245 and 0.375)
        forests[0].state.p_pos = np.array([0.0, 0.3])
        forests[1].state.p_pos = np.array([0.72, 0.3])
        food[0].state.p_pos = np.array([-0.7, 0.7])
        food[1].state.p_pos = np.array([0.7, -0.7])
        agents[0].state.p_pos = np.array([-0.7, -0.4])           # the leader, in the open
        agents[1].state.p_pos = np.array([-0.62, 0.3])           # adversary 1 outside forest 0, driven to the right
        agents[adv].state.p_pos = np.array([0.1, 0.45])          # the good agent inside forest 0, at rest, off the path
        return {2: 1, adv + 1: 0}
    if design == "food":
        food[0].state.p_pos = np.array([0.0, 0.2])
        food[1].state.p_pos = np.array([0.6, -0.6])
        forests[0].state.p_pos = np.array([-0.6, 0.7])
        forests[1].state.p_pos = np.array([0.7, 0.7])
        agents[0].state.p_pos = np.array([-0.7, -0.5])
        agents[adv].state.p_pos = np.array([-0.06, 0.2])         # left of food 0, hovering about it
        agents[adv + 1].state.p_pos = np.array([0.3, 0.75])

        def hover():
            return 1 if agents[adv].state.p_pos[0] < food[0].state.p_pos[0] else 2
        return {adv + 1: hover}
    if design == "catch":           # adversary 0 and the good agent face each other, everything else out of the way
        forests[0].state.p_pos = np.array([-0.7, -0.3])
        forests[1].state.p_pos = np.array([0.7, -0.3])
        food[0].state.p_pos = np.array([-0.2, 0.8])
        food[1].state.p_pos = np.array([0.2, -0.5])
        agents[0].state.p_pos = np.array([-0.05, 0.3])
        agents[adv].state.p_pos = np.array([0.05, 0.3])
        agents[1].state.p_pos = np.array([-0.6, 0.8])
        agents[2].state.p_pos = np.array([0.6, 0.8])

        def at(me, other):
            return lambda: 1 if agents[other].state.p_pos[0] > agents[me].state.p_pos[0] else 2
        return {0: at(0, adv), adv + 1: at(adv, 0)}
    if design == "speak":
        step = [0]

        def word():
            step[0] += 1
            return (step[0] - 1) % 4
        return {1: word}
    assert design == "bound"        # good agent 1 leaves to the right, good agent 2 is far above the screen
    forests[0].state.p_pos = np.array([-0.6, -0.3])
    forests[1].state.p_pos = np.array([-0.6, 0.6])
    food[0].state.p_pos = np.array([0.1, -0.6])
    food[1].state.p_pos = np.array([0.3, 0.4])
    agents[0].state.p_pos = np.array([-0.1, 0.5])
    agents[1].state.p_pos = np.array([0.85, 0.0])
    agents[2].state.p_pos = np.array([0.0, 2.3])
    return {2: 1, 3: 3}


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
        args = types.SimpleNamespace(scenario_name="simple_world_comm", num_agents=A, num_adversaries=adv,
                                     num_good_agents=good, num_landmarks=L, episode_length=T)
        env = MPEEnv(args)
        env.seed(seed)
        obs0 = env.reset()
        w = env.world
        scripted = {}
        if design:
            scripted = _design(design, w, adv, L)
            obs0 = [env._get_obs(agent) for agent in w.agents]
        key = "wc%d_" % ci
        assert type(env.action_space[0]).__name__ == "MultiDiscrete"
        assert list(env.action_space[0].high - env.action_space[0].low + 1) == [5, 4]
        widths = [9] + [int(sp.n) for sp in env.action_space[1:]]       # one-hot width per agent
        heads = [5, 4] + widths[1:]                                     # one head per action column
        out[key + "dims"] = np.array([A, L], dtype=np.int64)
        out[key + "num_adversaries"] = np.array(adv, dtype=np.int64)
        out[key + "pos0"] = np.array([a.state.p_pos for a in w.agents])
        out[key + "vel0"] = np.array([a.state.p_vel for a in w.agents])
        out[key + "landmarks"] = np.array([l.state.p_pos for l in w.landmarks])
        assert out[key + "landmarks"].shape == (L + 4, 2)
        for i in range(A):
            out[key + "obs0_%d" % i] = np.array(obs0[i], dtype=np.float64)
            if i < adv:
                assert not out[key + "obs0_%d" % i][-4:].any()
        rng = np.random.default_rng(seed)
        rec = {k: [] for k in ["action_idx", "rewards", "individual_rewards", "dones", "pos", "vel", "comm"]
               + ["obs_%d" % i for i in range(A)]}
        size = np.array([a.size for a in w.agents])
        assert list(size) == [SIZE[0]] * adv + [SIZE[1]] * good
        land = np.array([l.state.p_pos for l in w.landmarks])
        seen = dict(catches=0, fed=0, hidden=0, hidden_from_1=0, shown_after=0, different=0, observer_in=0, clamped=0)
        margin = np.inf
        ramp = exp = capped = False

        def geometry():
            pos = np.array([a.state.p_pos for a in w.agents])
            pair = np.sqrt(((pos[adv:, None] - pos[None, :adv]) ** 2).sum(-1))              # [good, adversaries]
            food = np.sqrt(((pos[adv:, None] - land[None, L:L + 2]) ** 2).sum(-1))          # [good, food]
            forest = np.sqrt(((pos[:, None] - land[None, L + 2:]) ** 2).sum(-1))            # [agents, forests]
            m = min(np.abs(pair - CATCH).min(), np.abs(food - FOOD).min(),
                    np.abs(forest - (size[:, None] + FOREST)).min())
            return pair, food, forest < size[:, None] + FOREST, float(m)
        margin = min(margin, geometry()[3])
        for t in range(T):
            idx = np.array([rng.integers(0, d) for d in heads], dtype=np.int64)             # [A + 1]
            for col, move in scripted.items():
                idx[col] = move() if callable(move) else move
            one_hot = [np.concatenate([np.eye(5)[idx[0]], np.eye(4)[idx[1]]])] + [np.eye(5)[i] for i in idx[2:]]
            obs, rew, done, info = env.step(one_hot)
            rec["action_idx"].append(idx)
            for i in range(A):
                rec["obs_%d" % i].append(np.array(obs[i], dtype=np.float64))
            rec["rewards"].append(np.array(rew, dtype=np.float64))
            rec["individual_rewards"].append(np.array([i["individual_reward"] for i in info], dtype=np.float64))
            rec["dones"].append(np.array(done))
            rec["pos"].append(np.array([a.state.p_pos for a in w.agents]))
            rec["vel"].append(np.array([a.state.p_vel for a in w.agents]))
            rec["comm"].append(np.array(w.agents[0].state.c, dtype=np.float64))
            assert np.array_equal(rec["comm"][-1], np.eye(4)[idx[1]])
            for i in range(adv):            # every adversary hears the word in the step it is said
                assert np.array_equal(rec["obs_%d" % i][-1][-4:], rec["comm"][-1])
            pair, food, inside, m = geometry()
            margin = min(margin, m)
            r = rec["rewards"][-1][:, 0]
            hits = int((pair < CATCH).sum())
            seen["catches"] += hits
            if hits:
                want = 5 * hits - 0.1 * pair.min(0)
                assert np.allclose(r[:adv], want, rtol=0, atol=1e-12) and r[adv:].min() < -4.0
            fed = (food < FOOD).sum(1)
            seen["fed"] += int(fed[0] > 0)
            for g in range(good):
                p = rec["pos"][-1][adv + g]
                want = (-5 * (pair[g] < CATCH).sum() - 2 * (bound(abs(p[0])) + bound(abs(p[1]))) + 2 * fed[g]
                        + 0.05 * food[g].min())
                assert abs(r[adv + g] - want) < 1e-12, (ci, t, g, r[adv + g], want)
                for x in np.abs(p):
                    ramp, exp, capped = ramp or 0.9 < x < 1.0, exp or (x >= 1.0 and bound(x) < 10), capped or bound(x) == 10
            # who sees whom, from the positions; the recorded observations must agree
            free = ~inside.any(1)
            vis = (inside[:, None, 0] & inside[None, :, 0]) | (inside[:, None, 1] & inside[None, :, 1]) \
                | (free[:, None] & free[None, :])
            vis[0] = True
            lo = 4 + 2 * (L + 4)
            for i in range(A):
                others = [j for j in range(A) if j != i]
                for k, j in enumerate(others):
                    cols = rec["obs_%d" % i][-1][lo + 2 * k:lo + 2 * k + 2]
                    assert bool(cols.any()) == bool(vis[i, j]), (ci, t, i, j)
            seen["hidden"] += int((~vis).sum())
            if design == "forest":
                k = adv - 1                 # the good agent's slot among adversary 1's others (agents 0, 2, ..)
                o1 = rec["obs_1"][-1][lo + 2 * k:lo + 2 * k + 2]
                o0 = rec["obs_0"][-1][lo + 2 * (adv - 1):lo + 2 * (adv - 1) + 2]
                v1 = rec["obs_1"][-1][lo + 2 * (A - 1):lo + 2 * (A - 1) + 2]
                if not o1.any():
                    assert o0.any() and not v1.any()
                    seen["hidden_from_1"] += 1
                elif seen["hidden_from_1"]:
                    seen["shown_after"] += 1
                i1, ig = inside[1], inside[adv]
                seen["different"] += int(i1.any() and ig.any() and not (i1 & ig).any() and not vis[1, adv])
                seen["observer_in"] += int(ig.any() and not i1.any() and not vis[adv, 1])
            speed = np.sqrt((rec["vel"][-1] ** 2).sum(-1))
            seen["clamped"] += bool((np.abs(speed - np.array([a.max_speed for a in w.agents])) < 1e-12).any())
        assert margin > THRESHOLD_MARGIN, (ci, margin)
        if design == "forest":
            assert seen["hidden_from_1"] >= 1 and seen["shown_after"] >= 1, (ci, seen)
            assert seen["different"] >= 1 and seen["observer_in"] >= 1, (ci, seen)
        if design == "food":
            assert seen["fed"] >= 3, (ci, seen)
        if design == "catch":
            assert seen["catches"] >= 1, (ci, seen)
        if design == "speak":
            assert [int(c.argmax()) for c in rec["comm"]] == [t % 4 for t in range(T)]
        if design == "bound":
            assert ramp and exp and capped, (ci, ramp, exp, capped)
            assert min(r[0] for r in np.array(rec["rewards"])[:, adv + 1]) <= -20.0 + 0.05 * 10
        for k, v in rec.items():
            out[key + k] = np.array(v)
        out[key + "obs_dims"] = np.array([sp.shape[0] for sp in env.observation_space], dtype=np.int64)
        out[key + "share_obs_dim"] = np.array(env.share_observation_space[0].shape)
        out[key + "action_dims"] = np.array(widths, dtype=np.int64)
        print("case %d (%s): adv=%d good=%d L=%d obs_dims %s margin %.3g %s" % (
            ci, design or "free play", adv, good, L, out[key + "obs_dims"], margin, seen))
    path = os.path.join(GOLD, "mpe_world_comm_cases.npz")
    np.savez_compressed(path, **out)
    print("mpe_world_comm_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
