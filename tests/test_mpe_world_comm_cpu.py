"""The device-resident simple_world_comm (onpolicy/envs/mpe/simple_world_comm.py, tensor-op path on CPU tensors) against
trajectories of the reference's own particle environment (core.py + environment.py + scenarios/simple_world_comm.py,
fixtures from tools/make_golden_mpe_world_comm.py: free play, a walk through both forests, food, a catch, the leader's
words, agents leaving the screen); rewards recomputed from the state; spaces and column views; both action forms; draws,
resets and the fixed 25-step episode; who sees whom on hand-placed worlds; the new entry point's argument checks; the train
script's --use_device_env route."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from onpolicy import _native
from onpolicy.envs.mpe.simple_world_comm import TorchSimpleWorldComm, obs_widths

T = 25
CASES = "mpe_world_comm_cases"
N_CASES = 8     # 0-2 free play; 3 forest, 4 food, 5 catch, 6 speak, 7 bound
SHAPES = [(4, 2, 1), (2, 1, 2), (1, 1, 1), (2, 1, 1), (1, 2, 1), (3, 1, 2), (3, 1, 1), (1, 2, 1)]       # (adv, good, obstacles)
FOREST_CASE, FOOD_CASE, CATCH_CASE, SPEAK_CASE, BOUND_CASE = 3, 4, 5, 6, 7
SIZE = (0.075, 0.045)           # adversary, good agent
CATCH = SIZE[1] + SIZE[0]       # 0.12
FOOD = SIZE[1] + 0.03           # 0.075
FOREST = 0.3                    # + the agent's radius: 0.375 / 0.345


def widths(adv, good, l):
    """The issue's formulas."""
    a = adv + good
    return ((4 + 2 * (l + 4) + 2 * (a - 1) + 2 * good + 6,) * adv
            + (4 + 2 * (l + 4) + 2 * (a - 1) + 2 + 2 * (good - 1),) * good)


def make(n, adv, good, l, **kw):
    return TorchSimpleWorldComm(n, adv + good, l, num_adversaries=adv, **kw)


def bound(x):
    return 0.0 if x < 0.9 else (x - 0.9) * 10 if x < 1.0 else min(np.exp(2 * x - 2), 10)


def rewards_from_state(pos, land, adv, l):
    """The issue's formulas on post-step positions [A, 2] and landmarks [L + 4, 2] -> each agent's reward [A]."""
    pos, land = np.asarray(pos, dtype=np.float64), np.asarray(land, dtype=np.float64)
    dist = np.sqrt(((pos[adv:, None] - pos[None, :adv]) ** 2).sum(-1))                      # [good, adversaries]
    food = np.sqrt(((pos[adv:, None] - land[None, l:l + 2]) ** 2).sum(-1))                  # [good, food]
    touch = dist < CATCH
    good = [-5.0 * touch[g].sum() - 2 * (bound(abs(pos[adv + g, 0])) + bound(abs(pos[adv + g, 1])))
            + 2.0 * (food[g] < FOOD).sum() + 0.05 * food[g].min() for g in range(len(pos) - adv)]
    return np.array([-0.1 * dist[:, j].min() + 5.0 * touch.sum() for j in range(adv)] + good)


def geometry(pos, land, adv, l):
    """-> (inside [A, 2] bool, sees [A, A] bool, the smallest distance of any quantity from its threshold)."""
    pos, land = np.asarray(pos, dtype=np.float64), np.asarray(land, dtype=np.float64)
    size = np.array([SIZE[0]] * adv + [SIZE[1]] * (len(pos) - adv))
    forest = np.sqrt(((pos[:, None] - land[None, l + 2:]) ** 2).sum(-1))
    inside = forest < size[:, None] + FOREST
    free = ~inside.any(1)
    sees = (inside[:, None, 0] & inside[None, :, 0]) | (inside[:, None, 1] & inside[None, :, 1]) | (free[:, None] & free[None])
    sees[0] = True
    pair = np.sqrt(((pos[adv:, None] - pos[None, :adv]) ** 2).sum(-1))
    food = np.sqrt(((pos[adv:, None] - land[None, l:l + 2]) ** 2).sum(-1))
    margin = min(np.abs(forest - (size[:, None] + FOREST)).min(), np.abs(pair - CATCH).min(), np.abs(food - FOOD).min())
    return inside, sees, float(margin)


def observations_from_state(pos, vel, land, comm, adv, l):
    """The issue's layouts -> one float64 vector per agent."""
    a = len(pos)
    inside, sees, _ = geometry(pos, land, adv, l)
    out = []
    for i in range(a):
        others = [j for j in range(a) if j != i]
        rel = [(pos[j] - pos[i]) * sees[i, j] for j in others]
        flags = np.where(inside[i], 1.0, -1.0)
        head = [vel[i], pos[i]] + [p - pos[i] for p in land] + rel
        if i < adv:
            word = np.zeros(4) if comm < 0 else np.eye(4)[comm]
            out.append(np.concatenate(head + [vel[g] * sees[i, g] for g in range(adv, a)] + [flags, word]))
        else:
            out.append(np.concatenate(head + [flags] + [vel[g] * sees[i, g] for g in range(adv, a) if g != i]))
    return out


def _load_case(env, z, key, world=0):
    for name, src in (("pos", "pos0"), ("vel", "vel0"), ("landmarks", "landmarks")):
        getattr(env, name)[world] = torch.from_numpy(np.asarray(z[key + src], dtype=np.float64))
    env.t[world] = 0
    env.comm[world] = -1


def _close(got, want, tol, msg):
    np.testing.assert_allclose(got.cpu().numpy() if torch.is_tensor(got) else got, want, rtol=tol, atol=tol, err_msg=msg)


def random_actions(rng, n, a):
    """[n, A + 1]: the leader's movement, its word, the others' movements."""
    return np.concatenate([rng.integers(0, 5, (n, 1)), rng.integers(0, 4, (n, 1)), rng.integers(0, 5, (n, a - 1))], 1)


def one_hot_actions(idx):
    """Index actions [n, A + 1] -> the host protocol's concatenated one-hots [n, 9 + 5 (A - 1)]."""
    f = torch.nn.functional.one_hot
    return torch.cat([f(idx[:, 0], 5), f(idx[:, 1], 4), f(idx[:, 2:], 5).reshape(idx.shape[0], -1)], -1).double()


def replay_case(z, case, device="cpu", ops=False, n=2):
    """World 0 follows the reference case, the other worlds take random actions (worlds must not interact).  Tolerances:
    those of test_mpe_tag_cpu.replay_case -- state 1e-9, observations 2e-6, rewards 1e-6."""
    key = "wc%d_" % case
    A, L = (int(v) for v in z[key + "dims"])
    adv = int(z[key + "num_adversaries"])
    env = make(n, adv, A - adv, L, episode_length=T, seed=0, auto_reset=False, device=device)
    dims = widths(adv, A - adv, L)
    assert env.obs_dims == tuple(z[key + "obs_dims"]) == dims
    assert [s.shape for s in env.observation_space] == [(d,) for d in dims]
    assert [s.shape for s in env.share_observation_space] == [tuple(z[key + "share_obs_dim"])] * A == [(sum(dims),)] * A
    assert list(z[key + "action_dims"]) == [9] + [5] * (A - 1)
    assert [type(s).__name__ for s in env.action_space] == ["MultiDiscrete"] + ["Discrete"] * (A - 1)
    assert list(env.action_space[0].high - env.action_space[0].low + 1) == [5, 4]
    assert [s.n for s in env.action_space[1:]] == [5] * (A - 1)
    obs = env.reset()
    assert obs.shape == (n, sum(dims)) and obs.dtype == torch.float32
    _load_case(env, z, key)
    obs = env._obs()
    for i in range(A):
        _close(env.agent_obs(obs, i)[0], z[key + "obs0_%d" % i], 2e-6, "obs0 agent %d" % i)
    rng = np.random.default_rng(99)
    step = env._step_ops if ops else env.step                      # (_step_ops: the kernel's own reference)
    seen = dict(caught=0, fed=0, hidden=0, clamped=0)
    land = z[key + "landmarks"]
    for t in range(T):
        idx = np.concatenate([z[key + "action_idx"][t][None], random_actions(rng, n - 1, A)]).astype(np.int64)
        obs, rew, done, info = step(torch.from_numpy(idx).to(device))
        assert obs.dtype == torch.float32 and obs.shape == (n, sum(dims))
        assert rew.dtype == torch.float32 and rew.shape == (n, A, 1)
        assert done.dtype == torch.bool and done.shape == (n, A)
        msg = "case %d t=%d" % (case, t)
        _close(env.pos[0], z[key + "pos"][t], 1e-9, msg)
        _close(env.vel[0], z[key + "vel"][t], 1e-9, msg)
        _close(env.landmarks[0], land, 0, msg)
        for i in range(A):
            _close(env.agent_obs(obs, i)[0], z[key + "obs_%d" % i][t], 2e-6, msg + " agent %d" % i)
        _close(rew[0], z[key + "rewards"][t].reshape(A, 1), 1e-6, msg)
        ind = np.array([info[0][j]["individual_reward"] for j in range(A)])
        _close(ind, z[key + "individual_rewards"][t], 1e-6, msg)
        np.testing.assert_array_equal(done[0].cpu().numpy(), z[key + "dones"][t])
        assert bool(done[0].all()) == (t == T - 1)
        assert int(env.comm[0]) == int(z[key + "comm"][t].argmax()) == int(idx[0, 1]) and z[key + "comm"][t].sum() == 1
        # rewards and observations as the issue states them, from the state
        pos, vel = env.pos[0].cpu().numpy(), env.vel[0].cpu().numpy()
        want = rewards_from_state(pos, land, adv, L)
        _close(ind, want, 1e-9, msg)
        _close(rew[0, :, 0], want, 1e-6, msg)
        for i, o in enumerate(observations_from_state(pos, vel, land, int(env.comm[0]), adv, L)):
            _close(env.agent_obs(obs, i)[0], o, 2e-6, msg + " layout of agent %d" % i)
        inside, sees, margin = geometry(pos, land, adv, L)
        assert margin > 1e-6, (msg, margin)
        seen["caught"] += want[0] > 1.0
        seen["fed"] += bool((want[adv:] > 1.5).any())
        seen["hidden"] += int((~sees).sum())
        speed = env.vel[0].norm(dim=-1).cpu().numpy()
        top = np.array([1.0] * adv + [1.3] * (A - adv))
        assert (speed <= top + 1e-12).all(), (msg, speed)
        seen["clamped"] += bool((speed > top - 1e-12).any())
    assert seen["clamped"] >= 10, seen                  # the top speed acts in most steps
    if case == CATCH_CASE:
        assert seen["caught"] >= 1, seen
    if case == FOOD_CASE:
        assert seen["fed"] >= 3, seen
    if case == FOREST_CASE:
        assert seen["hidden"] >= 1, seen
    return seen


@pytest.mark.parametrize("case", range(N_CASES))
def test_step_ops_matches_reference_trajectories(gold, case):
    replay_case(gold.npz(CASES), case, ops=True)


def test_fixture_has_the_cases_the_scenario_needs(gold):
    z = gold.npz(CASES)
    shapes = [(int(z["wc%d_num_adversaries" % c]), int(z["wc%d_dims" % c][0]) - int(z["wc%d_num_adversaries" % c]),
               int(z["wc%d_dims" % c][1])) for c in range(N_CASES)]
    assert shapes == SHAPES and shapes[:3] == [(4, 2, 1), (2, 1, 2), (1, 1, 1)]
    assert "wc%d_dims" % N_CASES not in z
    assert list(z["wc0_obs_dims"]) == [34] * 4 + [28] * 2 and list(z["wc1_obs_dims"]) == [28, 28, 22]
    for c, (adv, good, l) in enumerate(shapes):
        key = "wc%d_" % c
        a = adv + good
        assert z[key + "rewards"].shape == (T, a, 1) and z[key + "action_idx"].shape == (T, a + 1)
        assert z[key + "landmarks"].shape == (l + 4, 2) and z[key + "comm"].shape == (T, 4)
        assert np.array_equal(z[key + "rewards"][..., 0], z[key + "individual_rewards"])      # not shared
        for i in range(adv):
            assert not z[key + "obs0_%d" % i][-4:].any()                                       # nothing said yet
            assert np.array_equal(z[key + "obs_%d" % i][:, -4:], z[key + "comm"])              # heard in the same step
        # no case is exempt: no distance within 1e-6 of the threshold that decides hiding, eating or a catch
        for pos in [z[key + "pos0"]] + list(z[key + "pos"]):
            assert geometry(pos, z[key + "landmarks"], adv, l)[2] > 1e-6, c
    # (a) forest: adversary 1's columns for the good agent (agent 2) are zero in some steps while the leader's are not,
    # non-zero later; the two in different forests, hidden; the observer in a forest, the other in the open, hidden
    key, (adv, good, l) = "wc%d_" % FOREST_CASE, SHAPES[FOREST_CASE]
    lo = 4 + 2 * (l + 4)
    mine, leaders = z[key + "obs_1"][:, lo + 2:lo + 4], z[key + "obs_0"][:, lo + 2:lo + 4]
    hidden = ~mine.any(1)
    assert hidden.any() and leaders[hidden].all() and mine[np.argmax(hidden):].any()
    assert not z[key + "vel0"][adv].any() and (z[key + "action_idx"][:, 2] == 1).all()
    inside0 = geometry(z[key + "pos0"], z[key + "landmarks"], adv, l)[0]
    assert inside0[adv, 0] and not inside0[1].any()
    different = observer_in = 0
    for pos in z[key + "pos"]:
        inside, sees, _ = geometry(pos, z[key + "landmarks"], adv, l)
        different += bool(inside[1].any() and inside[adv].any() and not (inside[1] & inside[adv]).any() and not sees[1, adv])
        observer_in += bool(inside[adv].any() and not inside[1].any() and not sees[adv, 1])
    assert different >= 1 and observer_in >= 1
    # (b) food: at least 3 steps pay the +2
    assert (z["wc%d_rewards" % FOOD_CASE][:, SHAPES[FOOD_CASE][0], 0] > 1.5).sum() >= 3
    # (c) catch: +5 to every adversary, -5 to the good agent
    r = z["wc%d_rewards" % CATCH_CASE][..., 0]
    paid = r[:, 0] > 4.0
    assert paid.sum() >= 1 and (r[paid, :3] > 4.0).all() and (r[paid, :3] < 5.0).all() and (r[paid, 3] < -4.0).all()
    # (d) speak: the word cycles 0, 1, 2, 3
    assert list(z["wc%d_comm" % SPEAK_CASE].argmax(1)) == [t % 4 for t in range(T)]
    assert list(z["wc%d_action_idx" % SPEAK_CASE][:, 1]) == [t % 4 for t in range(T)]
    # (e) bound: good agent 1 passes through the ramp into the exp branch, good agent 2 sits at the cap, paid doubled
    x = np.abs(z["wc%d_pos" % BOUND_CASE][:, 1, 0])
    assert z["wc%d_pos0" % BOUND_CASE][1, 0] == 0.85
    assert ((x > 0.9) & (x < 1.0)).any() and ((x >= 1.0) & (np.exp(2 * x - 2) < 10)).any()
    assert abs(z["wc%d_pos0" % BOUND_CASE][2, 1]) == 2.3
    assert (z["wc%d_rewards" % BOUND_CASE][:, 2, 0] <= -19.5).all()


def test_spaces_widths_and_column_views():
    for (adv, good, l), dims in (((4, 2, 1), (34,) * 4 + (28,) * 2), ((2, 1, 2), (28, 28, 22)), ((1, 1, 1), (24, 18))):
        a = adv + good
        env = make(3, adv, good, l)
        assert env.obs_dims == dims == widths(adv, good, l) == obs_widths(adv, good, l)
        assert env._obs_shape() == (3, sum(dims)) and (env.l, env.num_obstacles) == (l + 4, l)
        assert env.state_names == ("pos", "vel", "landmarks", "t", "comm") and env.shared_reward is False
        assert env.landmarks.shape == (3, l + 4, 2) and env.comm.shape == (3,) and env.comm.dtype == torch.int64
        assert [s.shape for s in env.observation_space] == [(d,) for d in dims]
        assert [s.shape for s in env.share_observation_space] == [(sum(dims),)] * a
        assert [type(s).__name__ for s in env.action_space] == ["MultiDiscrete"] + ["Discrete"] * (a - 1)
        obs = env.reset()
        assert obs.shape == (3, sum(dims)) and env.comm.tolist() == [-1] * 3
        lo = 0
        for i, d in enumerate(dims):
            view = env.agent_obs(obs, i)
            assert view.shape == (3, d) and view.data_ptr() == obs[:, lo:].data_ptr() and view._base is obs
            assert torch.equal(view[:, 0:2], env.vel[:, i].float()) and torch.equal(view[:, 2:4], env.pos[:, i].float())
            assert torch.equal(view[:, 4:4 + 2 * (l + 4)], (env.landmarks - env.pos[:, i:i + 1]).reshape(3, -1).float())
            lo += d
    assert float(make(64, 4, 2, 1, seed=2).reset()[:, 4:14].abs().max()) <= 1.8          # landmarks at 0.8 U(-1, 1)
    for bad in (dict(num_agents=4, num_adversaries=4), dict(num_agents=4, num_adversaries=0),
                dict(num_agents=1, num_adversaries=1), dict(num_landmarks=0)):
        with pytest.raises(AssertionError, match="simple_world_comm"):
            TorchSimpleWorldComm(4, **bad)
    default = TorchSimpleWorldComm(2)
    assert (default.a, default.num_obstacles, default.num_adversaries, default.world_length) == (6, 1, 4, 25)


def _placed(adv, good, where, forests=((-0.5, 0.0), (0.5, 0.0))):
    """One world with food and the obstacle far away, the forests at ``forests`` and the agents at ``where``."""
    env = make(1, adv, good, 1, auto_reset=False)
    env.reset()
    env.landmarks[0] = torch.tensor([[5.0, 5.0], [5.0, -5.0], [-5.0, 5.0]] + [list(f) for f in forests], dtype=torch.float64)
    env.pos[0] = torch.tensor(where, dtype=torch.float64)
    env.vel[0] = torch.arange(1, 2 * (adv + good) + 1, dtype=torch.float64).reshape(-1, 2)
    return env


def test_visibility_truth_table():
    """Every branch of the rule on hand-placed worlds: 3 adversaries (0 the leader) and 2 good agents; forest 0 at
    (-0.5, 0), forest 1 at (0.5, 0); an adversary is inside below 0.375, a good agent below 0.345."""
    f0, f1, out = (-0.5, 0.0), (0.5, 0.0), (0.0, 0.9)
    # leader in the open; adversary 1 in forest 0; adversary 2 in forest 1; good 3 in forest 0; good 4 in the open
    env = _placed(3, 2, [out, (-0.6, 0.1), f1, (-0.4, -0.1), (0.0, -0.9)])
    inside = env.inside()[0]
    assert inside.tolist() == [[False, False], [True, False], [False, True], [True, False], [False, False]]
    sees = env.visible()[0]
    want = torch.tensor([[1, 1, 1, 1, 1],          # the leader sees everybody, in a forest or not
                         [0, 1, 0, 1, 0],          # forest 0: the other one in forest 0 only -- not the open, not forest 1
                         [0, 0, 1, 0, 0],          # forest 1, alone in it
                         [0, 1, 0, 1, 0],          # forest 0
                         [1, 0, 0, 0, 1]],         # the open: the leader, who is in the open as well, and nobody in a forest
                        dtype=torch.bool)
    assert torch.equal(sees, want)
    obs = env._obs()
    pos, vel = env.pos[0], env.vel[0]
    for i in range(5):
        o = env.agent_obs(obs, i)[0].double()
        others = [j for j in range(5) if j != i]
        for k, j in enumerate(others):
            cols = o[14 + 2 * k:16 + 2 * k]
            assert torch.equal(cols, (pos[j] - pos[i]).float().double() if want[i, j] else torch.zeros(2, dtype=torch.float64)), (i, j)
        flags = [1.0 if inside[i, f] else -1.0 for f in (0, 1)]
        if i < 3:       # the good agents' velocities, the flags, the word
            for k, g in enumerate((3, 4)):
                assert o[22 + 2 * k:24 + 2 * k].tolist() == (vel[g].tolist() if want[i, g] else [0.0, 0.0]), (i, g)
            assert o[26:28].tolist() == flags and o[28:].tolist() == [0.0] * 4 and o.numel() == 32
        else:           # the flags, then the other good agent's velocity
            g = 7 - i
            assert o[22:24].tolist() == flags and o.numel() == 26
            assert o[24:26].tolist() == (vel[g].tolist() if want[i, g] else [0.0, 0.0]), i
    # the leader inside forest 1 still sees the open and forest 0; those in the open do not see it
    env = _placed(3, 2, [f1, out, f0, (-0.4, -0.1), (0.0, -0.9)])
    sees = env.visible()[0]
    assert sees[0].all() and sees[:, 0].tolist() == [True, False, False, False, False]
    assert sees[1].tolist() == [False, True, False, False, True]           # the open sees the open
    # forests that overlap: an agent inside both sees those in either, and is seen by them
    env = _placed(2, 2, [out, (0.0, 0.0), (-0.3, 0.0), (0.3, 0.0)], forests=((-0.2, 0.0), (0.2, 0.0)))
    assert env.inside()[0].tolist() == [[False, False], [True, True], [True, False], [False, True]]
    sees = env.visible()[0]
    assert sees[1].tolist() == [False, True, True, True] and sees[2].tolist() == [False, True, True, False]
    assert sees[3].tolist() == [False, True, False, True]
    # the radii: at 0.36 from a forest's centre an adversary is inside, a good agent is not
    env = _placed(2, 1, [out, (-0.5 + 0.36, 0.0), (0.5, 0.36)])
    assert env.inside()[0].tolist() == [[False, False], [True, False], [False, False]]
    env.comm[0] = 2
    o = env._obs()
    assert env.agent_obs(o, 0)[0, -4:].tolist() == env.agent_obs(o, 1)[0, -4:].tolist() == [0.0, 0.0, 1.0, 0.0]
    assert env.agent_obs(o, 1)[0, -6:-4].tolist() == [1.0, -1.0] and env.agent_obs(o, 2)[0, 18:20].tolist() == [-1.0, -1.0]


def test_rewards_are_per_agent_and_follow_the_formulas():
    for adv, good, l in ((4, 2, 1), (2, 1, 2), (1, 1, 1)):
        a = adv + good
        env = make(9, adv, good, l, seed=4)
        env.reset()
        env.pos[0, adv, 0], env.pos[0, adv, 1] = env.pos[0, 0, 0] + 0.12, env.pos[0, 0, 1]      # world 0: a pair that meets
        env.pos[1, adv] = torch.tensor([0.95, -1.4])        # world 1: on the ramp and in the exp branch
        env.landmarks[2, l] = env.pos[2, adv] + torch.tensor([0.02, 0.01], dtype=torch.float64)       # world 2: on a food ...
        env.landmarks[2, :l] = 5.0                                                                    # ... no obstacle near
        for step in range(5):
            act = torch.from_numpy(random_actions(np.random.default_rng(step), 9, a))
            if step == 0:
                act[0, 0], act[0, adv + 1] = 1, 2           # into each other: they cross, close after the step
                act[2, adv + 1] = 0
            obs, rew, done, info = env.step(act)
            per_agent = info._per_agent
            assert per_agent.shape == (9, a) and per_agent.dtype == torch.float64
            assert torch.equal(rew[..., 0], per_agent.float())
            want = np.stack([rewards_from_state(env.pos[w].numpy(), env.landmarks[w].numpy(), adv, l) for w in range(9)])
            assert min(geometry(env.pos[w].numpy(), env.landmarks[w].numpy(), adv, l)[2] for w in range(9)) > 1e-9
            np.testing.assert_allclose(per_agent.numpy(), want, rtol=1e-12, atol=1e-12)
            if step == 0:
                assert float(per_agent[0, 0]) > 4.0 and float(per_agent[0, adv]) < -4.0
                assert float(per_agent[1, adv]) < -0.8 and float(per_agent[2, adv]) > 1.5
            assert [d["individual_reward"] for d in info[3]] == per_agent[3].tolist()


def test_index_and_one_hot_actions_step_alike():
    n, a = 7, 6
    envs = [make(n, 4, 2, 1, seed=5, world_length=4) for _ in range(2)]
    first = [e.reset() for e in envs]
    assert torch.equal(first[0], first[1])
    rng = np.random.default_rng(1)
    for _ in range(9):                                          # crosses two auto-resets
        idx = torch.from_numpy(random_actions(rng, n, a))
        one_hot = one_hot_actions(idx)
        assert one_hot.shape == (n, 9 + 5 * (a - 1))
        assert torch.equal(envs[0]._kernel_actions(one_hot), idx) and envs[0]._kernel_actions(idx) is idx
        res = [envs[0].step(idx), envs[1].step(one_hot)]
        for x, y in zip(res[0][:3], res[1][:3]):
            assert torch.equal(x, y)
        for name in TorchSimpleWorldComm.state_names:
            assert torch.equal(getattr(envs[0], name), getattr(envs[1], name)), name
    with pytest.raises(AssertionError):
        envs[0].step(torch.zeros(n, a, dtype=torch.int64))     # the leader's word is missing


def test_state_names_and_draw_order():
    """comm besides the particle state; a restart draws agent positions, then all L + 4 landmarks."""
    assert TorchSimpleWorldComm.state_names == ("pos", "vel", "landmarks", "t", "comm")
    assert TorchSimpleWorldComm.landmark_scale == 0.8
    env = make(5, 4, 2, 1, seed=11)
    env.reset()
    g = torch.Generator().manual_seed(11)
    pos = torch.empty(5, 6, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    land = torch.empty(5, 5, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    assert torch.equal(env.pos, pos) and torch.equal(env.landmarks, 0.8 * land)
    assert float(env.vel.abs().max()) == 0.0 and int(env.t.abs().max()) == 0 and env.comm.tolist() == [-1] * 5
    assert torch.equal(env.rng.get_state(), g.get_state())


def test_reset_in_place_equals_reset_at_fixed_addresses():
    a, b = make(6, 2, 2, 2, seed=8), make(6, 2, 2, 2, seed=8)
    a.reset(), b.reset()
    rng = np.random.default_rng(3)
    for _ in range(3):
        act = torch.from_numpy(random_actions(rng, 6, 4))
        a.step(act), b.step(act)
    assert int(b.comm.min()) >= 0
    kept = {k: getattr(b, k) for k in b.state_names}
    oa, ob = a.reset(), b.reset_in_place()
    assert torch.equal(oa, ob)
    for k in a.state_names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert getattr(b, k) is kept[k], k
    assert b.comm.tolist() == [-1] * 6
    assert torch.equal(a.rng.get_state(), b.rng.get_state())


def test_auto_reset_clears_comm_and_takes_the_draws_of_reset():
    n, L, a = 16, 6, 6
    env = make(n, 4, 2, 1, seed=3, world_length=L)
    env.reset()
    env.t = torch.arange(n) % L                                                        # staggered episodes
    rng = np.random.default_rng(2)
    restarted = 0
    for _ in range(2 * L):
        before = {k: getattr(env, k).clone() for k in env.state_names}
        state = env.rng.get_state()
        act = torch.from_numpy(random_actions(rng, n, a))
        act[:, 0], act[:, 2:] = 1 + act[:, 0] % 4, 1 + act[:, 2:] % 4                  # every agent pushes
        obs, rew, done, info = env.step(act)
        fin = done[:, 0]
        assert bool((done == fin[:, None]).all())
        assert torch.equal(fin, before["t"] + 1 >= L)
        assert bool(fin.any()) and not bool(fin.all())
        restarted += int(fin.sum())
        g = torch.Generator()
        g.set_state(state)
        fresh_pos = torch.empty(n, a, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
        fresh_land = torch.empty(n, 5, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
        assert torch.equal(env.rng.get_state(), g.get_state())                         # the draws of a reset, no more
        assert bool((env.t[fin] == 0).all()) and float(env.vel[fin].abs().max()) == 0.0
        assert torch.equal(env.pos[fin], fresh_pos[fin]) and torch.equal(env.landmarks[fin], 0.8 * fresh_land[fin])
        assert bool((env.comm[fin] == -1).all()) and torch.equal(env.comm[~fin], act[~fin, 1])
        assert float(obs[fin][:, :2].abs().max()) == 0.0                               # the fresh world's observation
        assert torch.equal(obs[fin][:, 2:4], fresh_pos[fin][:, 0].float())
        assert float(obs[fin][:, 30:34].abs().max()) == 0.0                            # the leader's word columns
        assert torch.equal(obs[~fin][:, 30:34], torch.nn.functional.one_hot(act[~fin, 1], 4).float())
        go = ~fin
        assert torch.equal(env.t[go], before["t"][go] + 1)
        assert torch.equal(env.landmarks[go], before["landmarks"][go])
        assert float(env.vel[go].abs().sum(-1).min()) > 0.0
    assert restarted == 2 * n                                                          # every world, twice


def test_an_episode_is_25_steps_whatever_the_episode_length():
    env = make(3, 1, 1, 1, episode_length=10, seed=1)
    assert env.world_length == 25
    env.reset()
    for t in range(1, 27):
        done = env.step(torch.zeros(3, 3, dtype=torch.int64))[2]
        assert bool(done.all()) == (t == 25) and bool(done.any()) == (t == 25), t
    assert env.t.tolist() == [1, 1, 1]
    assert TorchSimpleWorldComm(3, episode_length=40, world_length=7).world_length == 7


def test_only_obstacles_collide_and_coincident_centres_get_no_force():
    """Food and forests exert no force; the reference divides by zero for coincident centres, the project leaves such a
    pair alone, agent on agent and agent on obstacle."""
    env = make(2, 2, 1, 1, seed=6, auto_reset=False)
    env.reset()
    far = [[5.0, 5.0], [5.0, -5.0], [-5.0, 5.0], [-5.0, -5.0], [-7.0, 0.0]]
    env.landmarks[:] = torch.tensor(far, dtype=torch.float64)
    env.pos[0] = torch.tensor([[0.3, 0.3], [-0.6, -0.6], [0.3, 0.3]])      # the leader and the good agent coincide ...
    env.landmarks[0, 0] = torch.tensor([-0.6, -0.6])                       # ... and adversary 1 sits on the obstacle's centre
    # world 1: every agent 0.05 from a food or a forest's centre, far enough apart for their own contact force to underflow
    env.pos[1] = torch.tensor([[0.0, 0.0], [2.0, 2.0], [-2.0, 2.0]])
    env.landmarks[1, 1:4] = env.pos[1] + torch.tensor([0.05, 0.0], dtype=torch.float64)
    before = env.pos.clone()
    obs, rew, _, _ = env.step(torch.zeros(2, 4, dtype=torch.int64))
    assert torch.isfinite(env.pos).all() and torch.isfinite(env.vel).all() and torch.isfinite(obs).all()
    assert torch.equal(env.pos, before) and float(env.vel.abs().max()) == 0.0
    assert float(rew[0, 0, 0]) == 5.0 and float(rew[0, 1, 0]) > 4.0 and float(rew[0, 2, 0]) < -4.0
    env.pos[0, 1, 0] += 0.1                                                # off the centre: now the obstacle pushes
    env.step(torch.zeros(2, 4, dtype=torch.int64))
    assert float(env.vel[0, 1, 0]) > 1.0 - 1e-12 and float(env.vel[0, 1, 1]) == 0.0
    assert float(env.vel[1].abs().max()) == 0.0


# particle_worlds.py changed by one line of its docstring (the list of scenarios): sha256 over state, observations and
# rewards of ten seeded tensor-op steps of the five older scenarios, recorded on the parent commit (the four oldest:
# test_mpe_tag_cpu.PARENT_DIGESTS, from before simple_tag; simple_tag with a pair and a landmark in contact)
TAG_PARENT_DIGEST = "19b0c847d9d82c8629fc8df1ac0cc09d7d431a2df85f86baef23dc1d66f37135"


def test_older_scenarios_step_bit_identically():
    import hashlib
    from onpolicy.envs.mpe.simple_tag import TorchSimpleTag
    from test_mpe_tag_cpu import PARENT_DIGESTS, older_scenario_digest
    for name in sorted(PARENT_DIGESTS):
        assert older_scenario_digest(name) == PARENT_DIGESTS[name], name
    n = 6
    g = torch.Generator().manual_seed(12)
    env = TorchSimpleTag(n, 4, 2, seed=2, world_length=4, num_adversaries=3)
    h = hashlib.sha256()
    h.update(env.reset().numpy().tobytes())
    env.pos[0, 3] = env.pos[0, 0] + torch.tensor([0.06, 0.01], dtype=torch.float64)
    env.landmarks[0, 0] = env.pos[0, 1] + torch.tensor([-0.2, 0.05], dtype=torch.float64)
    for _ in range(10):
        obs, rew, done, info = env._step_ops(torch.randint(0, 5, (n, 4), generator=g))
        for x in (obs, rew, done, info._per_agent) + tuple(getattr(env, k) for k in env.state_names):
            h.update(x.contiguous().numpy().tobytes())
    assert h.hexdigest() == TAG_PARENT_DIGEST


def test_new_entry_point_validates_arguments():
    lib = _native.lib()
    name = "mappo_simple_world_comm_step"
    assert name in _native.SIGNATURES
    fn = getattr(lib, name)
    assert fn(*([None] * 12), 4, 6, 4, 1, 25, 1, None) == -1
    keep = [(ctypes.c_double * 64)() for _ in range(12)]
    ptrs = [ctypes.addressof(b) for b in keep]
    # pos vel landmarks t comm actions | fresh_pos fresh_landmarks | obs rewards dones per_agent
    for i in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):                       # every required pointer
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 6, 4, 1, 25, 0, None) == -1, i
    for i in (6, 7):                                                 # the fresh draws: required with auto_reset
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 6, 4, 1, 25, 1, None) == -1, i
    for n, a, adv, l, length in ((0, 6, 4, 1, 25), (-3, 6, 4, 1, 25), (4, 6, 0, 1, 25), (4, 6, 6, 1, 25),
                                 (4, 6, 7, 1, 25), (4, 1, 1, 1, 25), (4, 0, 0, 1, 25), (4, 6, -1, 1, 25),
                                 (4, 6, 4, 0, 25), (4, 6, 4, 1, 0), (4, 17, 17, 1, 25), (4, 6, 4, -1, 25)):
        assert fn(*ptrs, n, a, adv, l, length, 1, None) == -2, (n, a, adv, l, length)
    assert fn(*ptrs, 4, 17, 4, 1, 25, 1, None) == -4                 # MAPPO_E_TOO_MANY: agents
    assert fn(*ptrs, 4, 6, 4, 5, 25, 1, None) == -4                  # ... obstacles
    assert lib.mappo_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "mappo_hip.h")).read()
    assert re.search(r"\bint mappo_simple_world_comm_step\(", header)
    assert "scenarios/simple_world_comm.py" in header and re.search(r"#define MAPPO_WORLD_COMM_MAX_OBSTACLES 4\b", header)
    from onpolicy.envs.mpe import simple_world_comm
    assert (simple_world_comm.KERNEL_MAX_AGENTS, simple_world_comm.KERNEL_MAX_LANDMARKS) == (16, 4)
    assert not make(2, 4, 2, 1).graph_safe                           # CPU tensors: the tensor-op path


def world_comm_argv(algo, adv=4, good=2, landmarks=1, n=2, steps=100, hidden=16, agents=None, counts=True):
    """The reference's train_mpe.sh family at small sizes."""
    argv = ["--env_name", "MPE", "--algorithm_name", algo, "--experiment_name", "check",
            "--scenario_name", "simple_world_comm", "--num_agents", str(adv + good if agents is None else agents),
            "--num_landmarks", str(landmarks),
            "--seed", "1", "--n_training_threads", "1", "--n_rollout_threads", str(n), "--num_mini_batch", "1",
            "--episode_length", "25", "--num_env_steps", str(steps), "--ppo_epoch", "2", "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--share_policy", "--hidden_size", str(hidden),
            "--data_chunk_length", "5", "--use_wandb", "--log_interval", "1"]
    return argv + (["--num_adversaries", str(adv), "--num_good_agents", str(good)] if counts else [])


@pytest.mark.parametrize("algo,adv,good", [("mappo", 4, 2), ("rmappo", 2, 1)])
def test_train_script_with_device_resident_worlds(monkeypatch, tmp_path, algo, adv, good):
    """train_mpe --use_device_env --share_policy for simple_world_comm end to end (host buffer stand-in, "device" = CPU
    tensors): no external env tree, one policy and buffer per agent with its own widths, action width and rewards."""
    import onpolicy.runner.separated.base_runner as base
    from host_buffer import HostSeparatedBuffer
    from onpolicy.scripts.train import _launch, train_mpe
    threads = torch.get_num_threads()
    agents = adv + good

    def device_of(all_args):
        torch.set_num_threads(all_args.n_training_threads)
        return torch.device("cpu")
    monkeypatch.setattr(base, "SeparatedReplayBuffer", HostSeparatedBuffer)
    monkeypatch.setattr(_launch, "device_of", device_of)
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    monkeypatch.delenv("MAPPO_ENVS_PATH", raising=False)
    try:
        # 100 steps: two episodes of 25; 4 against 2 without the two flags, which then read as 4 and 2
        runner = train_mpe.main(world_comm_argv(algo, adv, good, counts=(adv, good) != (4, 2)) + ["--use_device_env"])
        assert type(runner).__module__ == "onpolicy.runner.separated.mpe_runner"
        assert type(runner.envs) is TorchSimpleWorldComm and runner.rollout_graph is None
        assert runner.envs.num_adversaries == adv and runner.envs.a == agents and runner.envs.num_obstacles == 1
        dims = widths(adv, good, 1)
        assert len(runner.buffer) == agents
        lo = 0
        for agent, (b, d) in enumerate(zip(runner.buffer, dims)):
            assert b.obs.shape == (26, 2, d) and b.share_obs.shape == (26, 2, sum(dims))
            assert torch.equal(b.share_obs, runner.buffer[0].share_obs)               # a common share_obs ...
            assert torch.equal(b.share_obs[..., lo:lo + d], b.obs)                    # ... of which the agent's own is a slice
            lo += d
            assert b.actions.shape == (25, 2, 2 if agent == 0 else 1)                 # the leader: movement and word
            assert float(b.actions.min()) >= 0 and float(b.actions[..., 0].max()) <= 4
            assert bool((b.actions == b.actions.round()).all())
            assert torch.isfinite(b.rewards).all()
            assert float(b.masks.min()) == 0.0                                        # the worlds restarted at step 25
        assert float(runner.buffer[0].actions[..., 1].max()) <= 3
        # every adversary heard the leader's word of the step before; after the restart at step 25 nothing
        said = torch.nn.functional.one_hot(runner.buffer[0].actions[:, :, 1].long(), 4).float()
        for b in runner.buffer[:adv]:
            assert torch.equal(b.obs[1:25, :, -4:], said[:24]) and float(b.obs[25, :, -4:].abs().max()) == 0.0
        rows = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
        tags = {r["tag"] for r in rows}
        for agent in range(agents):
            want = {"agent%d/%s" % (agent, k) for k in ("value_loss", "policy_loss", "dist_entropy",
                                                        "average_episode_rewards", "individual_rewards")}
            assert want <= tags, sorted(tags)
        losses = [r for r in rows if r["tag"].split("/")[-1] in ("value_loss", "policy_loss", "dist_entropy")]
        assert len(losses) == agents * 3 * 2                                          # agents x tags x episodes
        for r in rows:
            assert all(np.isfinite(v) for k, v in r.items() if k not in ("tag", "step")), r
    finally:
        torch.set_num_threads(threads)


def test_device_env_refusals(monkeypatch, tmp_path):
    """simple_world_comm runs under the separated runner with rmappo / mappo / ippo, num_agents = adversaries + good
    agents, at least one of each and at least one obstacle."""
    from onpolicy.config import get_config
    from onpolicy.scripts.train import _launch, train_mpe
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    shared = [a for a in world_comm_argv("mappo") if a != "--share_policy"]
    with pytest.raises(NotImplementedError, match="use_device_env"):
        train_mpe.main(shared + ["--use_device_env"])
    for algo in ("happo", "hatrpo"):
        with pytest.raises(NotImplementedError, match="use_device_env"):
            train_mpe.main(world_comm_argv(algo) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"simple_world_comm .* not 7 = 4 \+ 2"):
        train_mpe.main(world_comm_argv("mappo", agents=7) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"not 4 = 4 \+ 2"):          # the flags left out: 4 and 2
        train_mpe.main(world_comm_argv("mappo", agents=4, counts=False) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"not 4 = 4 \+ 0"):
        train_mpe.main(world_comm_argv("mappo", adv=4, good=0) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"not 2 = 0 \+ 2"):
        train_mpe.main(world_comm_argv("mappo", adv=0, good=2) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match="at least one obstacle"):
        train_mpe.main(world_comm_argv("mappo", landmarks=0) + ["--use_device_env"])
    assert "simple_world_comm" in train_mpe.DEVICE_ENVS and "simple_world_comm" in train_mpe.SEPARATED_DEVICE_ENVS
    assert train_mpe.WORLD_COMM_DEFAULTS == (4, 2) and train_mpe.TAG_DEFAULTS == (3, 1)
    args = train_mpe.parse_args(["--scenario_name", "simple_world_comm"], get_config())
    assert not hasattr(args, "num_adversaries") and train_mpe.tag_counts(args) == (4, 2)
    args = train_mpe.parse_args(["--scenario_name", "simple_tag"], get_config())
    assert train_mpe.tag_counts(args) == (3, 1)
