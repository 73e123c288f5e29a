"""The device-resident simple_tag (onpolicy/envs/mpe/simple_tag.py, tensor-op path on CPU tensors) against trajectories
of the reference's own particle environment (core.py + environment.py + scenarios/simple_tag.py, fixtures from
tools/make_golden_mpe_tag.py: free play, a catch, an agent pressed against a landmark, agents leaving the screen); rewards
recomputed from the state; spaces and column views; both action forms; draws, resets and the fixed 25-step episode;
coincident centres; the four older scenarios stepping as they did before the core learnt top speeds, per-pair radii and
per-agent action scales; the new entry point's argument checks; the train script's --use_device_env route."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from onpolicy import _native
from onpolicy.envs.mpe.simple_tag import TorchSimpleTag

T = 25
CASES = "mpe_tag_cases"
N_CASES = 6     # 0-2 free play at (adv, good, L) = (3, 1, 2), (2, 2, 2), (1, 1, 1); 3 catch, 4 landmark, 5 bound
SHAPES = [(3, 1, 2), (2, 2, 2), (1, 1, 1), (3, 1, 2), (2, 2, 2), (1, 2, 1)]
CATCH_CASE, LANDMARK_CASE, BOUND_CASE = 3, 4, 5
CATCH = 0.05 + 0.075            # a good agent's radius + an adversary's


def widths(adv, good, l):
    a = adv + good
    return (4 + 2 * l + 2 * (a - 1) + 2 * good,) * adv + (4 + 2 * l + 2 * (a - 1) + 2 * (good - 1),) * good


def make(n, adv, good, l, **kw):
    return TorchSimpleTag(n, adv + good, l, num_adversaries=adv, **kw)


def bound(x):
    return 0.0 if x < 0.9 else (x - 0.9) * 10 if x < 1.0 else min(np.exp(2 * x - 2), 10)


def rewards_from_state(pos, adv):
    """The issue's formulas on post-step positions [A, 2] -> each agent's reward [A]."""
    pos = np.asarray(pos, dtype=np.float64)
    dist = np.sqrt(((pos[adv:, None] - pos[None, :adv]) ** 2).sum(-1))                      # [good, adversaries]
    touch = dist < CATCH
    good = [-10.0 * touch[g].sum() - bound(abs(pos[adv + g, 0])) - bound(abs(pos[adv + g, 1]))
            for g in range(len(pos) - adv)]
    return np.array([10.0 * touch.sum()] * adv + good)


def _load_case(env, z, key, world=0):
    for name, src in (("pos", "pos0"), ("vel", "vel0"), ("landmarks", "landmarks")):
        getattr(env, name)[world] = torch.from_numpy(np.asarray(z[key + src], dtype=np.float64))
    env.t[world] = 0


def _close(got, want, tol, msg):
    np.testing.assert_allclose(got.cpu().numpy() if torch.is_tensor(got) else got, want, rtol=tol, atol=tol, err_msg=msg)


def replay_case(z, case, device="cpu", ops=False, n=2):
    """World 0 follows the reference case, the other worlds take random actions (worlds must not interact).  Tolerances:
    those of test_mpe_push_cpu.replay_case -- state 1e-9, observations 2e-6, rewards 1e-6."""
    key = "tag%d_" % case
    A, L = (int(v) for v in z[key + "dims"])
    adv = int(z[key + "num_adversaries"])
    env = make(n, adv, A - adv, L, episode_length=T, seed=0, auto_reset=False, device=device)
    dims = widths(adv, A - adv, L)
    assert env.obs_dims == tuple(z[key + "obs_dims"]) == dims
    assert [s.shape for s in env.observation_space] == [(d,) for d in dims]
    assert [s.shape for s in env.share_observation_space] == [tuple(z[key + "share_obs_dim"])] * A == [(sum(dims),)] * A
    assert [s.n for s in env.action_space] == list(z[key + "action_dims"]) == [5] * A
    assert [type(s).__name__ for s in env.action_space] == ["Discrete"] * A
    obs = env.reset()
    assert obs.shape == (n, sum(dims)) and obs.dtype == torch.float32
    _load_case(env, z, key)
    obs = env._obs()
    for i in range(A):
        _close(env.agent_obs(obs, i)[0], z[key + "obs0_%d" % i], 2e-6, "obs0 agent %d" % i)
    rng = np.random.default_rng(99)
    step = env._step_ops if ops else env.step                      # (_step_ops: the kernel's own reference)
    seen = dict(pair=0, landmark=0, caught=0, clamped=0)
    size = np.array([0.075] * adv + [0.05] * (A - adv))
    for t in range(T):
        pos = env.pos[0].cpu().numpy()
        seen["pair"] += np.sqrt(((pos[adv] - pos[0]) ** 2).sum()) < CATCH
        seen["landmark"] += np.sqrt(((pos[0] - env.landmarks[0, 0].cpu().numpy()) ** 2).sum()) < size[0] + 0.2
        idx = np.concatenate([z[key + "action_idx"][t][None], rng.integers(0, 5, (n - 1, A))]).astype(np.int64)
        obs, rew, done, info = step(torch.from_numpy(idx).to(device))
        assert obs.dtype == torch.float32 and obs.shape == (n, sum(dims))
        assert rew.dtype == torch.float32 and rew.shape == (n, A, 1)
        assert done.dtype == torch.bool and done.shape == (n, A)
        msg = "case %d t=%d" % (case, t)
        _close(env.pos[0], z[key + "pos"][t], 1e-9, msg)
        _close(env.vel[0], z[key + "vel"][t], 1e-9, msg)
        for i in range(A):
            _close(env.agent_obs(obs, i)[0], z[key + "obs_%d" % i][t], 2e-6, msg + " agent %d" % i)
        _close(rew[0], z[key + "rewards"][t].reshape(A, 1), 1e-6, msg)
        ind = np.array([info[0][j]["individual_reward"] for j in range(A)])
        _close(ind, z[key + "individual_rewards"][t], 1e-6, msg)
        np.testing.assert_array_equal(done[0].cpu().numpy(), z[key + "dones"][t])
        assert bool(done[0].all()) == (t == T - 1)
        # the rewards as the issue states them, from the state
        want = rewards_from_state(env.pos[0].cpu().numpy(), adv)
        _close(ind, want, 1e-9, msg)
        _close(rew[0, :, 0], want, 1e-6, msg)
        seen["caught"] += want[0] > 0
        speed = env.vel[0].norm(dim=-1).cpu().numpy()
        assert (speed <= np.array([1.0] * adv + [1.3] * (A - adv)) + 1e-12).all(), (msg, speed)
        seen["clamped"] += bool((speed > np.array([1.0] * adv + [1.3] * (A - adv)) - 1e-12).any())
    assert seen["clamped"] >= 10, seen                  # the top speed acts in most steps
    if case == CATCH_CASE:          # at least three steps began with the pair inside 0.125, and a catch was paid
        assert seen["pair"] >= 3 and seen["caught"] >= 1, seen
    if case == LANDMARK_CASE:       # at least three steps began with adversary 0 inside the landmark's dist_min
        assert seen["landmark"] >= 3, seen


@pytest.mark.parametrize("case", range(N_CASES))
def test_step_ops_matches_reference_trajectories(gold, case):
    replay_case(gold.npz(CASES), case, ops=True)


def test_fixture_has_the_cases_the_scenario_needs(gold):
    z = gold.npz(CASES)
    shapes = [(int(z["tag%d_num_adversaries" % c]), int(z["tag%d_dims" % c][0]) - int(z["tag%d_num_adversaries" % c]),
               int(z["tag%d_dims" % c][1])) for c in range(N_CASES)]
    assert shapes == SHAPES
    assert "tag%d_dims" % N_CASES not in z
    margin = np.inf
    for c, (adv, good, l) in enumerate(shapes):
        assert z["tag%d_rewards" % c].shape == (T, adv + good, 1)
        assert np.array_equal(z["tag%d_rewards" % c][..., 0], z["tag%d_individual_rewards" % c])      # not shared
        pos = np.concatenate([z["tag%d_pos0" % c][None], z["tag%d_pos" % c]])
        d = np.sqrt(((pos[:, adv:, None] - pos[:, None, :adv]) ** 2).sum(-1))
        margin = min(margin, float(np.abs(d - CATCH).min()))
    assert margin > 1e-6, margin            # whether a pair touches is never a rounding question
    # (a) a catch is paid: +10 to every adversary, -10 to the good agent
    r = z["tag%d_rewards" % CATCH_CASE][..., 0]
    paid = r[:, 0] > 0
    assert paid.sum() >= 1 and (r[paid, :3] == 10.0).all() and (r[paid, 3] <= -10.0).all()
    d0 = np.sqrt(((z["tag%d_pos0" % CATCH_CASE][3] - z["tag%d_pos0" % CATCH_CASE][0]) ** 2).sum())
    assert abs(d0 - 0.1) < 1e-12
    # (b) the landmark holds adversary 0 off: driven at it with 9 every step, it never gets within 0.2 of the centre
    land, p = z["tag%d_landmarks" % LANDMARK_CASE][0], z["tag%d_pos" % LANDMARK_CASE][:, 0]
    assert abs(np.sqrt(((z["tag%d_pos0" % LANDMARK_CASE][0] - land) ** 2).sum()) - 0.22) < 1e-12
    assert (z["tag%d_action_idx" % LANDMARK_CASE][:, 0] == 2).all()
    assert (np.sqrt(((p - land) ** 2).sum(-1)) < 0.275).sum() >= 3
    # (c) good agent 1 passes through the ramp into the exp branch, good agent 2 sits at the cap
    x = np.abs(z["tag%d_pos" % BOUND_CASE][:, 1, 0])
    assert z["tag%d_pos0" % BOUND_CASE][1, 0] == 0.85
    assert ((x > 0.9) & (x < 1.0)).any() and ((x >= 1.0) & (np.exp(2 * x - 2) < 10)).any()
    assert abs(z["tag%d_pos0" % BOUND_CASE][2, 1]) == 2.3
    assert (z["tag%d_rewards" % BOUND_CASE][:, 2, 0] <= -10.0).all()


def test_spaces_widths_and_column_views():
    for (adv, good, l), dims in (((3, 1, 2), (16, 16, 16, 14)), ((2, 2, 2), (18, 18, 16, 16)), ((1, 1, 1), (10, 8))):
        a = adv + good
        env = make(3, adv, good, l)
        assert env.obs_dims == dims == widths(adv, good, l) and env._obs_shape() == (3, sum(dims))
        assert env.state_names == ("pos", "vel", "landmarks", "t") and env.shared_reward is False
        assert [s.shape for s in env.observation_space] == [(d,) for d in dims]
        assert [s.shape for s in env.share_observation_space] == [(sum(dims),)] * a
        assert [(type(s).__name__, s.n) for s in env.action_space] == [("Discrete", 5)] * a
        obs = env.reset()
        assert obs.shape == (3, sum(dims))
        env.vel = torch.arange(3 * a * 2, dtype=torch.float64).reshape(3, a, 2) + 1.0       # tell the velocities apart
        obs = env._obs()
        lo = 0
        for i, d in enumerate(dims):
            view = env.agent_obs(obs, i)
            assert view.shape == (3, d) and view.data_ptr() == obs[:, lo:].data_ptr() and view._base is obs
            assert torch.equal(view[:, 0:2], env.vel[:, i].float()) and torch.equal(view[:, 2:4], env.pos[:, i].float())
            assert torch.equal(view[:, 4:4 + 2 * l], (env.landmarks - env.pos[:, i:i + 1]).reshape(3, -1).float())
            others = [j for j in range(a) if j != i]
            assert torch.equal(view[:, 4 + 2 * l:4 + 2 * l + 2 * (a - 1)],
                               (env.pos[:, others] - env.pos[:, i:i + 1]).reshape(3, -1).float())
            fast = [j for j in others if j >= adv]          # the other good agents' velocities
            assert torch.equal(view[:, 4 + 2 * l + 2 * (a - 1):], env.vel[:, fast].reshape(3, -1).float())
            lo += d
    assert sum(widths(3, 1, 2)) == 62
    assert float(make(64, 3, 1, 2, seed=2).reset()[:, 4:8].abs().max()) <= 1.8               # landmarks at 0.8 U(-1, 1)
    for bad in (dict(num_agents=4, num_adversaries=4), dict(num_agents=4, num_adversaries=0),
                dict(num_agents=1, num_adversaries=1), dict(num_landmarks=0)):
        with pytest.raises(AssertionError, match="simple_tag"):
            TorchSimpleTag(4, **bad)
    default = TorchSimpleTag(2)
    assert (default.a, default.l, default.num_adversaries, default.world_length) == (4, 2, 3, 25)


def test_rewards_are_per_agent_and_follow_the_formulas():
    for adv, good, l in ((3, 1, 2), (2, 2, 2), (1, 1, 1)):
        a = adv + good
        env = make(9, adv, good, l, seed=4)
        env.reset()
        env.pos[0, adv, 0], env.pos[0, adv, 1] = env.pos[0, 0, 0] + 0.12, env.pos[0, 0, 1]      # world 0: a pair that meets
        env.pos[1, adv] = torch.tensor([0.95, -1.4])        # world 1: on the ramp and in the exp branch
        g = torch.Generator().manual_seed(a)
        for step in range(5):
            act = torch.randint(0, 5, (9, a), generator=g)
            if step == 0:
                act[0, 0], act[0, adv] = 1, 2               # into each other: they cross, 0.095 apart after the step
            obs, rew, done, info = env.step(act)
            per_agent = info._per_agent
            assert per_agent.shape == (9, a) and per_agent.dtype == torch.float64
            assert torch.equal(rew[..., 0], per_agent.float())
            want = np.stack([rewards_from_state(env.pos[w].numpy(), adv) for w in range(9)])
            d = (env.pos[:, adv:, None] - env.pos[:, None, :adv]).norm(dim=-1)
            assert float((d - CATCH).abs().min()) > 1e-9
            np.testing.assert_allclose(per_agent.numpy(), want, rtol=1e-12, atol=1e-12)
            if step == 0:
                assert float(per_agent[0, 0]) >= 10.0 and float(per_agent[0, adv]) <= -10.0
                assert float(per_agent[1, adv]) < -0.4
            assert [d["individual_reward"] for d in info[3]] == per_agent[3].tolist()


def test_index_and_one_hot_actions_step_alike():
    n, a = 7, 4
    envs = [make(n, 3, 1, 2, seed=5, world_length=4) for _ in range(4)]
    first = [e.reset() for e in envs]
    assert all(torch.equal(first[0], o) for o in first[1:])
    rng = np.random.default_rng(1)
    for _ in range(9):                                          # crosses two auto-resets
        idx = torch.from_numpy(rng.integers(0, 5, (n, a)))
        one_hot = torch.nn.functional.one_hot(idx, 5).double()
        res = [envs[0].step(idx), envs[1].step(idx[..., None]), envs[2].step(one_hot),
               envs[3].step(one_hot.reshape(n, 5 * a))]
        for other in res[1:]:
            for x, y in zip(res[0][:3], other[:3]):
                assert torch.equal(x, y)
        for name in TorchSimpleTag.state_names:
            assert all(torch.equal(getattr(envs[0], name), getattr(e, name)) for e in envs[1:]), name


def test_action_force_is_the_acceleration_squared_and_the_speed_is_clamped():
    env = make(1, 1, 1, 1, auto_reset=False)
    env.reset()
    env.pos[0] = torch.tensor([[-0.5, -0.5], [0.5, 0.5]])
    env.landmarks[0] = torch.tensor([[0.0, 5.0]])
    env.step(torch.tensor([[1, 4]]))                            # from rest: 9 dt = 0.9 < 1.0, 16 dt = 1.6 > 1.3
    torch.testing.assert_close(env.vel[0], torch.tensor([[0.9, 0.0], [0.0, -1.3]], dtype=torch.float64), rtol=0, atol=1e-15)
    torch.testing.assert_close(env.pos[0], torch.tensor([[-0.41, -0.5], [0.5, 0.37]], dtype=torch.float64), rtol=0,
                               atol=1e-15)
    env.step(torch.tensor([[1, 4]]))                            # 0.75 * 0.9 + 0.9 = 1.575 > 1.0
    torch.testing.assert_close(env.vel[0], torch.tensor([[1.0, 0.0], [0.0, -1.3]], dtype=torch.float64), rtol=0, atol=1e-15)


def test_state_names_and_draw_order():
    """No state besides the particle state; a restart draws agent positions, then landmarks."""
    assert TorchSimpleTag.state_names == ("pos", "vel", "landmarks", "t")
    assert TorchSimpleTag.landmark_scale == 0.8
    env = make(5, 3, 1, 2, seed=11)
    env.reset()
    g = torch.Generator().manual_seed(11)
    pos = torch.empty(5, 4, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    land = torch.empty(5, 2, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    assert torch.equal(env.pos, pos) and torch.equal(env.landmarks, 0.8 * land)
    assert float(env.vel.abs().max()) == 0.0 and int(env.t.abs().max()) == 0
    assert torch.equal(env.rng.get_state(), g.get_state())


def test_reset_in_place_equals_reset_at_fixed_addresses():
    a, b = make(6, 2, 2, 2, seed=8), make(6, 2, 2, 2, seed=8)
    a.reset(), b.reset()
    for _ in range(3):
        act = torch.randint(0, 5, (6, 4))
        a.step(act), b.step(act)
    kept = {k: getattr(b, k) for k in b.state_names}
    oa, ob = a.reset(), b.reset_in_place()
    assert torch.equal(oa, ob)
    for k in a.state_names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert getattr(b, k) is kept[k], k
    assert torch.equal(a.rng.get_state(), b.rng.get_state())


def test_auto_reset_restarts_exactly_the_finished_worlds():
    n, L, a = 16, 6, 4
    env = make(n, 3, 1, 2, seed=3, world_length=L)
    env.reset()
    env.t = torch.arange(n) % L                                                        # staggered episodes
    rng = np.random.default_rng(2)
    restarted = 0
    for _ in range(2 * L):
        before = {k: getattr(env, k).clone() for k in env.state_names}
        state = env.rng.get_state()
        obs, rew, done, info = env.step(torch.from_numpy(rng.integers(1, 5, (n, a))))
        fin = done[:, 0]
        assert bool((done == fin[:, None]).all())
        assert torch.equal(fin, before["t"] + 1 >= L)
        assert bool(fin.any()) and not bool(fin.all())
        restarted += int(fin.sum())
        g = torch.Generator()
        g.set_state(state)
        fresh_pos = torch.empty(n, a, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
        fresh_land = torch.empty(n, 2, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
        assert bool((env.t[fin] == 0).all()) and float(env.vel[fin].abs().max()) == 0.0
        assert torch.equal(env.pos[fin], fresh_pos[fin]) and torch.equal(env.landmarks[fin], 0.8 * fresh_land[fin])
        assert float(obs[fin][:, :2].abs().max()) == 0.0                               # the fresh world's observation
        assert torch.equal(obs[fin][:, 2:4], fresh_pos[fin][:, 0].float())
        go = ~fin
        assert torch.equal(env.t[go], before["t"][go] + 1)
        assert torch.equal(env.landmarks[go], before["landmarks"][go])
        assert float(env.vel[go].abs().sum(-1).min()) > 0.0                            # every movement action pushes
    assert restarted == 2 * n                                                          # every world, twice


def test_an_episode_is_25_steps_whatever_the_episode_length():
    env = make(3, 1, 1, 1, episode_length=10, seed=1)
    assert env.world_length == 25
    env.reset()
    for t in range(1, 27):
        done = env.step(torch.zeros(3, 2, dtype=torch.int64))[2]
        assert bool(done.all()) == (t == 25) and bool(done.any()) == (t == 25), t
    assert env.t.tolist() == [1, 1, 1]
    assert TorchSimpleTag(3, episode_length=40, world_length=7).world_length == 7


def test_coincident_centres_get_no_contact_force():
    """The reference divides by zero there; the project leaves such a pair alone, agent on agent and agent on landmark."""
    env = make(2, 2, 1, 1, seed=6, auto_reset=False)
    env.reset()
    env.pos[0] = torch.tensor([[0.3, 0.3], [-0.6, -0.6], [0.3, 0.3]])      # adversary 0 and the good agent coincide ...
    env.landmarks[0] = torch.tensor([[-0.6, -0.6]])                        # ... and adversary 1 sits on the landmark's centre
    before = env.pos.clone()
    obs, rew, _, _ = env.step(torch.zeros(2, 3, dtype=torch.int64))
    assert torch.isfinite(env.pos).all() and torch.isfinite(env.vel).all() and torch.isfinite(obs).all()
    assert torch.equal(env.pos[0], before[0]) and float(env.vel[0].abs().max()) == 0.0
    assert rew[0, :, 0].tolist() == [10.0, 10.0, -10.0]
    env.pos[0, 1, 0] += 0.1                                                # off the centre: now the landmark pushes
    env.step(torch.zeros(2, 3, dtype=torch.int64))
    assert float(env.vel[0, 1, 0]) > 1.0 - 1e-12 and float(env.vel[0, 1, 1]) == 0.0


# sha256 over state, observations and rewards of ten seeded tensor-op steps, recorded on the commit before
# TorchParticleWorlds took a top speed, per-pair radii, landmark contacts and a per-agent action scale (with torch's AVX2 /
# AVX-512 CPU kernels, which agree; its scalar fall-back rounds logaddexp differently)
PARENT_DIGESTS = {
    "simple_spread": "081d0b75dc338a3a22e01ffac494cc1cd50bda47f96ea77bcb611bf14ea31330",
    "simple_reference": "70b9d61ce22154942729270ecb0554b7a792cd893f620bb90639fd15f9a56a15",
    "simple_speaker_listener": "20f45075ec33b0022a8b97d4a3762fe6769a00a6d30926f9fd426e442f9f294a",
    "simple_push": "28af83a0594a20e47a55a7e8e05cc1e0968240cab81eb63332cce88f14749a0e",
}


def older_scenario_digest(name):
    from onpolicy.envs.mpe.simple_push import TorchSimplePush
    from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
    from onpolicy.envs.mpe.simple_speaker_listener import TorchSimpleSpeakerListener
    from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread
    n = 6
    g = torch.Generator().manual_seed(12)
    env, act = {
        "simple_spread": lambda: (TorchSimpleSpread(n, 3, 3, seed=2, episode_length=4),
                                  lambda: torch.randint(0, 5, (n, 3), generator=g)),
        "simple_reference": lambda: (TorchSimpleReference(n, seed=2, episode_length=4),
                                     lambda: torch.stack([torch.randint(0, 5, (n, 2), generator=g),
                                                          torch.randint(0, 10, (n, 2), generator=g)], -1)),
        "simple_speaker_listener": lambda: (TorchSimpleSpeakerListener(n, seed=2, episode_length=4),
                                            lambda: torch.stack([torch.randint(0, 3, (n,), generator=g),
                                                                 torch.randint(0, 5, (n,), generator=g)], -1)),
        "simple_push": lambda: (TorchSimplePush(n, 3, 2, seed=2, world_length=4),
                                lambda: torch.randint(0, 5, (n, 3), generator=g)),
    }[name]()
    h = hashlib.sha256()
    h.update(env.reset().numpy().tobytes())
    if name in ("simple_spread", "simple_push"):        # a pair in contact, so that the contact force is part of the digest
        env.pos[0, 1] = env.pos[0, 0] + torch.tensor([0.06, 0.01], dtype=torch.float64)
    for _ in range(10):
        obs, rew, done, info = env._step_ops(act())
        for x in (obs, rew, done, info._per_agent) + tuple(getattr(env, k) for k in env.state_names):
            h.update(x.contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", sorted(PARENT_DIGESTS))
def test_older_scenarios_step_bit_identically(name):
    assert older_scenario_digest(name) == PARENT_DIGESTS[name]


def test_new_entry_point_validates_arguments():
    lib = _native.lib()
    name = "mappo_simple_tag_step"
    assert name in _native.SIGNATURES
    fn = getattr(lib, name)
    assert fn(*([None] * 11), 4, 4, 3, 2, 25, 1, None) == -1
    keep = [(ctypes.c_double * 64)() for _ in range(11)]
    ptrs = [ctypes.addressof(b) for b in keep]
    # pos vel landmarks t actions | fresh_pos fresh_landmarks | obs rewards dones per_agent
    for i in (0, 1, 2, 3, 4, 7, 8, 9, 10):                           # every required pointer
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 4, 3, 2, 25, 0, None) == -1, i
    for i in (5, 6):                                                 # the fresh draws: required with auto_reset
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 4, 3, 2, 25, 1, None) == -1, i
    for n, a, adv, l, length in ((0, 4, 3, 2, 25), (-3, 4, 3, 2, 25), (4, 4, 0, 2, 25), (4, 4, 4, 2, 25),
                                 (4, 4, 5, 2, 25), (4, 1, 1, 2, 25), (4, 0, 0, 2, 25), (4, 4, -1, 2, 25),
                                 (4, 4, 3, 0, 25), (4, 4, 3, 2, 0), (4, 17, 17, 2, 25), (4, 4, 3, -1, 25)):
        assert fn(*ptrs, n, a, adv, l, length, 1, None) == -2, (n, a, adv, l, length)
    assert fn(*ptrs, 4, 17, 3, 2, 25, 1, None) == -4                 # MAPPO_E_TOO_MANY: agents
    assert fn(*ptrs, 4, 4, 3, 5, 25, 1, None) == -4                  # ... landmarks
    assert lib.mappo_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "mappo_hip.h")).read()
    assert re.search(r"\bint mappo_simple_tag_step\(", header)
    assert "scenarios/simple_tag.py" in header and re.search(r"#define MAPPO_TAG_MAX_LANDMARKS 4\b", header)
    from onpolicy.envs.mpe import simple_tag
    assert (simple_tag.KERNEL_MAX_AGENTS, simple_tag.KERNEL_MAX_LANDMARKS) == (16, 4)
    assert not make(2, 3, 1, 2).graph_safe                           # CPU tensors: the tensor-op path


def tag_argv(algo, adv=3, good=1, landmarks=2, n=2, steps=100, hidden=16, agents=None, counts=True):
    """The reference's train_mpe.sh family at small sizes."""
    argv = ["--env_name", "MPE", "--algorithm_name", algo, "--experiment_name", "check",
            "--scenario_name", "simple_tag", "--num_agents", str(adv + good if agents is None else agents),
            "--num_landmarks", str(landmarks),
            "--seed", "1", "--n_training_threads", "1", "--n_rollout_threads", str(n), "--num_mini_batch", "1",
            "--episode_length", "25", "--num_env_steps", str(steps), "--ppo_epoch", "2", "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--share_policy", "--hidden_size", str(hidden),
            "--data_chunk_length", "5", "--use_wandb", "--log_interval", "1"]
    return argv + (["--num_adversaries", str(adv), "--num_good_agents", str(good)] if counts else [])


@pytest.mark.parametrize("algo,adv,good", [("mappo", 3, 1), ("rmappo", 3, 1), ("rmappo", 1, 2)])
def test_train_script_with_device_resident_tag_worlds(monkeypatch, tmp_path, algo, adv, good):
    """train_mpe --use_device_env --share_policy for simple_tag end to end (host buffer stand-in, "device" = CPU
    tensors): no external env tree, one policy and buffer per agent with its own widths and its own rewards."""
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
        # 100 steps: two episodes of 25; 3 against 1 without the two flags, which then read as 3 and 1
        runner = train_mpe.main(tag_argv(algo, adv, good, counts=(adv, good) != (3, 1)) + ["--use_device_env"])
        assert type(runner).__module__ == "onpolicy.runner.separated.mpe_runner"
        assert type(runner.envs) is TorchSimpleTag and runner.rollout_graph is None
        assert runner.envs.num_adversaries == adv and runner.envs.a == agents
        dims = widths(adv, good, 2)
        assert len(runner.buffer) == agents
        lo = 0
        for b, d in zip(runner.buffer, dims):
            assert b.obs.shape == (26, 2, d) and b.share_obs.shape == (26, 2, sum(dims))
            assert torch.equal(b.share_obs, runner.buffer[0].share_obs)               # a common share_obs ...
            assert torch.equal(b.share_obs[..., lo:lo + d], b.obs)                    # ... of which the agent's own is a slice
            lo += d
            assert b.actions.shape == (25, 2, 1)
            assert float(b.actions.min()) >= 0 and float(b.actions.max()) <= 4
            assert bool((b.actions == b.actions.round()).all())
            assert torch.isfinite(b.rewards).all()
            assert float(b.masks.min()) == 0.0                                        # the worlds restarted at step 25
        for b in runner.buffer[:adv]:
            assert float(b.rewards.min()) >= 0.0 and torch.equal(b.rewards, runner.buffer[0].rewards)
        for b in runner.buffer[adv:]:
            assert float(b.rewards.max()) <= 0.0
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
    """simple_tag runs under the separated runner with rmappo / mappo / ippo and num_agents = adversaries + good agents."""
    from onpolicy.config import get_config
    from onpolicy.scripts.train import _launch, train_mpe
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    shared = [a for a in tag_argv("mappo") if a != "--share_policy"]
    with pytest.raises(NotImplementedError, match="use_device_env"):
        train_mpe.main(shared + ["--use_device_env"])
    for algo in ("happo", "hatrpo"):
        with pytest.raises(NotImplementedError, match="use_device_env"):
            train_mpe.main(tag_argv(algo) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"not 5 = 3 \+ 1"):
        train_mpe.main(tag_argv("mappo", agents=5) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"not 3 = 3 \+ 1"):          # the flags left out: 3 and 1
        train_mpe.main(tag_argv("mappo", agents=3, counts=False) + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match=r"not 4 = 4 \+ 0"):
        train_mpe.main(tag_argv("mappo", adv=4, good=0) + ["--use_device_env"])
    assert "simple_tag" in train_mpe.DEVICE_ENVS and "simple_tag" in train_mpe.SEPARATED_DEVICE_ENVS
    # a default parse carries neither attribute: the reference's own namespace
    args = train_mpe.parse_args([], get_config())
    assert not hasattr(args, "num_adversaries") and not hasattr(args, "num_good_agents")
    args = train_mpe.parse_args(["--num_adversaries", "2", "--num_good_agents", "2"], get_config())
    assert (args.num_adversaries, args.num_good_agents) == (2, 2)
