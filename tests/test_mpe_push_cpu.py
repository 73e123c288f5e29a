"""The device-resident simple_push (onpolicy/envs/mpe/simple_push.py, tensor-op path on CPU tensors) against
trajectories of the reference's own particle environment (core.py + environment.py + scenarios/simple_push.py, fixtures
from tools/make_golden_mpe_push.py: free play and agents driven into contact); rewards that are each agent's own; spaces
and column views; both action forms; draws, resets and the fixed 25-step episode; the new entry point's argument checks;
the train script's --use_device_env route through the separated runner with two and three agents."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from onpolicy import _native
from onpolicy.envs.mpe.simple_push import TorchSimplePush

T = 25
CASES = "mpe_push_cases"
N_CASES = 6                     # 0-3 free play at (A, L) = (2, 2), (2, 2), (3, 2), (4, 1); 4, 5 contacts at (2, 2), (3, 2)
CONTACT_CASES = (4, 5)


def widths(a, l):
    return (2 + 2 * l + 2 * (a - 1),) + (7 + 5 * l + 2 * (a - 1),) * (a - 1)


def _load_case(env, z, key, world=0):
    for name, src in (("pos", "pos0"), ("vel", "vel0"), ("landmarks", "landmarks")):
        getattr(env, name)[world] = torch.from_numpy(np.asarray(z[key + src], dtype=np.float64))
    env.goal[world] = int(z[key + "goal"])
    env.t[world] = 0


def _close(got, want, tol, msg):
    np.testing.assert_allclose(got.cpu().numpy() if torch.is_tensor(got) else got, want, rtol=tol, atol=tol, err_msg=msg)


def replay_case(z, case, device="cpu", ops=False, n=2):
    """World 0 follows the reference case, the other worlds take random actions (worlds must not interact).  Tolerances:
    those of test_mpe_speaker_listener_cpu.replay_case -- state 1e-9, observations 2e-6, rewards 1e-6."""
    key = "push%d_" % case
    A, L = (int(v) for v in z[key + "dims"])
    env = TorchSimplePush(n, A, L, episode_length=T, seed=0, auto_reset=False, device=device)
    dims = widths(A, L)
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
    closest = []
    for t in range(T):
        d = (env.pos[0, :, None] - env.pos[0, None, :]).norm(dim=-1) + 9.0 * torch.eye(A, device=env.pos.device)
        closest.append(float(d.min()))
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
        dist = (env.pos[0] - env.landmarks[0, int(env.goal[0])]).norm(dim=-1).cpu().numpy()
        want = np.concatenate([[dist[1:].min() - dist[0]], -dist[1:]])
        _close(ind, want, 1e-9, msg)
        _close(rew[0, :, 0], want, 1e-6, msg)
    if case in CONTACT_CASES:       # the contact force acted: at least three steps began with a pair closer than 0.1
        assert sum(c < 0.1 for c in closest) >= 3, closest


@pytest.mark.parametrize("case", range(N_CASES))
def test_step_ops_matches_reference_trajectories(gold, case):
    replay_case(gold.npz(CASES), case, ops=True)


def test_fixture_has_the_cases_the_scenario_needs(gold):
    z = gold.npz(CASES)
    shapes = [tuple(int(v) for v in z["push%d_dims" % c]) for c in range(N_CASES)]
    assert shapes == [(2, 2), (2, 2), (3, 2), (4, 1), (2, 2), (3, 2)]
    assert "push%d_dims" % N_CASES not in z
    for c in range(N_CASES):
        assert z["push%d_rewards" % c].shape == (T, shapes[c][0], 1)
        assert np.array_equal(z["push%d_rewards" % c][..., 0], z["push%d_individual_rewards" % c])      # not shared
    for c in CONTACT_CASES:         # the pair flies apart: the contact force outweighs the actions that push them together
        vx = z["push%d_vel" % c][:4, :2, 0]
        assert (vx[2:, 0] > 0.15).all() and (vx[2:, 1] < -0.15).all(), vx


def test_rewards_are_per_agent_and_follow_the_formulas():
    for a, l in ((2, 2), (3, 2), (4, 1)):
        env = TorchSimplePush(9, a, l, seed=4)
        assert env.shared_reward is False
        env.reset()
        g = torch.Generator().manual_seed(a)
        for _ in range(5):
            obs, rew, done, info = env.step(torch.randint(0, 5, (9, a), generator=g))
            per_agent = info._per_agent
            assert per_agent.shape == (9, a) and per_agent.dtype == torch.float64
            for i in range(a):
                assert torch.equal(rew[:, i, 0], per_agent[:, i].float())
            goal_pos = env.landmarks[torch.arange(9), env.goal]                                 # [N, 2]
            dist = (env.pos - goal_pos[:, None]).norm(dim=-1)                                   # [N, A]
            torch.testing.assert_close(per_agent[:, 1:], -dist[:, 1:], rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(per_agent[:, 0], dist[:, 1:].min(-1).values - dist[:, 0], rtol=1e-12, atol=1e-12)
            assert bool((per_agent[:, 1:] < 0).all())
            assert not torch.equal(rew[:, 0], rew[:, 1])                                        # rewards differ between agents
            assert [d["individual_reward"] for d in info[3]] == per_agent[3].tolist()


def test_spaces_widths_and_column_views():
    for (a, l), dims in (((2, 2), (8, 19)), ((3, 2), (10, 21, 21)), ((4, 1), (10, 18, 18, 18)), ((2, 1), (6, 14))):
        env = TorchSimplePush(3, a, l)
        assert env.obs_dims == dims == widths(a, l) and not hasattr(env, "obs_dim")
        assert env._obs_shape() == (3, sum(dims))
        assert [s.shape for s in env.observation_space] == [(d,) for d in dims]
        assert [s.shape for s in env.share_observation_space] == [(sum(dims),)] * a
        assert [(type(s).__name__, s.n) for s in env.action_space] == [("Discrete", 5)] * a
        obs = env.reset()
        assert obs.shape == (3, sum(dims))
        lo = 0
        for i, d in enumerate(dims):
            view = env.agent_obs(obs, i)
            assert view.shape == (3, d) and view.data_ptr() == obs[:, lo:].data_ptr() and view._base is obs
            assert float(view[:, :2].abs().max()) == 0.0                                        # own velocity: at rest
            lo += d
        # a good agent: the goal relative to it (2:4) is one of the landmarks relative to it (7:7 + 2 L), named by its colour
        for i in range(1, a):
            o = env.agent_obs(obs, i)
            colour = torch.full((3, 3), 0.25)
            colour[torch.arange(3), env.goal + 1] = 0.75
            assert torch.equal(o[:, 4:7], colour)
            rel = o[:, 7:7 + 2 * l].reshape(3, l, 2)
            assert torch.equal(o[:, 2:4], rel[torch.arange(3), env.goal])
            palette = torch.full((l, 3), 0.1)
            palette[torch.arange(l), torch.arange(l) + 1] = 0.9
            assert torch.equal(o[:, 7 + 2 * l:7 + 5 * l], palette.reshape(1, -1).expand(3, -1))
        # the adversary sees the other agents where they see it, mirrored
        adv, good = env.agent_obs(obs, 0), env.agent_obs(obs, 1)
        assert torch.equal(adv[:, 2 + 2 * l:4 + 2 * l], -good[:, 7 + 5 * l:9 + 5 * l])
    assert float(TorchSimplePush(64, 2, 2, seed=2).reset()[:, 2:6].abs().max()) <= 1.8    # landmarks at 0.8 U(-1, 1)
    for bad in (dict(num_agents=1), dict(num_landmarks=3), dict(num_landmarks=0)):
        with pytest.raises(AssertionError, match="simple_push"):
            TorchSimplePush(4, **bad)


def test_index_and_one_hot_actions_step_alike():
    n, a = 7, 3
    envs = [TorchSimplePush(n, a, 2, seed=5, world_length=4) for _ in range(4)]
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
        for name in TorchSimplePush.state_names:
            assert all(torch.equal(getattr(envs[0], name), getattr(e, name)) for e in envs[1:]), name


def test_state_names_and_draw_order():
    """goal is part of the declared state; a restart draws agent positions, landmarks, then the goal."""
    assert TorchSimplePush.state_names == ("pos", "vel", "landmarks", "t", "goal")
    assert TorchSimplePush.landmark_scale == 0.8
    env = TorchSimplePush(5, 3, 2, seed=11)
    env.reset()
    g = torch.Generator().manual_seed(11)
    pos = torch.empty(5, 3, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    land = torch.empty(5, 2, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    goal = torch.randint(0, 2, (5,), generator=g)
    assert torch.equal(env.pos, pos) and torch.equal(env.landmarks, 0.8 * land) and torch.equal(env.goal, goal)
    assert env.goal.dtype == torch.int64 and env.goal.shape == (5,)
    assert float(env.vel.abs().max()) == 0.0 and int(env.t.abs().max()) == 0


def test_reset_in_place_equals_reset_at_fixed_addresses():
    a, b = TorchSimplePush(6, 3, 2, seed=8), TorchSimplePush(6, 3, 2, seed=8)
    a.reset(), b.reset()
    for _ in range(3):
        act = torch.randint(0, 5, (6, 3))
        a.step(act), b.step(act)
    kept = {k: getattr(b, k) for k in b.state_names}
    oa, ob = a.reset(), b.reset_in_place()
    assert torch.equal(oa, ob)
    for k in a.state_names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert getattr(b, k) is kept[k], k
    assert torch.equal(a.rng.get_state(), b.rng.get_state())


def test_auto_reset_restarts_exactly_the_finished_worlds():
    n, L, a = 16, 6, 3
    env = TorchSimplePush(n, a, 2, seed=3, world_length=L)
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
        fresh_goal = torch.randint(0, 2, (n,), generator=g)
        assert bool((env.t[fin] == 0).all()) and float(env.vel[fin].abs().max()) == 0.0
        assert torch.equal(env.pos[fin], fresh_pos[fin]) and torch.equal(env.landmarks[fin], 0.8 * fresh_land[fin])
        assert torch.equal(env.goal[fin], fresh_goal[fin])
        assert float(obs[fin][:, :2].abs().max()) == 0.0                               # the fresh world's observation
        go = ~fin
        assert torch.equal(env.t[go], before["t"][go] + 1)
        assert torch.equal(env.landmarks[go], before["landmarks"][go]) and torch.equal(env.goal[go], before["goal"][go])
        assert float(env.vel[go].abs().sum(-1).min()) > 0.0                            # every movement action pushes
        # the rewards are those of the step that ended, not of the fresh world
        assert float(rew.abs().min()) > 0.0
    assert restarted == 2 * n                                                          # every world, twice


def test_an_episode_is_25_steps_whatever_the_episode_length():
    env = TorchSimplePush(3, 2, 2, episode_length=10, seed=1)
    assert env.world_length == 25
    env.reset()
    for t in range(1, 27):
        done = env.step(torch.zeros(3, 2, dtype=torch.int64))[2]
        assert bool(done.all()) == (t == 25) and bool(done.any()) == (t == 25), t
    assert env.t.tolist() == [1, 1, 1]
    assert TorchSimplePush(3, episode_length=40, world_length=7).world_length == 7


def test_coincident_agents_get_no_contact_force():
    """The reference divides by zero there; both paths of simple_spread leave such a pair alone, and so does this."""
    env = TorchSimplePush(2, 3, 2, seed=6, auto_reset=False)
    env.reset()
    env.pos[0, 1] = env.pos[0, 0]
    env.pos[0, 2] = env.pos[0, 0] + 5.0                # far away
    env.step(torch.tensor([[1, 1, 0], [0, 0, 0]]))
    assert torch.isfinite(env.pos).all() and torch.isfinite(env.vel).all()
    assert torch.equal(env.pos[0, 0], env.pos[0, 1])   # the same action, no force between them: still coincident
    torch.testing.assert_close(env.vel[0, 0], torch.tensor([0.5, 0.0], dtype=torch.float64))


def test_other_device_scenarios_keep_the_shared_reward():
    from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
    from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
    from onpolicy.envs.mpe.simple_speaker_listener import TorchSimpleSpeakerListener
    from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread
    assert TorchParticleWorlds.shared_reward is True
    g = torch.Generator().manual_seed(0)
    for env, act in ((TorchSimpleSpread(5, 3, 3, seed=2), lambda: torch.randint(0, 5, (5, 3), generator=g)),
                     (TorchSimpleReference(5, seed=2),
                      lambda: torch.stack([torch.randint(0, 5, (5, 2), generator=g),
                                           torch.randint(0, 10, (5, 2), generator=g)], -1)),
                     (TorchSimpleSpeakerListener(5, seed=2),
                      lambda: torch.stack([torch.randint(0, 3, (5,), generator=g),
                                           torch.randint(0, 5, (5,), generator=g)], -1))):
        assert env.shared_reward is True and "shared_reward" not in type(env).__dict__
        env.reset()
        obs, rew, done, info = env.step(act())
        total = info._per_agent.sum(-1).float()
        for i in range(env.a):
            assert torch.equal(rew[:, i, 0], total)


def test_new_entry_point_validates_arguments():
    lib = _native.lib()
    name = "mappo_simple_push_step"
    assert name in _native.SIGNATURES
    fn = getattr(lib, name)
    assert fn(*([None] * 13), 4, 2, 2, 25, 1, None) == -1
    keep = [(ctypes.c_double * 64)() for _ in range(13)]
    ptrs = [ctypes.addressof(b) for b in keep]
    # pos vel landmarks t goal actions | fresh_pos fresh_landmarks fresh_goal | obs rewards dones per_agent
    for i in (0, 1, 2, 3, 4, 5, 9, 10, 11, 12):                      # every required pointer
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 2, 2, 25, 0, None) == -1, i
    for i in (6, 7, 8):                                              # the fresh draws: required with auto_reset
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 2, 2, 25, 1, None) == -1, i
    for n, a, l, length in ((0, 2, 2, 25), (-3, 2, 2, 25), (4, 1, 2, 25), (4, 0, 2, 25), (4, 2, 0, 25), (4, 2, 3, 25),
                            (4, 2, 2, 0), (4, 17, 3, 25)):
        assert fn(*ptrs, n, a, l, length, 1, None) == -2, (n, a, l, length)
    assert fn(*ptrs, 4, 17, 2, 25, 1, None) == -4                    # MAPPO_E_TOO_MANY
    assert lib.mappo_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "mappo_hip.h")).read()
    assert re.search(r"\bint mappo_simple_push_step\(", header)
    assert "scenarios/simple_push.py" in header


def push_argv(algo, agents=2, landmarks=2, n=2, steps=100, hidden=16):
    """The reference's train_mpe.sh family at small sizes."""
    return ["--env_name", "MPE", "--algorithm_name", algo, "--experiment_name", "check",
            "--scenario_name", "simple_push", "--num_agents", str(agents), "--num_landmarks", str(landmarks),
            "--seed", "1", "--n_training_threads", "1", "--n_rollout_threads", str(n), "--num_mini_batch", "1",
            "--episode_length", "25", "--num_env_steps", str(steps), "--ppo_epoch", "2", "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--share_policy", "--hidden_size", str(hidden),
            "--data_chunk_length", "5", "--use_wandb", "--log_interval", "1"]


@pytest.mark.parametrize("algo,agents", [("mappo", 2), ("rmappo", 2), ("rmappo", 3)])
def test_train_script_with_device_resident_push_worlds(monkeypatch, tmp_path, algo, agents):
    """train_mpe --use_device_env --share_policy for simple_push end to end (host buffer stand-in, "device" = CPU
    tensors): no external env tree, one policy and buffer per agent with its own widths and its own rewards."""
    import onpolicy.runner.separated.base_runner as base
    from host_buffer import HostSeparatedBuffer
    from onpolicy.scripts.train import _launch, train_mpe
    threads = torch.get_num_threads()

    def device_of(all_args):
        torch.set_num_threads(all_args.n_training_threads)
        return torch.device("cpu")
    monkeypatch.setattr(base, "SeparatedReplayBuffer", HostSeparatedBuffer)
    monkeypatch.setattr(_launch, "device_of", device_of)
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    monkeypatch.delenv("MAPPO_ENVS_PATH", raising=False)
    try:
        runner = train_mpe.main(push_argv(algo, agents) + ["--use_device_env"])       # 100 steps: two episodes of 25
        assert type(runner).__module__ == "onpolicy.runner.separated.mpe_runner"
        assert type(runner.envs) is TorchSimplePush and runner.rollout_graph is None
        dims = widths(agents, 2)
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
            assert torch.isfinite(b.rewards).all() and float(b.rewards.abs().max()) > 0.0
            assert float(b.masks.min()) == 0.0                                        # the worlds restarted at step 25
        for b in runner.buffer[1:]:
            assert not torch.equal(b.rewards, runner.buffer[0].rewards)               # rewards are the agents' own
            assert float(b.rewards.max()) <= 0.0                                      # a good agent: -distance
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
    """simple_push runs under the separated runner with rmappo / mappo / ippo and one or two landmarks, nothing else."""
    from onpolicy.scripts.train import _launch, train_mpe
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    shared = [a for a in push_argv("mappo") if a != "--share_policy"]
    with pytest.raises(NotImplementedError, match="use_device_env"):
        train_mpe.main(shared + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match="use_device_env"):
        train_mpe.main(push_argv("happo") + ["--use_device_env"])
    with pytest.raises(NotImplementedError, match="num_landmarks"):
        train_mpe.main(push_argv("mappo", landmarks=3) + ["--use_device_env"])
    assert "simple_push" in train_mpe.DEVICE_ENVS and "simple_push" in train_mpe.SEPARATED_DEVICE_ENVS
