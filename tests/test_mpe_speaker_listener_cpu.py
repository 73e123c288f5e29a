"""The device-resident simple_speaker_listener (onpolicy/envs/mpe/simple_speaker_listener.py, tensor-op path on CPU
tensors) against trajectories of the reference's own particle environment (core.py + environment.py +
scenarios/simple_speaker_listener.py, fixtures from tools/make_golden_mpe_speaker_listener.py); both action forms;
auto-reset; the new entry point's argument checks; the train script's --use_device_env route through the separated
runner."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from onpolicy import _native
from onpolicy.envs.mpe.simple_speaker_listener import TorchSimpleSpeakerListener

T = 25
CASES = "mpe_speaker_listener_cases"


def _load_case(env, z, key, world=0):
    for name, src in (("pos", "pos0"), ("vel", "vel0"), ("landmarks", "landmarks")):
        getattr(env, name)[world] = torch.from_numpy(np.asarray(z[key + src], dtype=np.float64))
    env.goal[world] = int(z[key + "goal"])
    env.comm[world] = -1
    env.t[world] = 0


def _close(got, want, tol, msg):
    np.testing.assert_allclose(got.cpu().numpy() if torch.is_tensor(got) else got, want, rtol=tol, atol=tol, err_msg=msg)


def replay_case(z, case, device="cpu", ops=False, n=2):
    """World 0 follows the reference case, the other worlds take random actions (worlds must not interact).  Tolerances:
    those of test_mpe_reference_cpu.replay_case for simple_reference."""
    key = "spk%d_" % case
    env = TorchSimpleSpeakerListener(n, 2, 3, episode_length=T, seed=0, auto_reset=False, device=device)
    assert env.obs_dims == tuple(z[key + "obs_dims"]) == (3, 11)
    assert [s.shape for s in env.observation_space] == [(3,), (11,)]
    assert [s.shape for s in env.share_observation_space] == [tuple(z[key + "share_obs_dim"])] * 2 == [(14,)] * 2
    assert [s.n for s in env.action_space] == list(z[key + "action_dims"]) == [3, 5]
    assert [type(s).__name__ for s in env.action_space] == ["Discrete", "Discrete"]
    obs = env.reset()
    assert obs.shape == (n, 14) and obs.dtype == torch.float32
    _load_case(env, z, key)
    obs = env._obs()
    _close(env.agent_obs(obs, 0)[0], z[key + "obs0_speaker"], 2e-6, "obs0 speaker")
    _close(env.agent_obs(obs, 1)[0], z[key + "obs0_listener"], 2e-6, "obs0 listener")
    rng = np.random.default_rng(99)
    step = env._step_ops if ops else env.step                      # (_step_ops: the kernel's own reference)
    pos0 = z[key + "pos0"]
    for t in range(T):
        other = np.stack([rng.integers(0, 3, n - 1), rng.integers(0, 5, n - 1)], -1)
        idx = np.concatenate([z[key + "action_idx"][t][None], other]).astype(np.int64)
        obs, rew, done, info = step(torch.from_numpy(idx).to(device))
        assert obs.dtype == torch.float32 and obs.shape == (n, 14)
        assert rew.dtype == torch.float32 and rew.shape == (n, 2, 1)
        assert done.dtype == torch.bool and done.shape == (n, 2)
        msg = "case %d t=%d" % (case, t)
        _close(env.pos[0], z[key + "pos"][t], 1e-9, msg)
        assert np.array_equal(env.pos[0, 0].cpu().numpy(), pos0[0]), msg          # the speaker never moves
        assert float(env.vel[0, 0].abs().max()) == 0.0, msg
        _close(env.agent_obs(obs, 0)[0], z[key + "obs_speaker"][t], 2e-6, msg)
        _close(env.agent_obs(obs, 1)[0], z[key + "obs_listener"][t], 2e-6, msg)
        _close(rew[0], z[key + "rewards"][t].reshape(2, 1), 1e-6, msg)
        ind = [info[0][j]["individual_reward"] for j in range(2)]
        _close(np.array(ind), z[key + "individual_rewards"][t], 1e-6, msg)
        np.testing.assert_array_equal(done[0].cpu().numpy(), z[key + "dones"][t])
        np.testing.assert_array_equal(np.eye(3)[int(env.comm[0])], z[key + "comm"][t])
        # the reward as the issue states it: -d2 each, -2 d2 shared
        d2 = float(((env.pos[0, 1] - env.landmarks[0, int(env.goal[0])]) ** 2).sum())
        _close(np.array(ind), [-d2, -d2], 1e-9, msg)
        _close(rew[0, :, 0], [-2 * d2, -2 * d2], 1e-6, msg)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_step_ops_matches_reference_trajectories(gold, case):
    replay_case(gold.npz(CASES), case, ops=True)


def one_hot(idx):
    return np.concatenate([np.eye(3)[idx[..., 0]], np.eye(5)[idx[..., 1]]], -1)


def test_index_and_one_hot_actions_step_alike():
    n = 7
    a = TorchSimpleSpeakerListener(n, episode_length=4, seed=5)
    b = TorchSimpleSpeakerListener(n, episode_length=4, seed=5)
    c = TorchSimpleSpeakerListener(n, episode_length=4, seed=5)
    o1, o2, o3 = a.reset(), b.reset(), c.reset()
    assert torch.equal(o1, o2) and torch.equal(o1, o3)
    rng = np.random.default_rng(1)
    for _ in range(9):                                          # crosses two auto-resets
        idx = np.stack([rng.integers(0, 3, n), rng.integers(0, 5, n)], -1)
        r1 = a.step(torch.from_numpy(idx))
        r2 = b.step(torch.from_numpy(one_hot(idx)))
        r3 = c.step(torch.from_numpy(idx)[..., None])           # [N, 2, 1]
        assert r2[0].shape == (n, 14)
        for x, y, z in zip(r1[:3], r2[:3], r3[:3]):
            assert torch.equal(x, y) and torch.equal(x, z)
        for name in TorchSimpleSpeakerListener.state_names:
            assert torch.equal(getattr(a, name), getattr(b, name)), name
            assert torch.equal(getattr(a, name), getattr(c, name)), name


def test_state_names_and_draw_order():
    """goal and comm are part of the declared state; a restart draws agent positions, landmarks, then the goal."""
    assert TorchSimpleSpeakerListener.state_names == ("pos", "vel", "landmarks", "t", "goal", "comm")
    env = TorchSimpleSpeakerListener(5, seed=11)
    env.reset()
    g = torch.Generator().manual_seed(11)
    pos = torch.empty(5, 2, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    land = torch.empty(5, 3, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    goal = torch.randint(0, 3, (5,), generator=g)
    assert torch.equal(env.pos, pos) and torch.equal(env.landmarks, land) and torch.equal(env.goal, goal)
    assert env.goal.dtype == env.comm.dtype == torch.int64 and env.goal.shape == env.comm.shape == (5,)
    assert bool((env.comm == -1).all())
    with pytest.raises(AssertionError):
        TorchSimpleSpeakerListener(4, num_agents=3)
    with pytest.raises(AssertionError):
        TorchSimpleSpeakerListener(4, num_landmarks=2)


def test_auto_reset_restarts_exactly_the_finished_worlds():
    n, L = 16, 6
    env = TorchSimpleSpeakerListener(n, episode_length=L, seed=3)
    env.reset()
    env.t = torch.arange(n) % L                                                        # staggered episodes
    rng = np.random.default_rng(2)
    palette = torch.tensor([[0.65, 0.15, 0.15], [0.15, 0.65, 0.15], [0.15, 0.15, 0.65]])
    restarted = 0
    for _ in range(2 * L):
        before = {k: getattr(env, k).clone() for k in env.state_names}
        state = env.rng.get_state()
        idx = torch.from_numpy(np.stack([rng.integers(0, 3, n), rng.integers(1, 5, n)], -1))
        obs, rew, done, info = env.step(idx)
        fin = done[:, 0]
        assert bool((done[:, 0] == done[:, 1]).all())
        assert torch.equal(fin, before["t"] + 1 >= L)
        assert bool(fin.any()) and not bool(fin.all())
        restarted += int(fin.sum())
        # restarted worlds: fresh state, a silent channel, a fresh goal (the draw this step made for the world)
        g = torch.Generator()
        g.set_state(state)
        torch.empty(n, 2, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
        torch.empty(n, 3, 2, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
        fresh_goal = torch.randint(0, 3, (n,), generator=g)
        assert bool((env.t[fin] == 0).all()) and bool((env.comm[fin] == -1).all())
        assert float(env.vel[fin].abs().max()) == 0.0
        assert torch.equal(env.goal[fin], fresh_goal[fin])
        assert float(env.landmarks[fin].abs().max()) <= 1.0 and float(env.pos[fin].abs().max()) <= 1.0
        # columns 8:11 of the listener's observation (11:14 of the row): nobody has spoken yet
        assert float(env.agent_obs(obs, 1)[fin][:, 8:11].abs().max()) == 0.0 == float(obs[fin][:, 11:14].abs().max())
        assert torch.equal(env.agent_obs(obs, 0)[fin], palette[env.goal[fin]])
        # the others: one step on, their landmarks, goal and speaker untouched, this step's symbol heard
        go = ~fin
        assert torch.equal(env.t[go], before["t"][go] + 1)
        assert torch.equal(env.landmarks[go], before["landmarks"][go]) and torch.equal(env.goal[go], before["goal"][go])
        assert torch.equal(env.pos[go][:, 0], before["pos"][go][:, 0])
        assert torch.equal(env.comm[go], idx[go][:, 0])
        assert float(env.vel[go][:, 1].abs().sum(-1).min()) > 0.0                  # every movement action pushes
        heard = env.agent_obs(obs, 1)[go][:, 8:11]
        assert torch.equal(heard, torch.nn.functional.one_hot(idx[go][:, 0], 3).float())
    assert restarted == 2 * n                                                      # every world, twice


def test_other_device_worlds_keep_their_attributes():
    """The per-agent widths live in the base class; the scenarios with one width are as they were."""
    from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
    from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread
    for env, dim in ((TorchSimpleSpread(3, 3, 3), 18), (TorchSimpleReference(3), 21)):
        assert env.obs_dim == dim and env._obs_shape() == (3, env.a, dim)
        assert [s.shape for s in env.observation_space] == [(dim,)] * env.a
        assert [s.shape for s in env.share_observation_space] == [(dim * env.a,)] * env.a
        assert env.reset().shape == (3, env.a, dim) and env._movable is None and not hasattr(env, "agent_obs")


def test_new_entry_point_validates_arguments():
    lib = _native.lib()
    name = "mappo_simple_speaker_listener_step"
    assert name in _native.SIGNATURES
    assert _native.SIGNATURES[name] == _native.SIGNATURES["mappo_simple_reference_step"]
    fn = getattr(lib, name)
    assert fn(*([None] * 14), 4, 25, 1, None) == -1
    import ctypes
    keep = [(ctypes.c_double * 64)() for _ in range(14)]
    ptrs = [ctypes.addressof(b) for b in keep]
    for i in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13):                  # every required pointer
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 25, 0, None) == -1, i
    for i in (7, 8, 9):                                              # the fresh draws: required with auto_reset
        assert fn(*[None if j == i else q for j, q in enumerate(ptrs)], 4, 25, 1, None) == -1, i
    assert fn(*ptrs, 0, 25, 1, None) == -2 and fn(*ptrs, -3, 25, 1, None) == -2
    assert fn(*ptrs, 4, 0, 1, None) == -2
    assert lib.mappo_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "mappo_hip.h")).read()
    assert re.search(r"\bint mappo_simple_speaker_listener_step\(", header)
    assert "scenarios/simple_speaker_listener.py" in header


def comm_argv(algo, n=4, t=10, steps=80, hidden=16):
    """The reference's train_mpe_comm.sh at small sizes."""
    return ["--env_name", "MPE", "--algorithm_name", algo, "--experiment_name", "check",
            "--scenario_name", "simple_speaker_listener", "--num_agents", "2", "--num_landmarks", "3", "--seed", "1",
            "--n_training_threads", "1", "--n_rollout_threads", str(n), "--num_mini_batch", "1",
            "--episode_length", str(t), "--num_env_steps", str(steps), "--ppo_epoch", "2", "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--share_policy", "--hidden_size", str(hidden),
            "--data_chunk_length", "5", "--use_wandb", "--log_interval", "1"]


@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_train_script_with_device_resident_speaker_listener_worlds(monkeypatch, tmp_path, algo):
    """train_mpe --use_device_env --share_policy for simple_speaker_listener end to end (host buffer stand-in, "device" =
    CPU tensors): no external env tree, one policy and buffer per agent with its own widths, finite losses logged."""
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
        runner = train_mpe.main(comm_argv(algo) + ["--use_device_env"])
        assert type(runner).__module__ == "onpolicy.runner.separated.mpe_runner"
        assert type(runner.envs) is TorchSimpleSpeakerListener and runner.rollout_graph is None
        b0, b1 = runner.buffer
        assert b0.obs.shape == (11, 4, 3) and b1.obs.shape == (11, 4, 11)
        assert b0.share_obs.shape == b1.share_obs.shape == (11, 4, 14)
        assert torch.equal(b0.share_obs, b1.share_obs)
        assert torch.equal(b0.share_obs[..., :3], b0.obs) and torch.equal(b1.share_obs[..., 3:], b1.obs)
        for b, top in ((b0, 2), (b1, 4)):
            assert b.actions.shape == (10, 4, 1)
            assert float(b.actions.min()) >= 0 and float(b.actions.max()) <= top
            assert bool((b.actions == b.actions.round()).all())
            assert torch.isfinite(b.rewards).all() and float(b.rewards.max()) <= 0.0
            assert float(b.masks.min()) == 0.0                           # 80 steps = two episodes of 10: worlds restarted
        assert float(b1.actions.max()) > 2                                # (the listener's head is the wider one)
        assert torch.equal(b0.rewards, b1.rewards) and float(b0.rewards.abs().max()) > 0.0
        rows = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
        tags = {r["tag"] for r in rows}
        for agent in (0, 1):
            want = {"agent%d/%s" % (agent, k) for k in ("value_loss", "policy_loss", "dist_entropy",
                                                        "average_episode_rewards", "individual_rewards")}
            assert want <= tags, sorted(tags)
        losses = [r for r in rows if r["tag"].split("/")[-1] in ("value_loss", "policy_loss", "dist_entropy")]
        assert len(losses) == 2 * 3 * 2                                   # agents x tags x episodes
        for r in rows:
            assert all(np.isfinite(v) for k, v in r.items() if k not in ("tag", "step")), r
    finally:
        torch.set_num_threads(threads)


def test_device_env_refusals_stand(monkeypatch, tmp_path):
    """Only simple_speaker_listener + separated runner + rmappo / mappo / ippo is new."""
    from onpolicy.scripts.train import _launch, train_mpe
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    for algo in ("happo", "hatrpo"):
        with pytest.raises(NotImplementedError, match="use_device_env"):
            train_mpe.main(comm_argv(algo) + ["--use_device_env"])
    for scenario in ("simple_spread", "simple_reference", "simple_adversary"):
        argv = comm_argv("mappo")
        argv[argv.index("--scenario_name") + 1] = scenario
        with pytest.raises(NotImplementedError, match="use_device_env"):
            train_mpe.main(argv + ["--use_device_env"])
    argv = [a for a in comm_argv("mappo") if a != "--share_policy"]       # the shared runner cannot take this scenario
    with pytest.raises(AssertionError, match="can not use shared policy"):
        train_mpe.main(argv + ["--use_device_env"])
