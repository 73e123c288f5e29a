"""The device-resident simple_reference (onpolicy/envs/mpe/simple_reference.py, tensor-op path on CPU tensors) against
trajectories of the reference's own particle environment (core.py + environment.py + scenarios/simple_reference.py,
fixtures from tools/make_golden_mpe_reference.py); auto-reset; the train script's --use_device_env route."""
import numpy as np
import pytest
import torch

from onpolicy import _native
from onpolicy.envs.mpe.simple_reference import TorchSimpleReference

T = 25


def _load_case(env, z, key, world=0):
    for name, src in (("pos", "pos0"), ("vel", "vel0"), ("landmarks", "landmarks")):
        getattr(env, name)[world] = torch.from_numpy(np.asarray(z[key + src], dtype=np.float64))
    env.goal[world] = torch.from_numpy(np.asarray(z[key + "goals"], dtype=np.int64))
    env.comm[world] = -1
    env.t[world] = 0


def replay_case(z, case, device="cpu", ops=False):
    """World 0 follows the reference case, world 1 takes random actions (worlds must not interact)."""
    key = "ref%d_" % case
    env = TorchSimpleReference(2, 2, 3, episode_length=T, seed=0, auto_reset=False, device=device)
    assert env.observation_space[0].shape == tuple(z[key + "obs_dim"]) == (21,)
    assert env.share_observation_space[0].shape == tuple(z[key + "share_obs_dim"]) == (42,)
    widths = [int(h - l + 1) for l, h in zip(env.action_space[0].low, env.action_space[0].high)]
    assert widths == list(z[key + "action_dims"]) == [5, 10]
    env.reset()
    _load_case(env, z, key)
    np.testing.assert_allclose(env._obs()[0].cpu().numpy(), z[key + "obs0"], rtol=1e-6, atol=1e-6)
    rng = np.random.default_rng(99)
    step = env._step_ops if ops else env.step                      # (_step_ops: the kernel's own reference)
    for t in range(T):
        other = np.stack([rng.integers(0, 5, 2), rng.integers(0, 10, 2)], -1)
        idx = np.stack([z[key + "action_idx"][t], other]).astype(np.int64)
        obs, rew, done, info = step(torch.from_numpy(idx).to(device))
        assert obs.dtype == torch.float32 and obs.shape == (2, 2, 21) and rew.shape == (2, 2, 1)
        assert done.dtype == torch.bool
        msg = "case %d t=%d" % (case, t)
        np.testing.assert_allclose(env.pos[0].cpu().numpy(), z[key + "pos"][t], rtol=1e-9, atol=1e-9, err_msg=msg)
        np.testing.assert_allclose(obs[0].cpu().numpy(), z[key + "obs"][t], rtol=2e-6, atol=2e-6, err_msg=msg)
        np.testing.assert_allclose(rew[0].cpu().numpy(), z[key + "rewards"][t].reshape(2, 1), rtol=1e-6, atol=1e-6,
                                   err_msg=msg)
        ind = [info[0][j]["individual_reward"] for j in range(2)]
        np.testing.assert_allclose(ind, z[key + "individual_rewards"][t], rtol=1e-6, atol=1e-6, err_msg=msg)
        np.testing.assert_array_equal(done[0].cpu().numpy(), z[key + "dones"][t])
        heard = np.eye(10)[env.comm[0].cpu().numpy()]
        np.testing.assert_array_equal(heard, z[key + "comm"][t])


@pytest.mark.parametrize("case", [0, 1, 2])
def test_step_ops_matches_reference_trajectories(gold, case):
    replay_case(gold.npz("mpe_reference_cases"), case, ops=True)


def _one_hot(idx):
    return np.concatenate([np.eye(5)[idx[..., 0]], np.eye(10)[idx[..., 1]]], -1)


def test_index_and_one_hot_actions_step_alike():
    n = 7
    a = TorchSimpleReference(n, episode_length=4, seed=5)
    b = TorchSimpleReference(n, episode_length=4, seed=5)
    o1, o2 = a.reset(), b.reset()
    assert torch.equal(o1, o2)
    rng = np.random.default_rng(1)
    for _ in range(9):                                          # crosses two auto-resets
        idx = np.stack([rng.integers(0, 5, (n, 2)), rng.integers(0, 10, (n, 2))], -1)
        r1 = a.step(torch.from_numpy(idx))
        r2 = b.step(torch.from_numpy(_one_hot(idx)))
        for x, y in zip(r1[:3], r2[:3]):
            assert torch.equal(x, y)
        for name in TorchSimpleReference.state_names:
            assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_auto_reset_restarts_exactly_the_finished_worlds():
    n, L = 64, 6
    env = TorchSimpleReference(n, episode_length=L, seed=3)
    env.reset()
    env.t = torch.randint(0, L, (n,), generator=torch.Generator().manual_seed(0))     # staggered episodes
    rng = np.random.default_rng(2)
    for _ in range(3):
        before = {k: getattr(env, k).clone() for k in env.state_names}
        idx = torch.from_numpy(np.stack([rng.integers(1, 5, (n, 2)), rng.integers(0, 10, (n, 2))], -1))
        obs, rew, done, info = env.step(idx)
        fin = done[:, 0]
        assert bool((done[:, 0] == done[:, 1]).all())
        assert torch.equal(fin, before["t"] + 1 >= L)
        assert bool(fin.any()) and not bool(fin.all())
        # restarted worlds: fresh state
        assert bool((env.t[fin] == 0).all()) and bool((env.comm[fin] == -1).all())
        assert float(env.vel[fin].abs().max()) == 0.0
        assert bool(((env.goal[fin] >= 0) & (env.goal[fin] <= 2)).all())
        assert float(env.landmarks[fin].abs().max()) <= 0.8 and float(env.pos[fin].abs().max()) <= 1.0
        assert float(obs[fin][..., 11:].abs().max()) == 0.0                       # nobody has spoken yet
        # the others: one step on, their landmarks and goals untouched, this step's symbols heard
        go = ~fin
        assert torch.equal(env.t[go], before["t"][go] + 1)
        assert torch.equal(env.landmarks[go], before["landmarks"][go]) and torch.equal(env.goal[go], before["goal"][go])
        assert torch.equal(env.comm[go], idx[go][..., 1])
        assert float(env.vel[go].abs().sum(-1).min()) > 0.0                       # every movement action pushes
        heard = obs[go][..., 11:].argmax(-1)
        assert torch.equal(heard, idx[go][..., 1].flip(1))


def test_new_entry_points_validate_arguments():
    lib = _native.lib()
    assert lib.mappo_simple_reference_step(*([None] * 14), 4, 25, 1, None) == -1
    assert lib.mappo_multi_categorical_sample(None, None, None, 2, None, None, 4, None) == -1
    assert "mappo_simple_reference_step" in _native.SIGNATURES
    assert "mappo_multi_categorical_sample" in _native.SIGNATURES


def _device_env_argv(algo):
    return ["--env_name", "MPE", "--scenario_name", "simple_reference", "--num_agents", "2", "--num_landmarks", "3",
            "--algorithm_name", algo, "--n_rollout_threads", "4", "--episode_length", "10", "--num_env_steps", "80",
            "--ppo_epoch", "2", "--num_mini_batch", "1", "--data_chunk_length", "5", "--hidden_size", "16",
            "--gain", "0.01", "--lr", "7e-4", "--critic_lr", "7e-4", "--use_wandb", "--log_interval", "1",
            "--n_training_threads", "1"]


@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_train_script_with_device_resident_reference_worlds(monkeypatch, tmp_path, algo):
    """train_mpe --use_device_env for simple_reference end to end (host buffer stand-in, "device" = CPU tensors): no
    external env tree, MultiDiscrete actions stored two wide, finite losses logged."""
    import json
    import os
    import onpolicy.runner.shared.base_runner as base
    from host_buffer import HostSharedBuffer
    from onpolicy.scripts.train import _launch, train_mpe
    threads = torch.get_num_threads()

    def device_of(all_args):
        torch.set_num_threads(all_args.n_training_threads)
        return torch.device("cpu")
    monkeypatch.setattr(base, "SharedReplayBuffer", HostSharedBuffer)
    monkeypatch.setattr(_launch, "device_of", device_of)
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    monkeypatch.delenv("MAPPO_ENVS_PATH", raising=False)
    argv = _device_env_argv(algo)
    try:
        runner = train_mpe.main(argv + ["--use_device_env"])
        assert type(runner.envs).__name__ == "TorchSimpleReference"
        assert runner.buffer.actions.shape[-1] == 2 and runner.buffer.action_log_probs.shape[-1] == 2
        rows = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
        tags = {r["tag"] for r in rows}
        assert {"value_loss", "policy_loss", "average_episode_rewards", "agent0/individual_rewards"} <= tags
        for r in rows:
            if r["tag"] in ("value_loss", "policy_loss", "dist_entropy"):
                assert all(np.isfinite(v) for k, v in r.items() if k not in ("tag", "step")), r
        assert torch.isfinite(runner.buffer.rewards).all() and float(runner.buffer.masks.min()) == 0.0
        acts = runner.buffer.actions.reshape(-1, 2)
        assert float(acts[:, 0].max()) <= 4 and float(acts[:, 1].max()) <= 9 and float(acts.min()) >= 0
    finally:
        torch.set_num_threads(threads)


def test_device_env_still_refuses_the_separated_runner(monkeypatch, tmp_path):
    from onpolicy.scripts.train import _launch, train_mpe
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    with pytest.raises(NotImplementedError, match="use_device_env"):
        train_mpe.main(_device_env_argv("mappo") + ["--use_device_env", "--share_policy"])   # store_false: separated
    with pytest.raises(NotImplementedError, match="use_device_env"):
        train_mpe.main(_device_env_argv("happo") + ["--use_device_env"])
