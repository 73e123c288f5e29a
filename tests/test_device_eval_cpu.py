"""``--use_device_eval`` without a device ("device" = CPU tensors, host buffer stand-ins as in test_mpe_env_cpu.py): worlds
that reset in place, the flag's conditions, eval worlds built in-tree for all three device scenarios, and the runners'
tensor eval loop against a loop written here from public pieces."""
import json
import os

import numpy as np
import pytest
import torch

from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
from onpolicy.envs.mpe.simple_speaker_listener import TorchSimpleSpeakerListener
from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread

WORLDS = {"simple_spread": lambda seed: TorchSimpleSpread(5, 3, 3, 4, seed=seed),
          "simple_reference": lambda seed: TorchSimpleReference(5, 2, 3, 4, seed=seed),
          "simple_speaker_listener": lambda seed: TorchSimpleSpeakerListener(5, 2, 3, 4, seed=seed)}


def _actions(env, rng):
    cols = [torch.from_numpy(rng.integers(0, int(h) + 1, (env.n,))) for sp in env.action_space
            for h in (sp.high if sp.__class__.__name__ == "MultiDiscrete" else [sp.n - 1])]
    flat = torch.stack(cols, -1)                                # [N, sum of the agents' action widths]
    return flat if "agent_obs" in dir(env) else flat.reshape(env.n, env.a, -1)


@pytest.mark.parametrize("scenario", sorted(WORLDS))
def test_reset_in_place_is_reset_at_fixed_addresses(scenario):
    a, b = WORLDS[scenario](7), WORLDS[scenario](7)
    assert set(("pos", "vel", "landmarks", "t")) <= set(a.state_names)

    def same():
        for name in a.state_names:
            x, y = getattr(a, name), getattr(b, name)
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), name
    o1, o2 = a.reset(), b.reset_in_place()
    assert o1.dtype == o2.dtype and torch.equal(o1, o2)
    same()
    ptrs = {name: getattr(b, name).data_ptr() for name in b.state_names}
    rng = np.random.default_rng(0)
    for _ in range(3):
        act = _actions(a, rng)
        ra, rb = a.step(act), b.step(act.clone())
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2])
    if b.graph_safe:         # (the tensor-op step of a CPU device rebinds: the addresses to keep are the current ones)
        assert ptrs == {name: getattr(b, name).data_ptr() for name in b.state_names}
    ptrs = {name: getattr(b, name).data_ptr() for name in b.state_names}
    o1, o2 = a.reset(), b.reset_in_place()
    assert torch.equal(o1, o2) and float(o1.abs().sum()) > 0
    same()
    assert ptrs == {name: getattr(b, name).data_ptr() for name in b.state_names}
    assert int(b.t.sum()) == 0 and float(b.vel.abs().sum()) == 0.0
    # ... and the generators stand where they stood: the next draws agree too
    assert torch.equal(a.reset(), b.reset_in_place())


def _cpu(monkeypatch, tmp_path):
    import onpolicy.runner.separated.base_runner as sep_base
    import onpolicy.runner.shared.base_runner as base
    from host_buffer import HostSeparatedBuffer, HostSharedBuffer
    from onpolicy.scripts.train import _launch

    def device_of(all_args):
        torch.set_num_threads(all_args.n_training_threads)
        return torch.device("cpu")
    monkeypatch.setattr(base, "SharedReplayBuffer", HostSharedBuffer)
    monkeypatch.setattr(sep_base, "SeparatedReplayBuffer", HostSeparatedBuffer)
    monkeypatch.setattr(_launch, "device_of", device_of)
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    monkeypatch.delenv("MAPPO_ENVS_PATH", raising=False)


@pytest.fixture
def threads():
    n = torch.get_num_threads()
    yield
    torch.set_num_threads(n)


def _argv(scenario, algo):
    agents = "3" if scenario == "simple_spread" else "2"
    argv = ["--env_name", "MPE", "--scenario_name", scenario, "--num_agents", agents, "--num_landmarks", "3",
            "--algorithm_name", algo, "--n_rollout_threads", "4", "--episode_length", "10", "--num_env_steps", "120",
            "--ppo_epoch", "2", "--num_mini_batch", "1", "--data_chunk_length", "5", "--hidden_size", "16",
            "--use_wandb", "--log_interval", "1", "--n_training_threads", "1"]
    return argv + (["--share_policy"] if scenario == "simple_speaker_listener" else [])      # store_false: separated


EVAL = ["--use_device_env", "--use_eval", "--use_device_eval", "--eval_interval", "2", "--n_eval_rollout_threads", "2"]


def _rows(runner):
    return [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]


def test_flag_is_absent_by_default_and_refuses_what_it_cannot_do(monkeypatch, tmp_path, threads):
    from onpolicy.config import get_config
    from onpolicy.scripts.train import train_mpe
    assert not hasattr(train_mpe.parse_args([], get_config()), "use_device_eval")
    assert train_mpe.parse_args(["--use_device_eval"], get_config()).use_device_eval is True
    _cpu(monkeypatch, tmp_path)
    base = _argv("simple_spread", "mappo")
    with pytest.raises(NotImplementedError, match="use_device_eval"):
        train_mpe.main(base + ["--use_device_env", "--use_device_eval"])                       # no --use_eval
    with pytest.raises(NotImplementedError, match="use_device_eval"):
        train_mpe.main(base + ["--use_eval", "--use_device_eval"])                             # no --use_device_env
    with pytest.raises(NotImplementedError, match="use_device_eval"):
        train_mpe.main(_argv("simple_spread", "happo") + EVAL)


@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_simple_spread_eval_worlds_on_the_device(monkeypatch, tmp_path, threads, algo):
    from onpolicy.scripts.train import train_mpe
    _cpu(monkeypatch, tmp_path)
    runner = train_mpe.main(_argv("simple_spread", algo) + EVAL)
    assert type(runner.envs).__name__ == "TorchSimpleSpread"
    assert type(runner.eval_envs).__name__ == "TorchSimpleSpread" and runner.eval_envs is not runner.envs
    assert runner.eval_envs.n == 2 and runner.eval_graph is None           # a CPU device: the eager tensor loop
    assert runner.trainer.policy.actor.act.fused_mode is True
    evals = [r for r in _rows(runner) if r["tag"] == "eval_average_episode_rewards"]
    assert len(evals) == 2 and all(np.isfinite(r["eval_average_episode_rewards"]) for r in evals)   # episodes 0 and 2
    assert tuple(runner.eval_totals.shape) == (2, 3, 1) and float(runner.eval_totals.max()) < 0.0
    # without the new flag: the parent's worlds, the parent's policies
    runner = train_mpe.main(_argv("simple_spread", algo) + [a for a in EVAL if a != "--use_device_eval"])
    assert type(runner.eval_envs).__name__ == "VecSimpleSpread" and not hasattr(runner, "eval_graph")
    assert runner.trainer.policy.actor.act.fused_mode is False


def test_simple_reference_evaluates_without_an_external_tree(monkeypatch, tmp_path, threads):
    from onpolicy.scripts.train import train_mpe
    _cpu(monkeypatch, tmp_path)
    runner = train_mpe.main(_argv("simple_reference", "rmappo") + EVAL)
    assert type(runner).__module__ == "onpolicy.runner.shared.mpe_runner"
    assert type(runner.eval_envs) is TorchSimpleReference
    evals = [r for r in _rows(runner) if r["tag"] == "eval_average_episode_rewards"]
    assert len(evals) == 2 and all(np.isfinite(r["eval_average_episode_rewards"]) for r in evals)


def test_simple_speaker_listener_evaluates_without_an_external_tree(monkeypatch, tmp_path, threads):
    from onpolicy.scripts.train import train_mpe
    _cpu(monkeypatch, tmp_path)
    runner = train_mpe.main(_argv("simple_speaker_listener", "rmappo") + EVAL)
    assert type(runner).__module__ == "onpolicy.runner.separated.mpe_runner"
    assert type(runner.eval_envs) is TorchSimpleSpeakerListener and runner.eval_graph is None
    rows = _rows(runner)
    for agent in (0, 1):
        tag = "agent%d/eval_average_episode_rewards" % agent
        evals = [r[tag] for r in rows if r["tag"] == tag]
        assert len(evals) == 2 and all(np.isfinite(v) and v < 0.0 for v in evals), (tag, evals)
    # the reward is shared: both agents' totals are the same numbers
    assert torch.equal(runner.eval_totals[:, 0], runner.eval_totals[:, 1])


@pytest.mark.parametrize("algo", ["rmappo", "mappo"])
def test_shared_eval_logs_what_a_hand_written_loop_gives(monkeypatch, tmp_path, threads, algo):
    from onpolicy.scripts.train import train_mpe
    _cpu(monkeypatch, tmp_path)
    runner = train_mpe.main(_argv("simple_spread", algo) + EVAL)
    n, A, T = 2, 3, runner.episode_length
    runner.eval_envs, twin = TorchSimpleSpread(n, A, 3, T, seed=321), TorchSimpleSpread(n, A, 3, T, seed=321)
    for call in range(2):               # the second call resets worlds that have run
        runner.eval(1000 + call)
        logged = [r for r in _rows(runner) if r["step"] == 1000 + call]
        assert len(logged) == 1
        policy = runner.trainer.policy
        with torch.no_grad():
            obs = twin.reset()
            rnn = torch.zeros(n * A, runner.recurrent_N, runner.hidden_size)
            masks = torch.ones(n * A, 1)
            total = torch.zeros(n, A, 1)
            for _ in range(T):
                act, rnn = policy.act(obs.reshape(n * A, -1), rnn, masks, deterministic=True)
                obs, rewards, dones, _ = twin.step(act.reshape(n, A, 1))
                total = total + rewards
                masks = (~dones).to(torch.float32).reshape(n * A, 1)
                rnn = rnn * masks.view(-1, 1, 1)
        assert torch.equal(runner.eval_totals, total)
        assert logged[0]["eval_average_episode_rewards"] == float(np.mean(total.numpy()))
        assert bool(dones.all())          # the episode ended inside the loop: masks and RNN states were reset once
    assert algo != "rmappo" or float(rnn.abs().sum()) == 0.0


@pytest.mark.parametrize("algo", ["rmappo", "mappo"])
def test_separated_eval_logs_what_a_hand_written_loop_gives(monkeypatch, tmp_path, threads, algo):
    from onpolicy.scripts.train import train_mpe
    _cpu(monkeypatch, tmp_path)
    runner = train_mpe.main(_argv("simple_speaker_listener", algo) + EVAL)
    n, T = 2, runner.episode_length
    runner.eval_envs = TorchSimpleSpeakerListener(n, 2, 3, T, seed=321)
    twin = TorchSimpleSpeakerListener(n, 2, 3, T, seed=321)
    runner.eval(1000)
    rows = [r for r in _rows(runner) if r["step"] == 1000]
    assert len(rows) == 2
    with torch.no_grad():
        obs = twin.reset()
        rnn = [torch.zeros(n, runner.recurrent_N, runner.hidden_size) for _ in range(2)]
        masks = torch.ones(n, 2)
        total = torch.zeros(n, 2, 1)
        for _ in range(T):
            acts = []
            for i, tr in enumerate(runner.trainer):
                act, rnn[i] = tr.policy.act(twin.agent_obs(obs, i), rnn[i], masks[:, i:i + 1], deterministic=True)
                acts.append(act)
            obs, rewards, dones, _ = twin.step(torch.cat(acts, -1))
            total = total + rewards
            masks = (~dones).to(torch.float32)
            rnn = [h * masks[:, i].view(-1, 1, 1) for i, h in enumerate(rnn)]
    assert torch.equal(runner.eval_totals, total)
    for i in range(2):
        tag = "agent%d/eval_average_episode_rewards" % i
        assert [r[tag] for r in rows if r["tag"] == tag] == [float(np.mean(total.numpy()[:, i]))]
