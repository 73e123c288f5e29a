"""-m gpu: simple_adversary with its worlds on the device.  The step kernel (``mappo_simple_adversary_step``, one
lane-per-entity kernel for 2 to 64 agents) against the tensor-op step in float64; the separated runner's rollout replayed
from one captured graph against its eager loop; the train script end to end."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("agents,landmarks,worlds", [
    (2, 1, 1),          # the smallest shape
    (3, 2, 65),         # the script's shape: 8 worlds per workgroup, and a ninth workgroup with one
    (32, 31, 3),        # a full 32-lane world
    (33, 32, 5),        # the first shape on 64 lanes, a partly filled workgroup
    (64, 63, 2),        # every lane busy
    (3, 40, 7),         # landmark lanes far past the agent lanes, 64 lanes
    (20, 1, 9)])        # one landmark, idle landmark lanes
def test_step_kernel_equals_tensor_ops(agents, landmarks, worlds):
    """Every step on its own against ``_step_ops`` in float64 from the same seed and the same state (the reference's state
    is copied into the kernel's tensors after each step): worlds of 2 steps over 5, so two restarts with fresh goals.
    State and per_agent to 1e-12 (a handful of float64 operations on values below 10), float32 outputs to 1e-6, dones / t
    / goal equal.  The row is written between NaN canaries, and the state tensors stay where they are."""
    from onpolicy.envs.mpe.simple_adversary import TorchSimpleAdversary
    a, b = (TorchSimpleAdversary(worlds, agents, landmarks=landmarks, seed=5, device=DEV, world_length=2)
            for _ in range(2))
    assert a.graph_safe and (a.a, a.l) == (agents, landmarks)
    assert torch.equal(a.reset(), b.reset())
    where = [getattr(a, name).data_ptr() for name in a.state_names]
    width, pad = sum(a.obs_dims), 16
    g = torch.Generator(device=DEV).manual_seed(1)
    restarts = 0
    for step in range(5):
        act = torch.randint(0, 5, (worlds, agents), generator=g, device=DEV)
        flat = torch.full((worlds * width + 2 * pad,), float("nan"), device=DEV)
        obs = flat[pad:pad + worlds * width].view(worlds, width)
        rew = torch.full((worlds, agents, 1), float("nan"), device=DEV)
        dones = torch.empty(worlds, agents, dtype=torch.bool, device=DEV)
        per_agent = torch.full((worlds, agents), float("nan"), dtype=torch.float64, device=DEV)
        a._launch(act, a._fresh(), obs, rew, dones, per_agent)
        want = b._step_ops(act)
        assert bool(flat[:pad].isnan().all()) and bool(flat[-pad:].isnan().all()), "the row writer left its rows"
        got = dict(pos=a.pos, vel=a.vel, landmarks=a.landmarks, per_agent=per_agent)
        ref = dict(pos=b.pos, vel=b.vel, landmarks=b.landmarks, per_agent=want[3]._per_agent)
        torch.testing.assert_close(obs, want[0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(rew, want[1], rtol=1e-6, atol=1e-6)
        assert torch.equal(dones, want[2]) and torch.equal(a.t, b.t) and torch.equal(a.goal, b.goal)
        for name in got:
            torch.testing.assert_close(got[name], ref[name], rtol=0, atol=1e-12, msg=lambda m: name + ": " + m)
        restarts += int(dones[0, 0])
        for name in a.state_names:
            getattr(a, name).copy_(getattr(b, name))
    assert restarts == 2 and where == [getattr(a, name).data_ptr() for name in a.state_names]
    obs = a.step(torch.nn.functional.one_hot(act, 5).float())[0]              # the public route, one-hot actions
    torch.testing.assert_close(obs, b._step_ops(act)[0], rtol=1e-6, atol=1e-6)


def _run(tmp_path, monkeypatch, graph, n, episodes, algo="rmappo"):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / ("results" + graph)))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    argv = ("--env_name MPE --algorithm_name %s --experiment_name check --scenario_name simple_adversary --num_agents 3 "
            "--num_landmarks 2 --seed 1 --n_training_threads 1 --n_rollout_threads %d --num_mini_batch 1 --episode_length 25 "
            "--num_env_steps %d --ppo_epoch 2 --gain 0.01 --lr 7e-4 --critic_lr 7e-4 --share_policy --hidden_size 64 "
            "--data_chunk_length 5 --use_wandb --log_interval 1 --use_device_env" % (algo, n, episodes * n * 25)).split()
    threads = torch.get_num_threads()
    try:
        return train_mpe.main(argv)
    finally:
        torch.set_num_threads(threads)      # (--n_training_threads 1 sets the process's thread count)


def test_captured_rollout_equals_eager_rollout(tmp_path, monkeypatch):
    """The separated rollout replayed from one captured graph leaves in every agent's buffer what the eager loop leaves,
    bit for bit."""
    captured, eager = _run(tmp_path, monkeypatch, "1", 8, 1), _run(tmp_path, monkeypatch, "0", 8, 1)
    rg = captured.rollout_graph
    assert type(captured.envs).__name__ == "TorchSimpleAdversary" and len(captured.buffer) == 3
    assert rg is not None and rg.graph is not None, "the rollout step was not captured"
    assert rg.replays == 25 and eager.rollout_graph is None
    for agent, (got, want) in enumerate(zip(captured.buffer, eager.buffer)):
        assert got.obs.shape[-1] == (8, 10, 10)[agent] and got.share_obs.shape[-1] == 28
        assert float(got.masks.min()) == 0.0                        # the worlds restarted at step 25
        for name in ("share_obs", "obs", "actions", "rewards", "masks", "value_preds", "action_log_probs"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (agent, name)
    assert not torch.equal(captured.buffer[0].rewards, captured.buffer[1].rewards)      # the agents' own rewards
    assert torch.equal(captured.buffer[1].rewards, captured.buffer[2].rewards)          # ... the good agents' alike


def test_train_script_end_to_end_on_device_worlds(tmp_path, monkeypatch):
    from onpolicy import _native
    _native.count_calls(True)
    try:
        runner = _run(tmp_path, monkeypatch, "1", 4, 2)
        calls = _native.calls()
    finally:
        _native.count_calls(False)
    assert runner.envs.device.type == "cuda" and runner.rollout_graph.replays == 50
    assert calls.get("mappo_simple_adversary_step", 0) > 0, calls
    for b in runner.buffer:
        assert torch.isfinite(b.rewards).all() and torch.isfinite(b.obs).all() and torch.isfinite(b.value_preds).all()
    assert float(runner.buffer[0].rewards.max()) <= 0.0             # the adversary: -d^2
    assert int(runner.envs.t.max()) == 0
