"""-m gpu: K11 wide (``mappo_simple_spread_step_wide``): simple_spread worlds of up to 64 agents and 64 landmarks as one
launch, the lanes of a wave along a world's entities -- against the tensor-op step, and under the captured rollout."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("agents,landmarks,worlds,forced", [
    (17, 17, 65, False),        # the first shape past K11; 32 lanes per world, the last wave holds one world
    (32, 32, 3, False),         # 32 lanes per world, all busy
    (33, 5, 1, False),          # 64 lanes per world by the agents alone, a single world
    (5, 40, 65, False),         # 64 lanes per world by the landmarks, more landmarks than agents
    (64, 64, 65, False),        # every lane busy, the last workgroup partly filled
    (3, 3, 193, True),          # MAPPO_SPREAD_WIDE=1: a row's pairs all inside one trip
    (16, 16, 5, True)])         # the shape K11 takes too
def test_wide_step_equals_tensor_ops(monkeypatch, agents, landmarks, worlds, forced):
    """Every step on its own against ``_step_ops`` in float64 from the same seed and the same state (the reference's
    state is copied into the kernel's tensors after each step: at 64 agents pairs start millimetres apart, and a
    trajectory would amplify the last bits in which the two orders of summation differ).  State and per_agent to 1e-12:
    at most 63 contacts of at most 1e2 * 0.3 in force, 8 ulp each, times dt, is below 2e-13.  The kernel must have run:
    the state tensors stay where they are."""
    from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread
    if forced:
        monkeypatch.setenv("MAPPO_SPREAD_WIDE", "1")
    T = 7
    a = TorchSimpleSpread(worlds, agents, landmarks, episode_length=T, seed=5, device=DEV)
    b = TorchSimpleSpread(worlds, agents, landmarks, episode_length=T, seed=5, device=DEV)
    assert a.graph_safe and a._wide
    assert torch.equal(a.reset(), b.reset())
    where = a.pos.data_ptr(), a.vel.data_ptr()
    # the contact count compares a distance with 0.3: no pair of the reference may sit on the threshold
    margins, reward = [], b._reward
    def watched():
        dist = ((b.pos[:, :, None, :] - b.pos[:, None, :, :]) ** 2).sum(-1).sqrt()
        margins.append((dist - 0.3).abs().min())
        return reward()
    b._reward = watched
    g = torch.Generator(device=DEV).manual_seed(1)
    for step in range(3 * T + 2):
        act = torch.randint(0, 5, (worlds, agents, 1), generator=g, device=DEV)
        if step % 2:        # the host protocol's one-hot actions are accepted too
            act = torch.nn.functional.one_hot(act[..., 0], 5).float()
        ra, rb = a.step(act), b._step_ops(act)
        assert float(margins[-1]) > 1e-9, "a pair distance on the contact threshold: change the seed"
        torch.testing.assert_close(ra[0], rb[0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(ra[1], rb[1], rtol=1e-6, atol=1e-6)
        assert torch.equal(ra[2], rb[2]) and torch.equal(a.t, b.t)
        torch.testing.assert_close(ra[3]._per_agent, rb[3]._per_agent, rtol=0, atol=1e-12)
        for name in ("pos", "vel", "landmarks", "t"):
            if name != "t":
                torch.testing.assert_close(getattr(a, name), getattr(b, name), rtol=0, atol=1e-12)
            getattr(a, name).copy_(getattr(b, name))
    assert where == (a.pos.data_ptr(), a.vel.data_ptr())


def _run(tmp_path, monkeypatch, graph):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / ("results" + graph)))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    threads = torch.get_num_threads()
    try:
        return train_mpe.main(["--env_name", "MPE", "--scenario_name", "simple_spread", "--num_agents", "17",
                               "--num_landmarks", "3", "--algorithm_name", "mappo", "--n_rollout_threads", "8",
                               "--episode_length", "8", "--num_env_steps", str(2 * 8 * 8), "--ppo_epoch", "2",
                               "--num_mini_batch", "1", "--data_chunk_length", "4", "--hidden_size", "64", "--use_ReLU",
                               "--use_wandb", "--log_interval", "1", "--n_training_threads", "1", "--use_device_env"])
    finally:
        torch.set_num_threads(threads)      # (--n_training_threads 1 sets the process's thread count)


def test_rollout_with_17_agents_is_captured(tmp_path, monkeypatch):
    """One agent past K11 the rollout step still captures, and the captured run fills the buffer as the eager one."""
    captured, eager = _run(tmp_path, monkeypatch, "1"), _run(tmp_path, monkeypatch, "0")
    rg = captured.rollout_graph
    assert rg is not None and rg.graph is not None, "the rollout step was not captured"
    assert rg.replays == 2 * 8
    for name in ("actions", "rewards", "masks", "obs"):
        assert torch.equal(getattr(captured.buffer, name), getattr(eager.buffer, name)), name
    for name in ("value_preds", "action_log_probs"):
        torch.testing.assert_close(getattr(captured.buffer, name), getattr(eager.buffer, name), rtol=1e-5, atol=1e-6)
