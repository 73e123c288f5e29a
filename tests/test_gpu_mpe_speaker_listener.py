"""-m gpu: simple_speaker_listener with its worlds on the device.  The step kernel
(``mappo_simple_speaker_listener_step``) against the reference's trajectories and against the tensor-op path it
replaces; the separated runner's rollout replayed from one captured graph against its eager loop; the train script end
to end with the flags of the reference's train_mpe_comm.sh."""
import json
import os

import numpy as np
import pytest
import torch

from test_mpe_speaker_listener_cpu import CASES, comm_argv, replay_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_step_kernel_matches_reference_trajectories(gold, case):
    replay_case(gold.npz(CASES), case, device=DEV, n=1)


def test_step_kernel_equals_tensor_ops_with_auto_reset():
    """Same seed, same generator draws: three episodes of 193 worlds (three 64-thread blocks and one thread), staggered,
    so every world restarts at least twice -- float64 state to 1e-12, float32 outputs to 1e-6, t / goal / comm / dones
    identical, the state advanced in place."""
    from onpolicy.envs.mpe.simple_speaker_listener import TorchSimpleSpeakerListener
    n, T = 193, 5
    a = TorchSimpleSpeakerListener(n, episode_length=T, seed=7, device=DEV)
    b = TorchSimpleSpeakerListener(n, episode_length=T, seed=7, device=DEV)
    assert a.graph_safe
    assert torch.equal(a.reset(), b.reset())
    a.t.copy_(torch.arange(n, device=DEV) % T)                      # staggered episodes
    b.t.copy_(a.t)
    g = torch.Generator(device=DEV).manual_seed(1)
    ptrs = {k: getattr(a, k).data_ptr() for k in a.state_names}
    restarts = torch.zeros(n, dtype=torch.int64, device=DEV)
    for step in range(3 * T):
        act = torch.stack([torch.randint(0, 3, (n,), generator=g, device=DEV),
                           torch.randint(0, 5, (n,), generator=g, device=DEV)], -1)
        if step % 2 == 1:       # the host protocol's one-hot actions are accepted too
            act = torch.cat([torch.nn.functional.one_hot(act[:, 0], 3), torch.nn.functional.one_hot(act[:, 1], 5)],
                            -1).float()
        ra = a.step(act)                        # kernel
        rb = b._step_ops(act)
        assert ra[0].shape == (n, 14) and ra[0].dtype == torch.float32
        torch.testing.assert_close(ra[0], rb[0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(ra[1], rb[1], rtol=1e-6, atol=1e-6)
        assert torch.equal(ra[2], rb[2])
        torch.testing.assert_close(ra[3]._per_agent, rb[3]._per_agent, rtol=1e-12, atol=1e-12)
        for name in ("pos", "vel", "landmarks"):
            torch.testing.assert_close(getattr(a, name), getattr(b, name), rtol=1e-12, atol=1e-12, msg=name)
        for name in ("t", "goal", "comm"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        restarts += ra[2][:, 0]
    assert int(restarts.min()) >= 2
    assert {k: getattr(a, k).data_ptr() for k in a.state_names} == ptrs       # advanced in place: a graph can replay it


def _runner(tmp_path, monkeypatch, algo, N, T, episodes, graph="1"):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    argv = comm_argv(algo, n=N, t=T, steps=episodes * N * T, hidden=64)
    argv[argv.index("--data_chunk_length") + 1] = "4" if T % 4 == 0 else "5"
    threads = torch.get_num_threads()
    try:
        return train_mpe.main(argv + ["--use_device_env"])
    finally:
        torch.set_num_threads(threads)      # (--n_training_threads 1 sets the process's thread count)


FIELDS = ("share_obs", "obs", "actions", "action_log_probs", "value_preds", "rewards", "masks", "rnn_states",
          "rnn_states_critic")


def _fields(runner):
    return [{k: getattr(b, k).clone() for k in FIELDS if getattr(b, k).stride()[0] != 0} for b in runner.buffer]


@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_graphed_rollout_equals_eager_rollout(tmp_path, monkeypatch, algo):
    """A rollout replayed from the captured graph -- after two train() calls, so with updated weights -- fills both
    agents' buffers as the eager loop does from the same worlds (goal and symbol included) and generator states."""
    runner = _runner(tmp_path, monkeypatch, algo, N=16, T=30, episodes=2)      # 30 steps: worlds restart in the rollout
    e = runner.envs
    rg = runner.rollout_graph
    assert type(e).__name__ == "TorchSimpleSpeakerListener" and len(runner.buffer) == 2
    assert rg is not None and rg.graph is not None, "the rollout step was not captured"
    assert rg._state_names() == e.state_names and rg.replays == 2 * runner.episode_length
    T = runner.episode_length
    steps = [b.step for b in runner.buffer]
    snap = ({k: getattr(e, k).clone() for k in e.state_names}, e.rng.get_state(), torch.cuda.get_rng_state(DEV))
    row0 = [{k: getattr(b, k)[0].clone() for k in ("obs", "share_obs", "masks")} for b in runner.buffer]

    for step in range(T):
        values, actions, logp, rnn_a, rnn_c, actions_env = runner.collect(step)
        assert torch.is_tensor(actions_env) and actions_env.shape == (16, 2) and actions_env.dtype == torch.int64
        obs, rewards, dones, infos = e.step(actions_env)
        runner.insert((obs, rewards, dones, infos, values, actions, logp, rnn_a, rnn_c))
    torch.cuda.synchronize()
    eager = _fields(runner)
    eager_state = {k: getattr(e, k).clone() for k in e.state_names}
    eager_infos = [[d["individual_reward"] for d in row] for row in infos]

    state, env_rng, dev_rng = snap
    for k, v in state.items():
        getattr(e, k).copy_(v)
    e.rng.set_state(env_rng)
    torch.cuda.set_rng_state(dev_rng, DEV)
    for b, s, rows in zip(runner.buffer, steps, row0):
        b._inner.step = s
        for k, v in rows.items():
            getattr(b, k)[0].copy_(v)
    for tr in runner.trainer:
        tr.prep_rollout()
    rg.begin_episode()
    for step in range(T):
        g_infos = rg.step()
    torch.cuda.synchronize()
    assert rg.replays == 3 * T
    graphed = _fields(runner)
    for agent, (got, want, top) in enumerate(zip(graphed, eager, (2, 4))):
        assert float(got["masks"].min()) == 0.0
        assert got["actions"].shape[-1] == 1 and float(got["actions"].max()) <= top
        np.testing.assert_array_equal(got["actions"].cpu().numpy(), want["actions"].cpu().numpy())
        assert ("rnn_states" in got) == (algo == "rmappo")
        for name in want:
            torch.testing.assert_close(got[name], want[name], rtol=1e-5, atol=1e-6, msg="agent %d %s" % (agent, name))
    assert graphed[0]["obs"].shape[-1] == 3 and graphed[1]["obs"].shape[-1] == 11
    assert graphed[0]["share_obs"].shape[-1] == graphed[1]["share_obs"].shape[-1] == 14
    for k in e.state_names:
        torch.testing.assert_close(getattr(e, k), eager_state[k], rtol=0, atol=0, msg=k)
    np.testing.assert_allclose([[d["individual_reward"] for d in row] for row in g_infos], eager_infos, rtol=1e-6)


def test_train_script_end_to_end_on_device_worlds(tmp_path, monkeypatch):
    """The reference's train_mpe_comm.sh flags (rmappo, 128 threads, 25 steps, gain 0.01, lr 7e-4, --share_policy) with
    --use_device_env: two episodes through the captured rollout graph, finite training info for both agents."""
    from onpolicy import _native
    _native.count_calls(True)
    try:
        runner = _runner(tmp_path, monkeypatch, "rmappo", N=128, T=25, episodes=2)
        calls = _native.calls()
    finally:
        _native.count_calls(False)
    assert type(runner.envs).__name__ == "TorchSimpleSpeakerListener" and runner.envs.device.type == "cuda"
    assert runner.rollout_graph is not None and runner.rollout_graph.replays == 50
    # the captured step was recorded from the two kernels (warm-up + capture call them from Python)
    assert calls.get("mappo_simple_speaker_listener_step", 0) > 0 and calls.get("mappo_categorical_sample", 0) > 0, calls
    recs = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    for agent in (0, 1):
        for tag in ("value_loss", "policy_loss", "dist_entropy", "average_episode_rewards", "individual_rewards"):
            vals = [r["agent%d/%s" % (agent, tag)] for r in recs if r["tag"] == "agent%d/%s" % (agent, tag)]
            assert len(vals) == 2 and all(np.isfinite(vals)), (agent, tag, vals)
    b0, b1 = runner.buffer
    assert b0.obs.shape[-1] == 3 and b1.obs.shape[-1] == 11 and b0.share_obs.shape[-1] == b1.share_obs.shape[-1] == 14
    for b, top in ((b0, 2), (b1, 4)):
        assert torch.isfinite(b.rewards).all() and torch.isfinite(b.obs).all()
        assert float(b.rewards.max()) <= 0.0                # negative squared distances
        assert float(b.actions.min()) >= 0 and float(b.actions.max()) <= top
    assert torch.equal(b0.rewards, b1.rewards)
