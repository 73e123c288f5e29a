"""-m gpu: simple_reference with its worlds on the device.  The step kernel (``mappo_simple_reference_step``) against the
reference's trajectories and against the tensor-op path it replaces; the MultiDiscrete form of K14
(``mappo_multi_categorical_sample``) against the framework's sampling rule and route; the rollout replayed from one
captured graph against the eager loop; the train script end to end."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import Box, make_args
from test_mpe_reference_cpu import replay_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_step_kernel_matches_reference_trajectories(gold, case):
    replay_case(gold.npz("mpe_reference_cases"), case, device=DEV)


def test_step_kernel_equals_tensor_ops_with_auto_reset():
    """Same seed, same generator draws: three episodes (two restarts) of 4097 worlds (not a multiple of the 64-thread
    block) -- float64 state to 1e-12, float32 outputs to 1e-6, goals / symbols / t / dones identical."""
    from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
    n, T = 4097, 5
    a = TorchSimpleReference(n, episode_length=T, seed=7, device=DEV)
    b = TorchSimpleReference(n, episode_length=T, seed=7, device=DEV)
    assert a.graph_safe
    assert torch.equal(a.reset(), b.reset())
    a.t.random_(0, T, generator=torch.Generator(device=DEV).manual_seed(3))      # staggered episodes
    b.t.copy_(a.t)
    g = torch.Generator(device=DEV).manual_seed(1)
    ptrs = {k: getattr(a, k).data_ptr() for k in a.state_names}
    restarts = 0
    for step in range(3 * T):
        act = torch.stack([torch.randint(0, 5, (n, 2), generator=g, device=DEV),
                           torch.randint(0, 10, (n, 2), generator=g, device=DEV)], -1)
        if step % 3 == 2:       # the host protocol's one-hot actions are accepted too
            act = torch.cat([torch.nn.functional.one_hot(act[..., 0], 5), torch.nn.functional.one_hot(act[..., 1], 10)],
                            -1).float()
        ra = a.step(act)                        # kernel
        rb = b._step_ops(act)
        torch.testing.assert_close(ra[0], rb[0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(ra[1], rb[1], rtol=1e-6, atol=1e-6)
        assert torch.equal(ra[2], rb[2])
        torch.testing.assert_close(ra[3]._per_agent, rb[3]._per_agent, rtol=1e-12, atol=1e-12)
        for name in ("pos", "vel", "landmarks"):
            torch.testing.assert_close(getattr(a, name), getattr(b, name), rtol=1e-12, atol=1e-12, msg=name)
        for name in ("t", "goal", "comm"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        restarts += int(ra[2][:, 0].sum())
    assert restarts >= 2 * n
    assert {k: getattr(a, k).data_ptr() for k in a.state_names} == ptrs       # advanced in place: a graph can replay it


def _sample_on_noise(logits, noise, sizes):
    from onpolicy import _native
    rows, k = logits.shape[0], len(sizes)
    actions = torch.empty((rows, k), dtype=torch.int64, device=DEV)
    logp = torch.empty((rows, k), dtype=torch.float32, device=DEV)
    p = _native.ptr
    rc = _native.lib().mappo_multi_categorical_sample(
        p(logits), (ctypes.c_void_p * k)(*[p(q) for q in noise]), (ctypes.c_int * k)(*sizes), k, p(actions), p(logp),
        rows, _native.stream_of(DEV))
    _native.check(rc, "mappo_multi_categorical_sample")
    return actions, logp


@pytest.mark.parametrize("sizes,rows", [([5, 10], 4099), ([3, 4], 333), ([8] * 8, 1025), ([40, 23, 1], 3),
                                        ([5, 10], 1), ([57, 7], 4099), ([1] * 8, 257), ([57, 7], 262145),
                                        ([8] * 8, 256)])
def test_multi_categorical_sample_kernel_vs_the_framework_rule(sizes, rows):
    """Per sub-head: log p = x - logsumexp(x), action = argmax p / q on the SAME Exponential(1) noise (torch.multinomial's
    rule for one draw), log-prob of the action; sub-heads side by side, log-probs not summed."""
    g = torch.Generator(device=DEV).manual_seed(sum(sizes) + rows)
    logits = torch.randn(rows, sum(sizes), device=DEV, generator=g) * 2.0
    noise = [torch.empty(rows, n, device=DEV).exponential_(1.0, generator=g) for n in sizes]
    actions, logp = _sample_on_noise(logits, noise, sizes)
    assert actions.shape == (rows, len(sizes)) and logp.shape == (rows, len(sizes))
    same, ref_lp = [], []
    for k, x in enumerate(logits.split(sizes, -1)):
        ref_l = x - x.logsumexp(-1, keepdim=True)
        ref_a = (ref_l.exp() / noise[k]).argmax(-1, keepdim=True)
        same.append(actions[:, k:k + 1] == ref_a)
        ref_lp.append(ref_l.gather(-1, ref_a))
    same, ref_lp = torch.cat(same, -1), torch.cat(ref_lp, -1)
    assert same.float().mean() >= 0.999
    assert bool(((actions >= 0) & (actions < torch.tensor(sizes, device=DEV))).all())
    torch.testing.assert_close(logp[same], ref_lp[same], rtol=1e-5, atol=1e-6)
    # where an action differs it is a near-tie: in float64 the two candidates' p / q agree to 1e-5 (no wrong action can hide
    # in the 0.1 %), and every log-prob is that of the action the kernel chose
    for k, x in enumerate(logits.split(sizes, -1)):
        l64 = x.double() - x.double().logsumexp(-1, keepdim=True)
        score = l64.exp() / noise[k].double()
        mine, best = score.gather(-1, actions[:, k:k + 1]), score.max(-1, keepdim=True).values
        assert bool(((best - mine).abs() <= 1e-5 * best).all()), (k, sizes)
        torch.testing.assert_close(logp[:, k:k + 1].double(), l64.gather(-1, actions[:, k:k + 1]), rtol=1e-5, atol=1e-6)
    if sizes == [1] * 8:
        assert float(actions.abs().max()) == 0 and float(logp.abs().max()) == 0.0       # one action: chosen, log 1


def test_multi_categorical_sample_with_wide_logits():
    """Logits x 30 (probabilities from 1 down to underflow) through two sub-heads that fill the 64 columns."""
    sizes, rows = [57, 7], 4099
    g = torch.Generator(device=DEV).manual_seed(4)
    logits = torch.randn(rows, 64, device=DEV, generator=g) * 30.0
    noise = [torch.empty(rows, n, device=DEV).exponential_(1.0, generator=g) for n in sizes]
    actions, logp = _sample_on_noise(logits, noise, sizes)
    same = 0
    for k, x in enumerate(logits.split(sizes, -1)):
        l64 = x.double() - x.double().logsumexp(-1, keepdim=True)
        score = l64.exp() / noise[k].double()
        a = actions[:, k:k + 1]
        mine, best = score.gather(-1, a), score.max(-1, keepdim=True).values
        assert bool(((best - mine).abs() <= 1e-5 * best).all())
        same += int((a == score.argmax(-1, keepdim=True)).sum())
        # (one float32 ulp of the largest logit on top of the benign tolerance: rounding logsumexp to float32)
        torch.testing.assert_close(logp[:, k:k + 1].double(), l64.gather(-1, a), rtol=1e-5,
                                   atol=1e-6 + 2.0 ** -23 * float(x.abs().max()))
    assert same >= 0.999 * rows * len(sizes)


def test_multi_categorical_sample_frequencies():
    from onpolicy.algorithms.utils import fused_loss
    sizes = [5, 10]
    x = torch.randn(1, 15, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    with torch.no_grad():
        a, _ = fused_loss.sample_multi_categorical(x.expand(20000, 15).contiguous(), sizes)
    for k, part in enumerate(x[0].split(sizes)):
        freq = torch.bincount(a[:, k], minlength=sizes[k]).float() / 20000
        torch.testing.assert_close(freq, torch.softmax(part, -1), rtol=0, atol=0.015)


def test_multi_discrete_policy_samples_like_the_framework(monkeypatch):
    """The same policy and seed with and without MAPPO_FUSED_SAMPLE=0: the fused path draws the noise per sub-head in order
    as torch.multinomial(p, 1) does, so actions (and the random stream after them) agree."""
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from onpolicy.algorithms.utils import distributions, fused_loss
    from onpolicy.utils.multi_discrete import MultiDiscrete
    distributions.set_sampling_rng("device")
    args = make_args(hidden_size=64)
    space = MultiDiscrete([[0, 4], [0, 9]])
    torch.manual_seed(1)
    policy = R_MAPPOPolicy(args, Box((21,)), Box((42,)), space, device=DEV)
    assert sorted(k for k in policy.actor.state_dict() if k.startswith("act.")) == [
        "act.action_outs.0.linear.bias", "act.action_outs.0.linear.weight",
        "act.action_outs.1.linear.bias", "act.action_outs.1.linear.weight"]
    rows = 4097
    g = torch.Generator(device=DEV).manual_seed(2)
    obs = torch.randn(rows, 21, device=DEV, generator=g)
    rnn = torch.zeros(rows, 1, 64, device=DEV)
    masks = torch.ones(rows, 1, device=DEV)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MAPPO_FUSED_SAMPLE", mode)
        with torch.no_grad():
            assert fused_loss.multi_sample_supported(obs, [5, 10]) == (mode == "1")
            torch.manual_seed(77)
            a, lp, _ = policy.actor(obs, rnn, masks)
            after = torch.rand(4, device=DEV)
        out[mode] = a, lp, after
    (a1, l1, r1), (a0, l0, r0) = out["1"], out["0"]
    assert a1.shape == a0.shape == (rows, 2) and a1.dtype == a0.dtype == torch.int64 and l1.shape == (rows, 2)
    same = a1 == a0
    assert same.float().mean() >= 0.999
    torch.testing.assert_close(l1[same], l0[same], rtol=1e-5, atol=1e-6)
    assert torch.equal(r1, r0)                                   # both paths consumed the same random stream


def _runner(tmp_path, monkeypatch, algo, N=64, T=12, episodes=2, graph="1"):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    return train_mpe.main(["--env_name", "MPE", "--scenario_name", "simple_reference", "--num_agents", "2",
                           "--num_landmarks", "3", "--algorithm_name", algo, "--n_rollout_threads", str(N),
                           "--episode_length", str(T), "--num_env_steps", str(episodes * N * T), "--ppo_epoch", "2",
                           "--num_mini_batch", "1", "--data_chunk_length", "4", "--hidden_size", "64", "--gain", "0.01",
                           "--lr", "7e-4", "--critic_lr", "7e-4", "--use_wandb", "--log_interval", "1",
                           "--n_training_threads", "1", "--use_device_env"])


FIELDS = ("share_obs", "obs", "actions", "action_log_probs", "value_preds", "rewards", "masks", "rnn_states",
          "rnn_states_critic")


def _fields(runner):
    return {k: getattr(runner.buffer, k).clone() for k in FIELDS if getattr(runner.buffer, k).stride()[0] != 0}


@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_graphed_rollout_equals_eager_rollout(tmp_path, monkeypatch, algo):
    """A rollout replayed from the captured graph -- after two train() calls, so with updated weights -- fills the buffer
    as the eager loop does from the same worlds (goals and symbols included) and generator states."""
    runner = _runner(tmp_path, monkeypatch, algo, T=30)          # episodes of 30 steps: worlds restart inside the rollout
    e = runner.envs
    rg = runner.rollout_graph
    assert type(e).__name__ == "TorchSimpleReference"
    assert rg is not None and rg.graph is not None, "the rollout step was not captured"
    assert rg._state_names() == e.state_names and rg.replays == 2 * runner.episode_length
    T = runner.episode_length
    snap = ({k: getattr(e, k).clone() for k in e.state_names}, e.rng.get_state(), torch.cuda.get_rng_state(DEV),
            runner.buffer.step)
    row0 = {k: getattr(runner.buffer, k)[0].clone() for k in ("obs", "share_obs", "masks")}

    for step in range(T):
        values, actions, logp, rnn_a, rnn_c, actions_env = runner.collect(step)
        obs, rewards, dones, infos = e.step(actions_env)
        runner.insert((obs, rewards, dones, infos, values, actions, logp, rnn_a, rnn_c))
    torch.cuda.synchronize()
    eager = _fields(runner)
    eager_state = {k: getattr(e, k).clone() for k in e.state_names}
    eager_infos = [[d["individual_reward"] for d in row] for row in infos]

    state, env_rng, dev_rng, bstep = snap
    for k, v in state.items():
        getattr(e, k).copy_(v)
    e.rng.set_state(env_rng)
    torch.cuda.set_rng_state(dev_rng, DEV)
    runner.buffer.step = bstep
    for k, v in row0.items():
        getattr(runner.buffer, k)[0].copy_(v)
    runner.trainer.prep_rollout()
    rg.begin_episode()
    for step in range(T):
        g_infos = rg.step()
    torch.cuda.synchronize()
    graphed = _fields(runner)
    assert float(graphed["masks"].min()) == 0.0
    assert graphed["actions"].shape[-1] == 2 and graphed["action_log_probs"].shape[-1] == 2
    np.testing.assert_array_equal(graphed["actions"].cpu().numpy(), eager["actions"].cpu().numpy())
    for name in eager:
        torch.testing.assert_close(graphed[name], eager[name], rtol=1e-5, atol=1e-6, msg=name)
    for k in e.state_names:
        torch.testing.assert_close(getattr(e, k), eager_state[k], rtol=0, atol=0, msg=k)
    np.testing.assert_allclose([[d["individual_reward"] for d in row] for row in g_infos], eager_infos, rtol=1e-6)


def test_train_script_end_to_end_on_device_worlds(tmp_path, monkeypatch):
    """The reference's train_mpe_reference.sh flags (rmappo, gain 0.01, lr 7e-4) at small sizes with --use_device_env:
    two episodes through the captured rollout graph, finite training info."""
    from onpolicy import _native
    _native.count_calls(True)
    try:
        runner = _runner(tmp_path, monkeypatch, "rmappo", N=128, T=25, episodes=2)
        calls = _native.calls()
    finally:
        _native.count_calls(False)
    assert type(runner.envs).__name__ == "TorchSimpleReference" and runner.envs.device.type == "cuda"
    assert runner.rollout_graph is not None and runner.rollout_graph.replays == 2 * 25
    # the captured step was recorded from the two kernels (warm-up + capture call them from Python)
    assert calls.get("mappo_simple_reference_step", 0) > 0 and calls.get("mappo_multi_categorical_sample", 0) > 0, calls
    recs = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    for tag in ("value_loss", "policy_loss", "dist_entropy", "average_episode_rewards", "agent0/individual_rewards"):
        vals = [r[tag] for r in recs if r["tag"] == tag]
        assert len(vals) == 2 and all(np.isfinite(vals)), (tag, vals)
    assert torch.isfinite(runner.buffer.rewards).all() and torch.isfinite(runner.buffer.obs).all()
    assert float(runner.buffer.rewards.max()) <= 0.0                # negative squared distances
    acts = runner.buffer.actions.reshape(-1, 2)
    assert float(acts[:, 0].max()) <= 4 and float(acts[:, 1].max()) <= 9 and float(acts.min()) >= 0
