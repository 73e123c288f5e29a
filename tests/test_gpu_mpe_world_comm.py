"""-m gpu: simple_world_comm with its worlds on the device.  The step kernel (``mappo_simple_world_comm_step``) against the
reference's trajectories and against the tensor-op path it replaces (block boundaries, catches, obstacle contacts, food,
forests, coincident centres, restarts, the agent cap); the caps and the C entry point's refusal codes; the separated
runner's rollout -- a MultiDiscrete leader among Discrete agents -- replayed from one captured graph against its eager loop
at 2 against 1 and 4 against 2; ``--use_device_eval`` captured against eager, and leaving training untouched; the train
script end to end."""
import json
import os

import numpy as np
import pytest
import torch

from test_mpe_world_comm_cpu import (CASES, CATCH, FOOD, FOREST, N_CASES, SIZE, make, one_hot_actions, random_actions,
                                     replay_case, widths, world_comm_argv)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("case", range(N_CASES))
def test_step_kernel_matches_reference_trajectories(gold, case):
    replay_case(gold.npz(CASES), case, device=DEV, n=1)


def _thresholds(env):
    """-> (pair [n, G, Nadv], food [n, G, 2], forest [n, A, 2] distances, the forests' reach [A, 1]) of ``env``'s state."""
    adv, l = env.num_adversaries, env.num_obstacles
    pair = (env.pos[:, adv:, None] - env.pos[:, None, :adv]).norm(dim=-1)
    food = (env.pos[:, adv:, None] - env.landmarks[:, None, l:l + 2]).norm(dim=-1)
    forest = (env.pos[:, :, None] - env.landmarks[:, None, l + 2:]).norm(dim=-1)
    reach = torch.tensor([SIZE[0]] * adv + [SIZE[1]] * (env.a - adv), dtype=torch.float64, device=env.device)[:, None] + FOREST
    return pair, food, forest, reach


def _near(env):
    """How many distances of ``env``'s state lie within 1e-9 of the threshold that decides a catch, a meal or hiding."""
    pair, food, forest, reach = _thresholds(env)
    return int(((pair - CATCH).abs() < 1e-9).sum() + ((food - FOOD).abs() < 1e-9).sum()
               + ((forest - reach).abs() < 1e-9).sum())


@pytest.mark.parametrize("n", [1, 64, 65, 193])
@pytest.mark.parametrize("adv,good,landmarks", [(4, 2, 1), (2, 1, 2), (1, 1, 1), (1, 3, 4), (13, 3, 4)])
def test_step_kernel_equals_tensor_ops_with_auto_reset(adv, good, landmarks, n):
    """Same seed, same generator draws: 10 steps of worlds that last 4, so every world restarts twice -- float64 state and
    per_agent to 1e-12, float32 outputs to 1e-6, t / dones / comm identical, the state advanced in place.  Every third
    world starts with, all at once: the leader on the first good agent, driven into each other; obstacle 0 against
    another agent (``other``; with two agents, against the good one); food 0 where that good agent arrives; forest 0
    around the leader and that good agent, forest 1 around one more agent (``far``) where there are more than two,
    everybody else -- somebody, from four agents on -- in the open.  In one world the leader, the last good agent, the
    last obstacle and food 1 start at the same point (no force between them, on either path), 0.36 from forest 0's
    centre: the leader is inside, the good agent is not and does not see it.  No distance of a compared step may lie
    within 1e-9 of 0.12, 0.075, 0.375 or 0.345, where the two paths could disagree."""
    A, L, T = adv + good, landmarks, 4
    f64 = dict(dtype=torch.float64, device=DEV)
    a = make(n, adv, good, L, seed=7, device=DEV, world_length=T)
    b = make(n, adv, good, L, seed=7, device=DEV, world_length=T)
    assert a.graph_safe
    assert torch.equal(a.reset(), b.reset())
    for name in a.state_names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    prepared = torch.arange(n, device=DEV) % 3 == 0
    same = 1 if n > 1 else 0
    other = 1 if adv >= 2 else A - 1
    far = A - 1 if A - 1 != adv else 1
    for env in (a, b):
        env.pos[prepared, adv] = env.pos[prepared, 0] + torch.tensor([0.06, 0.01], **f64)
        for k in range(1, A):       # ... the other agents out of that pair's reach, 0.5 apart, and the landmarks as well
            if k != adv:
                env.pos[prepared, k] = env.pos[prepared, 0] + torch.tensor([2.0 + 0.5 * k, 0.0], **f64)
        for l in range(L + 4):
            env.landmarks[prepared, l] = env.pos[prepared, 0] + torch.tensor([-3.0 - l, 0.0], **f64)
        env.landmarks[prepared, 0] = env.pos[prepared, other] + torch.tensor([0.2 if A == 2 else -0.2, 0.05], **f64)
        env.landmarks[prepared, L] = env.pos[prepared, adv] + torch.tensor([-0.1, 0.02], **f64)          # food 0
        env.landmarks[prepared, L + 2] = env.pos[prepared, 0] + torch.tensor([0.03, -0.1], **f64)        # forest 0
        if A > 2:
            env.landmarks[prepared, L + 3] = env.pos[prepared, far] + torch.tensor([0.0, 0.1], **f64)    # forest 1
        for k in range(1, A - 1):   # the coincident world: everything else out of reach as well
            env.pos[same, k] = env.pos[same, 0] + torch.tensor([2.0 + 0.5 * k, 0.0], **f64)
        for l in range(L - 1):
            env.landmarks[same, l] = env.pos[same, 0] + torch.tensor([-3.0 - l, 0.0], **f64)
        env.pos[same, A - 1] = env.pos[same, 0]
        env.landmarks[same, L - 1] = env.pos[same, 0]
        env.landmarks[same, L + 1] = env.pos[same, 0]                                                    # food 1
        env.landmarks[same, L + 2] = env.pos[same, 0] + torch.tensor([0.36, 0.0], **f64)                 # forest 0
    if n > 1:
        inside = a.inside()[0]      # world 0 is prepared: one agent inside each forest, one outside
        assert bool(inside[0, 0]) and bool(inside[adv, 0])
        assert A == 2 or (bool(inside[far, 1]) and not bool(inside[far, 0]))
        assert A < 4 or bool((~inside.any(1)).any())
        assert a.inside()[same, [0, A - 1], 0].tolist() == [True, False]
    c = make(n, adv, good, L, seed=7, device=DEV, world_length=T, auto_reset=False)     # the positions the rewards see
    g = np.random.default_rng(1)
    ptrs = {k: getattr(a, k).data_ptr() for k in a.state_names}
    restarts = torch.zeros(n, dtype=torch.int64, device=DEV)
    near_threshold = _near(b)
    caught = fed = hidden = 0
    for step in range(10):
        act = torch.from_numpy(random_actions(g, n, A)).to(DEV)
        if step == 0:
            act[prepared, 0], act[prepared, adv + 1] = 1, 2     # into each other
            if A > 2:
                act[prepared, other + 1] = 0                    # moved by the obstacle alone
            act[same, 0], act[same, A] = 0, 0                   # coincident and at rest: they stay where they are
        before = a.pos[same].clone()
        sent = one_hot_actions(act).float() if step % 2 == 1 else act      # the host protocol's one-hots are accepted too
        for name in c.state_names:
            setattr(c, name, getattr(b, name).clone())
        ra = a.step(sent)                       # kernel
        rb = b._step_ops(sent)
        c._step_ops(sent)                       # (b without the restarts: takes no draws)
        assert ra[0].shape == (n, sum(widths(adv, good, L))) and ra[0].dtype == torch.float32
        torch.testing.assert_close(ra[0], rb[0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(ra[1], rb[1], rtol=1e-6, atol=1e-6)
        assert torch.equal(ra[2], rb[2])
        torch.testing.assert_close(ra[3]._per_agent, rb[3]._per_agent, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ra[1][..., 0], ra[3]._per_agent.float(), rtol=0, atol=0)     # each agent's own
        for name in ("pos", "vel", "landmarks"):
            torch.testing.assert_close(getattr(a, name), getattr(b, name), rtol=1e-12, atol=1e-12, msg=name)
        assert torch.equal(a.t, b.t) and torch.equal(a.comm, b.comm)
        assert torch.equal(a.comm, torch.where(ra[2][:, 0], -1, act[:, 1]))
        assert bool(torch.isfinite(a.pos).all()) and bool(torch.isfinite(ra[0]).all())
        near_threshold += _near(c) + _near(b)           # what the rewards saw, what the observations saw
        pair, food, _, _ = _thresholds(c)
        caught += int((pair < CATCH).sum())
        fed += int((food < FOOD).sum())
        hidden += int((~b.visible()).sum())
        if step == 0 and n > 1:
            # the contact force acted: without it the leader left with +0.9; the obstacle alone moved `other`
            assert bool((a.vel[prepared, 0, 0] < 0.5).all())
            if A > 2:
                assert bool((a.vel[prepared, other, 0] > 0.1).all())
            assert torch.equal(a.pos[same, 0], before[0]) and torch.equal(a.pos[same, A - 1], before[0])
            # caught by the leader at least, and on food 1: -5 + 2 and what the other food and adversaries add
            assert float(ra[3]._per_agent[same, 0]) >= 5.0 and float(ra[3]._per_agent[same, A - 1]) < 0.0
        restarts += ra[2][:, 0]
    assert near_threshold == 0, "a distance within 1e-9 of 0.12, 0.075, 0.375 or 0.345: choose another seed"
    assert caught > 0 and fed > 0 and hidden > 0, (caught, fed, hidden)
    assert int(restarts.min()) == int(restarts.max()) == 2
    assert {k: getattr(a, k).data_ptr() for k in a.state_names} == ptrs       # advanced in place: a graph can replay it


def test_past_the_kernels_caps_worlds_step_as_tensor_ops():
    for adv, good, l in ((13, 4, 2), (4, 2, 5)):            # one agent, one obstacle past the cap
        env = make(3, adv, good, l, seed=1, device=DEV)
        assert not env.graph_safe
        env.reset()
        obs, rew, done, _ = env.step(torch.zeros(3, adv + good + 1, dtype=torch.int64, device=DEV))
        assert obs.shape == (3, sum(widths(adv, good, l))) and rew.shape == (3, adv + good, 1)
        assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
    assert make(3, 13, 3, 4, device=DEV).graph_safe


def test_entry_point_refusal_codes_on_device_buffers():
    """The C entry point called directly with device buffers that would serve 4 worlds of 6 agents: -1 for a missing
    pointer, -2 for a bad shape, MAPPO_E_TOO_MANY (-4) past either cap; nothing is launched, nothing is written."""
    from onpolicy import _native
    fn = _native.lib().mappo_simple_world_comm_step
    env = make(4, 4, 2, 1, seed=1, device=DEV)
    env.reset()
    kept = {k: getattr(env, k).clone() for k in env.state_names}
    act = torch.zeros(4, 7, dtype=torch.int64, device=DEV)
    fresh = env._fresh()
    out = [torch.zeros(4, sum(env.obs_dims), device=DEV), torch.zeros(4, 6, 1, device=DEV),
           torch.zeros(4, 6, dtype=torch.bool, device=DEV), torch.zeros(4, 6, dtype=torch.float64, device=DEV)]
    p = _native.ptr
    ptrs = [p(env.pos), p(env.vel), p(env.landmarks), p(env.t), p(env.comm), p(act), p(fresh[0]), p(fresh[1])] + [p(x) for x in out]
    stream = _native.stream_of(DEV)
    assert fn(*[None if j == 4 else q for j, q in enumerate(ptrs)], 4, 6, 4, 1, 25, 1, stream) == -1      # comm
    assert fn(*[None if j == 6 else q for j, q in enumerate(ptrs)], 4, 6, 4, 1, 25, 1, stream) == -1      # fresh_pos
    assert fn(*ptrs, 4, 6, 6, 1, 25, 1, stream) == -2 and fn(*ptrs, 4, 6, 4, 0, 25, 1, stream) == -2
    assert fn(*ptrs, 4, 17, 4, 1, 25, 1, stream) == -4 and fn(*ptrs, 4, 6, 4, 5, 25, 1, stream) == -4
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert torch.equal(getattr(env, k), v), k
    assert all(float(x.float().abs().max()) == 0.0 for x in out)


def _runner(tmp_path, monkeypatch, algo, adv, good, N, T, episodes, graph="1", extra=(), name="results"):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / name))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    argv = world_comm_argv(algo, adv, good, n=N, steps=episodes * N * T, hidden=64)
    argv[argv.index("--episode_length") + 1] = str(T)
    threads = torch.get_num_threads()
    try:
        return train_mpe.main(argv + ["--use_device_env"] + list(extra))
    finally:
        torch.set_num_threads(threads)      # (--n_training_threads 1 sets the process's thread count)


FIELDS = ("share_obs", "obs", "actions", "action_log_probs", "value_preds", "rewards", "masks", "rnn_states",
          "rnn_states_critic")


def _fields(runner):
    return [{k: getattr(b, k).clone() for k in FIELDS if getattr(b, k).stride()[0] != 0} for b in runner.buffer]


@pytest.mark.parametrize("adv,good", [(2, 1), (4, 2)])
@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_graphed_rollout_equals_eager_rollout(tmp_path, monkeypatch, algo, adv, good):
    """A rollout replayed from the captured graph -- after two train() calls, so with updated weights -- fills every
    agent's buffer bit for bit as the eager loop does from the same worlds and generator states: the leader's two
    sub-actions and the other agents' single ones go side by side into one env step, and that step captures."""
    agents = adv + good
    runner = _runner(tmp_path, monkeypatch, algo, adv, good, N=16, T=30, episodes=2)    # 30 steps: worlds restart at 25
    e = runner.envs
    rg = runner.rollout_graph
    assert type(e).__name__ == "TorchSimpleWorldComm" and len(runner.buffer) == agents
    assert rg is not None and rg.graph is not None, "the rollout step was not captured"
    assert rg._state_names() == e.state_names and rg.replays == 2 * runner.episode_length and rg.replays > 0
    T = runner.episode_length
    steps = [b.step for b in runner.buffer]
    snap = ({k: getattr(e, k).clone() for k in e.state_names}, e.rng.get_state(), torch.cuda.get_rng_state(DEV))
    row0 = [{k: getattr(b, k)[0].clone() for k in ("obs", "share_obs", "masks")} for b in runner.buffer]

    for step in range(T):
        values, actions, logp, rnn_a, rnn_c, actions_env = runner.collect(step)
        assert torch.is_tensor(actions_env) and actions_env.shape == (16, agents + 1) and actions_env.dtype == torch.int64
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
    dims = widths(adv, good, 1)
    for agent, (got, want) in enumerate(zip(graphed, eager)):
        assert float(got["masks"].min()) == 0.0
        assert got["actions"].shape[-1] == (2 if agent == 0 else 1) and float(got["actions"][..., 0].max()) <= 4
        assert ("rnn_states" in got) == (algo == "rmappo")
        for name in want:
            assert torch.equal(got[name], want[name]), "agent %d %s" % (agent, name)
        assert got["obs"].shape[-1] == dims[agent] and got["share_obs"].shape[-1] == sum(dims)
    assert float(graphed[0]["actions"][..., 1].max()) <= 3 and float(graphed[0]["actions"][..., 1].max()) > 0
    said = torch.nn.functional.one_hot(graphed[0]["actions"][:, :, 1].long(), 4).float()
    for agent in range(adv):            # every adversary heard the leader's word; after a restart nothing
        assert torch.equal(graphed[agent]["obs"][1:, :, -4:], said * graphed[agent]["masks"][1:])
    for k in e.state_names:
        assert torch.equal(getattr(e, k), eager_state[k]), k
    np.testing.assert_array_equal([[d["individual_reward"] for d in row] for row in g_infos], eager_infos)


EVAL_N, EVAL_T = 5, 6
EVAL = ("--use_eval", "--use_device_eval", "--eval_interval", "1", "--n_eval_rollout_threads", str(EVAL_N))


def _eval_runner(tmp_path, monkeypatch, name, algo, adv, good, episodes=1, extra=EVAL, graph="1"):
    monkeypatch.setenv("MAPPO_EVAL_GRAPH", graph)
    return _runner(tmp_path, monkeypatch, algo, adv, good, N=EVAL_N, T=EVAL_T, episodes=episodes, extra=extra, name=name)


def _logged(runner, step):
    rows = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    return sorted((r["tag"], r[r["tag"]]) for r in rows if r["step"] == step and "eval_average_episode_rewards" in r["tag"])


@pytest.mark.parametrize("algo,adv,good", [("rmappo", 2, 1), ("mappo", 4, 2)])
def test_captured_eval_equals_eager_eval(tmp_path, monkeypatch, algo, adv, good):
    """The pattern of test_gpu_mpe_tag.test_captured_eval_equals_eager_eval: two evaluations in a row, replayed from the
    captured step and run by the eager tensor loop -- logged values, totals and eval-world state bit for bit."""
    agents = adv + good
    g = _eval_runner(tmp_path, monkeypatch, "graph", algo, adv, good, graph="1")
    e = _eval_runner(tmp_path, monkeypatch, "eager", algo, adv, good, graph="0")
    worlds = g.eval_envs
    assert type(worlds).__name__ == "TorchSimpleWorldComm" and worlds.device.type == "cuda" and worlds is not g.envs
    assert worlds.num_adversaries == adv
    assert g.eval_graph is not None and g.eval_graph.graph is not None, "the eval step was not captured"
    assert type(g.eval_graph).__name__ == "SeparatedEvalGraph" and e.eval_graph is None
    assert g.eval_graph.replays == EVAL_T
    for ps, pd in zip(g.policy, e.policy):
        pd.actor.load_state_dict(ps.actor.state_dict())
    for name in worlds.state_names:
        getattr(e.eval_envs, name).copy_(getattr(worlds, name))
    e.eval_envs.rng.set_state(worlds.rng.get_state())
    ptrs = {name: getattr(worlds, name).data_ptr() for name in worlds.state_names}
    for call in (0, 1):
        g.eval(5000 + call)
        e.eval(5000 + call)
        torch.cuda.synchronize()
        got, want = _logged(g, 5000 + call), _logged(e, 5000 + call)
        assert len(want) == agents and got == want, (got, want)
        assert g.eval_totals.shape == e.eval_totals.shape == (EVAL_N, agents, 1)
        assert torch.equal(g.eval_totals, e.eval_totals)
        for name in worlds.state_names:
            assert torch.equal(getattr(worlds, name), getattr(e.eval_envs, name)), (call, name)
        assert int(worlds.comm.min()) >= 0          # 6 steps of 25: the leader's last word stands
        assert torch.equal(worlds.rng.get_state(), e.eval_envs.rng.get_state())
    assert g.eval_graph.replays == EVAL_T + 2 * EVAL_T
    assert ptrs == {name: getattr(worlds, name).data_ptr() for name in worlds.state_names}


def test_evaluation_does_not_perturb_training(tmp_path, monkeypatch):
    """Two episodes with an evaluation after each, and without any: the same weights and training worlds, bit for bit."""
    a = _eval_runner(tmp_path, monkeypatch, "with", "rmappo", 2, 1, episodes=2)
    b = _eval_runner(tmp_path, monkeypatch, "without", "rmappo", 2, 1, episodes=2, extra=())
    assert a.eval_graph is not None and a.eval_graph.replays == 2 * EVAL_T and b.eval_envs is None
    for pa, pb in zip(a.policy, b.policy):
        for net in ("actor", "critic"):
            sa, sb = getattr(pa, net).state_dict(), getattr(pb, net).state_dict()
            assert sorted(sa) == sorted(sb)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), (net, k)
    for name in a.envs.state_names:
        assert torch.equal(getattr(a.envs, name), getattr(b.envs, name)), name
    assert torch.equal(a.envs.rng.get_state(), b.envs.rng.get_state())


def test_train_script_end_to_end_on_device_worlds(tmp_path, monkeypatch):
    """The reference's script-family flags (rmappo, 128 threads, 25 steps, gain 0.01, lr 7e-4, --share_policy) with
    --use_device_env at 4 against 2: two episodes through the captured rollout graph, finite training info for all six."""
    from onpolicy import _native
    _native.count_calls(True)
    try:
        runner = _runner(tmp_path, monkeypatch, "rmappo", 4, 2, N=128, T=25, episodes=2)
        calls = _native.calls()
    finally:
        _native.count_calls(False)
    assert type(runner.envs).__name__ == "TorchSimpleWorldComm" and runner.envs.device.type == "cuda"
    assert runner.rollout_graph is not None and runner.rollout_graph.replays == 50
    # the captured step was recorded from the kernels (warm-up + capture call them from Python)
    assert calls.get("mappo_simple_world_comm_step", 0) > 0 and calls.get("mappo_categorical_sample", 0) > 0, calls
    recs = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    for agent in range(6):
        for tag in ("value_loss", "policy_loss", "dist_entropy", "average_episode_rewards", "individual_rewards"):
            vals = [r["agent%d/%s" % (agent, tag)] for r in recs if r["tag"] == "agent%d/%s" % (agent, tag)]
            assert len(vals) == 2 and all(np.isfinite(vals)), (agent, tag, vals)
    assert [b.obs.shape[-1] for b in runner.buffer] == [34] * 4 + [28] * 2
    for agent, b in enumerate(runner.buffer):
        assert b.share_obs.shape[-1] == 192 and b.actions.shape[-1] == (2 if agent == 0 else 1)
        assert torch.isfinite(b.rewards).all() and torch.isfinite(b.obs).all()
        assert float(b.actions.min()) >= 0 and float(b.actions[..., 0].max()) <= 4
        assert float(b.masks[-1].max()) == 0.0              # every world ended with the rollout's 25th step
    assert float(runner.buffer[0].actions[..., 1].max()) == 3.0
    assert int(runner.envs.t.max()) == 0 and int(runner.envs.comm.max()) == -1
