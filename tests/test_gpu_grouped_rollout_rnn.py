"""-m gpu: the recurrent grouped kernel (K19 recurrent, ``mappo_grouped_rnn_forward``) against float64 and its sampling against
K14 bit for bit; the separated runner's recurrent grouped route (``MAPPO_GROUPED_ROLLOUT=1 MAPPO_GROUPED_ROLLOUT_RNN=1``)
captured against eager, its launch counts, and one step against the per-agent K9 + K12 path."""
import pytest
import torch

import loss_reference as lr      # (the 4 x judge and its record)
from onpolicy import _native
from test_gpu_grouped_rollout import DEV, PAD, _guarded       # (K19's canaried outputs)

pytestmark = pytest.mark.gpu
JUDGE = lr.Judge()
# floor of the 4 x judge relative to the output's scale: ~3 x the largest kernel error measured on the MI355X (values
# 1.00e-6, logits 1.15e-6, state 9.4e-7 over these cases: profiles/small_kernel_margins.json, k19rnn.*); it began at 1e-5
FLOOR = {"k19rnn.values": 3e-6, "k19rnn.logits": 3.5e-6, "k19rnn.state": 3e-6}

# (rows, row stride of the joint matrix, networks (column offset, width, layers, act, input LayerNorm, out, actor))
CASES = {
    "one row, width 3": (1, 3, [(0, 3, 2, 1, False, 1, False)]),
    "exactly one chunk, three layers": (32, 64, [(0, 64, 3, 1, False, 32, True)]),
    "an actor and a critic, odd widths": (33, 160, [(1, 8, 2, 2, True, 5, True), (7, 143, 3, 1, True, 1, False)]),
    "three row tiles": (65, 150, [(7, 143, 3, 2, False, 32, True), (0, 3, 2, 1, True, 5, True)]),
    "128 networks": (65, 41, [(i % 7, 3 + i % 31, 2 + i % 2, 1 + i % 2, i % 3 != 1, (1, 5, 32)[i % 3], i % 3 != 0)
                              for i in range(128)]),
}


@pytest.fixture(autouse=True, scope="module")
def _record_margins():
    yield
    JUDGE.dump()


def _reference(x, h_in, mask, p, layers, act, dtype):
    """-> (head output, h'): the network of include/mappo_hip.h's K19 recurrent paragraph, written with torch.nn.functional."""
    F = torch.nn.functional
    t = lambda v: v.to(dtype)
    f = torch.tanh if act == 1 else torch.relu
    x = t(x)
    if "in_g" in p:
        x = F.layer_norm(x, x.shape[1:], t(p["in_g"]), t(p["in_b"]), 1e-5)
    for l in range(layers):
        x = F.layer_norm(f(F.linear(x, t(p["w"][l]), t(p["bias"][l]))), (64,), t(p["ln_g"][l]), t(p["ln_b"][l]), 1e-5)
    hm = t(h_in) * t(mask)[:, None]
    i_r, i_z, i_n = F.linear(x, t(p["w_ih"]), t(p["b_ih"])).chunk(3, -1)
    h_r, h_z, h_n = F.linear(hm, t(p["w_hh"]), t(p["b_hh"])).chunk(3, -1)
    r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    h = (1 - z) * n + z * hm
    return F.linear(F.layer_norm(h, (64,), t(p["rnn_g"]), t(p["rnn_b"]), 1e-5), t(p["wh"]), t(p["bh"])), h


def _launch(name):
    """One launch of a case -> per network (spec, parameters, (input columns, h_in, mask), guarded outputs)."""
    rows, ld, specs = CASES[name]
    g = torch.Generator(device=DEV).manual_seed(len(name))
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g, device=DEV) * scale
    joint = rn(rows, ld) + 0.5
    # masks: mixed in the first tile, all zero in the second, all one in the third
    mask = (torch.arange(rows, device=DEV) % 3 != 0).float()
    mask[32:64], mask[64:] = 0.0, 1.0
    nets, keep = (_native.GroupedRnnNet * len(specs))(), []
    for e, (col, din, layers, act, in_ln, out, actor) in zip(nets, specs):
        d = e.net
        p = dict(w=[rn(64, din if l == 0 else 64, scale=(din if l == 0 else 64) ** -0.5) for l in range(layers)],
                 bias=[rn(64, scale=0.1) for _ in range(layers)], ln_g=[1 + rn(64, scale=0.1) for _ in range(layers)],
                 ln_b=[rn(64, scale=0.1) for _ in range(layers)], wh=rn(out, 64, scale=0.125), bh=rn(out, scale=0.1),
                 w_ih=rn(192, 64, scale=0.125), w_hh=rn(192, 64, scale=0.125), b_ih=rn(192, scale=0.1), b_hh=rn(192, scale=0.1),
                 rnn_g=1 + rn(64, scale=0.1), rnn_b=rn(64, scale=0.1), h_in=rn(rows, 64))
        if in_ln:
            p.update(in_g=1 + rn(din, scale=0.1), in_b=rn(din, scale=0.1))
            d.in_g, d.in_b = p["in_g"].data_ptr(), p["in_b"].data_ptr()
        d.src, d.ld, d.col, d.din, d.n_layers, d.act, d.out, d.hidden, d.ln_eps = joint.data_ptr(), ld, col, din, layers, act, out, 64, 1e-5
        d.w1, d.wh, d.bh = p["w"][0].data_ptr(), p["wh"].data_ptr(), p["bh"].data_ptr()
        for l in range(layers):
            d.bias[l], d.ln_g[l], d.ln_b[l] = p["bias"][l].data_ptr(), p["ln_g"][l].data_ptr(), p["ln_b"][l].data_ptr()
            if l:
                d.w2[l - 1] = p["w"][l].data_ptr()
        for k in ("w_ih", "w_hh", "b_ih", "b_hh", "rnn_g", "rnn_b", "h_in"):
            setattr(e, k, p[k].data_ptr())
        o = dict(y=_guarded(rows * out), h_out=_guarded(rows * 64))
        e.mask, e.h_out, d.y = mask.data_ptr(), o["h_out"][1].data_ptr(), o["y"][1].data_ptr()
        if actor:
            o.update(noise=torch.empty(rows, out, device=DEV).exponential_(generator=g), actions=_guarded(rows, torch.int64),
                     logp=_guarded(rows))
            d.noise, d.actions, d.logp = o["noise"].data_ptr(), o["actions"][1].data_ptr(), o["logp"][1].data_ptr()
        keep.append(((layers, act, out, actor), p, (joint[:, col:col + din], p["h_in"], mask), o))
    lib = _native.lib()
    table = torch.empty(lib.mappo_grouped_rnn_table_bytes(len(specs)), dtype=torch.uint8, device=DEV)
    assert lib.mappo_grouped_rnn_prepare(nets, len(specs), table.data_ptr()) == 0
    assert lib.mappo_grouped_rnn_forward(table.data_ptr(), len(specs), rows, _native.stream_of(DEV)) == 0
    torch.cuda.synchronize()
    return keep


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64_and_k14(name):
    """Head outputs and new states under the 4 x judge against the float64 expression of the network (yardstick: the same
    expression in float32); nothing written outside the outputs; actions and log-probabilities bit for bit
    ``mappo_categorical_sample``'s on the logits the launch wrote with the same noise."""
    lib = _native.lib()
    for i, ((layers, act, out, actor), p, ins, o) in enumerate(_launch(name)):
        y32, h32 = _reference(*ins, p, layers, act, torch.float32)
        y64, h64 = _reference(*ins, p, layers, act, torch.float64)
        kind = "k19rnn.logits" if actor else "k19rnn.values"
        JUDGE.check(kind, o["y"][1].view(-1, out), y32, y64, FLOOR[kind], what=name)
        JUDGE.check("k19rnn.state", o["h_out"][1].view(-1, 64), h32, h64, FLOOR["k19rnn.state"], what=name)
        for flat, inner in (v for v in o.values() if isinstance(v, tuple)):
            edge = torch.cat([flat[:PAD], flat[-PAD:]])
            assert bool(edge.isnan().all() if flat.is_floating_point() else (edge == -7).all()), (name, i)
            assert bool(inner.isfinite().all() if flat.is_floating_point() else ((inner >= 0) & (inner < out)).all()), (name, i)
        if actor:
            rows = ins[0].shape[0]
            actions, logp = torch.empty(rows, dtype=torch.int64, device=DEV), torch.empty(rows, device=DEV)
            assert lib.mappo_categorical_sample(o["y"][1].data_ptr(), None, o["noise"].data_ptr(), actions.data_ptr(),
                                                logp.data_ptr(), rows, out, _native.stream_of(DEV)) == 0
            assert torch.equal(actions, o["actions"][1]) and torch.equal(logp, o["logp"][1]), (name, i)


def _run(tmp_path, graph):
    """train_mpe with the route on: 3-agent simple_adversary, recurrent policies, one rollout of 8 threads, one update."""
    from onpolicy.scripts.train import train_mpe
    argv = ("--env_name MPE --algorithm_name rmappo --experiment_name check --scenario_name simple_adversary --num_agents 3 "
            "--num_landmarks 2 --seed 1 --n_training_threads 1 --n_rollout_threads 8 --num_mini_batch 1 --episode_length 25 "
            "--num_env_steps 200 --ppo_epoch 2 --gain 0.01 --lr 7e-4 --critic_lr 7e-4 --share_policy --hidden_size 64 "
            "--use_wandb --log_interval 1 --use_device_env").split()
    threads = torch.get_num_threads()
    with pytest.MonkeyPatch.context() as mp:
        for k, v in dict(MAPPO_RESULTS_DIR=str(tmp_path / graph), MAPPO_ROLLOUT_GRAPH=graph, MAPPO_GROUPED_ROLLOUT="1",
                         MAPPO_GROUPED_ROLLOUT_RNN="1").items():
            mp.setenv(k, v)
        try:
            return train_mpe.main(argv)
        finally:
            torch.set_num_threads(threads)


@pytest.fixture(scope="module")
def eager_runner(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("eager"), "0")


def test_recurrent_grouped_route_captured_equals_eager(tmp_path, eager_runner):
    """With both switches the captured rollout leaves in every agent's buffer what the eager loop of the same route leaves,
    bit for bit, RNN states included; a step is one recurrent K19 call and no per-agent forward, GRU or sample; with the
    first switch alone recurrent policies stay on the per-agent body."""
    captured, eager = _run(tmp_path, "1"), eager_runner
    rg = captured.rollout_graph
    assert rg is not None and rg.graph is not None and rg.grouped is not None and rg.grouped.recurrent and rg.replays == 25
    assert eager.rollout_graph is None and eager._grouped and eager._grouped.recurrent
    for agent, (got, want) in enumerate(zip(captured.buffer, eager.buffer)):
        for name in ("share_obs", "obs", "actions", "rewards", "masks", "value_preds", "action_log_probs", "rnn_states",
                     "rnn_states_critic"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (agent, name)
        assert bool(got.rnn_states[1:].abs().sum() > 0), agent
    _native.count_calls(True)
    try:
        eager.collect(0)
        counts = [_native.calls().get(k, 0) for k in ("mappo_grouped_rnn_forward", "mappo_mlp_forward", "mappo_gru_seq_forward",
                                                      "mappo_categorical_sample")]
    finally:
        _native.count_calls(False)
    assert counts == [1, 0, 0, 0], counts
    from onpolicy.runner.separated import rollout_graph
    with pytest.MonkeyPatch.context() as mp:        # the first switch alone: the same runner's step, captured per agent
        mp.setenv("MAPPO_GROUPED_ROLLOUT", "1")
        mp.delenv("MAPPO_GROUPED_ROLLOUT_RNN", raising=False)
        first_only = rollout_graph.build(eager)
    assert first_only is not None and first_only.grouped is None


def test_recurrent_grouped_step_agrees_with_the_per_agent_path(eager_runner):
    """Values, logits and both new states of one grouped step against the per-agent launches (K9 trunk, K12 GRU with the head
    inside) on the same observations, states, masks and weights.  Bound: the sum of the paths' errors against float64, each
    relative to the output's scale -- K9's 3e-5 (tests/test_gpu_mlp.py holds its forward to 3e-5 max|y| + 1e-7), K12's
    (tests/test_gpu_gru_seq.py: a head's output to 3e-5 max|logits|, h_last to 2e-5 absolute) and the recurrent K19's
    measured 1.00e-6 (values) / 1.15e-6 (logits) / 9.4e-7 (states)."""
    from onpolicy.algorithms.utils import grouped_rollout
    r = eager_runner
    joint = r.buffer[0].share_obs[1].contiguous()
    g = grouped_rollout.GroupedRollout(r.policy, r.envs.obs_dims, joint, r.use_centralized_V, keep_logits=True)
    for i, b in enumerate(r.buffer):
        g.h_a[i].copy_(b.rnn_states[1]), g.h_c[i].copy_(b.rnn_states_critic[1]), g.masks[i].copy_(b.masks[1])
        g.masks[i][::3] = 0.0
    values, _, _, new_a, new_c = g.forward()
    with torch.no_grad():
        for i, po in enumerate(r.policy):
            obs = r.envs.agent_obs(joint, i).contiguous()
            want_v, want_c = po.critic(joint, g.h_c[i], g.masks[i])
            want_l = po.actor.evaluate_logits(obs, g.h_a[i], g.masks[i])
            want_a = po.actor(obs, g.h_a[i], g.masks[i])[2]
            for kind, got, want, k19 in (("values", values[i], want_v, 1.00e-6), ("logits", g.logits[i], want_l, 1.15e-6),
                                         ("actor state", new_a[i], want_a, 9.4e-7), ("critic state", new_c[i], want_c, 9.4e-7)):
                k12 = 2e-5 if "state" in kind else 3e-5 * float(want.abs().max())
                tol = (3e-5 + k19) * float(want.abs().max()) + k12 + 1e-7
                print("agent %d %s: |grouped - per-agent| %.3e, bound %.3e" % (i, kind, float((got - want).abs().max()), tol))
                torch.testing.assert_close(got, want, rtol=0, atol=tol)
