"""-m gpu: Hanabi evaluation on the device (``--use_device_eval``).  K18's two kernels (csrc/mappo_turn.hip) against their
tensor-op specification (runner/shared/hanabi_eval.py) bit for bit on synthetic operands; then the route through
``HanabiRunner._eval_games`` -- host loop, device eval eager, device eval captured -- an evaluation in the middle of training,
and the two scripts.  Nothing here feeds illegal moves: status 255 appears only as a synthetic flags word, which the kernels
merely read."""
import json
import math
import os

import numpy as np
import pytest
import torch

from onpolicy import _native

import hanabi_eval_common as ec
import hanabi_turns_common as common

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _synthetic(n, A, avail_w, rnn_w, recurrent, variant, seed):
    """-> (operands, (action, rnn_new), flags, arena): every output pre-filled with random values; table k has
    (status, can_move) number (k + variant) % 8 of {0, 1, 2, 255} x {0, 1}, score (7 k + variant) % 26 and a random
    can-move bit in its flags word."""
    from onpolicy.runner.shared import hanabi_eval
    g = torch.Generator().manual_seed(seed)
    arena = common.Arena(DEV)
    rnd = lambda *shape: arena.put(torch.randn(*shape, generator=g))        # noqa: E731
    with torch.cuda.device(DEV):
        o = hanabi_eval.EvalOperands(torch.zeros(n, 1, device=DEV), torch.zeros(n, avail_w, device=DEV), A, 1, rnn_w, recurrent)
    k = torch.arange(n)
    combo = (k + variant) % 8
    status = torch.tensor([0, 1, 2, 255])[combo % 4].to(torch.int32)
    score = ((7 * k + variant) % 26).to(torch.int32)
    movable = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    flags = arena.put(status | (movable << 8) | (score << 16))
    o.use_available_actions = rnd(n, avail_w)
    o.rnn_states = rnd(n, A, 1, rnn_w)
    o.can_move = arena.put((combo // 4).to(torch.int32) * torch.randint(1, 3, (n,), generator=g, dtype=torch.int32))
    o.env_actions = arena.put(torch.full((n,), 77, dtype=torch.int32))
    o.moves = arena.put(torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64))
    o.games = arena.put(torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32))
    o.scores = arena.put(torch.randint(-1, 26, (n,), generator=g, dtype=torch.int32))
    o.refused = arena.put(torch.zeros(n, dtype=torch.uint8))
    policy = (arena.put(torch.randint(0, avail_w, (n, 1), generator=g, dtype=torch.int64)), rnd(n, 1, rnn_w))
    return o, policy, flags, arena


def _everything(o, policy, flags):
    return dict(use_available_actions=o.use_available_actions, rnn_states=o.rnn_states, can_move=o.can_move,
                env_actions=o.env_actions, moves=o.moves, games=o.games, scores=o.scores, refused=o.refused,
                action=policy[0], rnn_new=policy[1], flags=flags)


WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 20, 64)
KERNEL_CASES = [(n, A, rec) for n in (1, 3, 193, common.CAP_TABLES + 1) for A in (2, 5) for rec in (False, True)]


def test_widths_cover_every_offset_from_a_16_byte_boundary():
    assert common.CAP_TABLES + 1 == 8193
    assert {w % 4 for w in WIDTHS} == {0, 1, 2, 3} and {(5 * w) % 4 for w in WIDTHS} == {0, 1, 2, 3}


@pytest.mark.parametrize("n,A,recurrent", KERNEL_CASES, ids=["%d-%dp-%s" % (n, A, "rnn" if r else "ff") for n, A, r in KERNEL_CASES])
def test_eval_kernels_equal_their_tensor_op_form(monkeypatch, n, A, recurrent):
    """``eval_begin`` then ``eval_end``: K18 on two copies of the inputs and the framework ops on a third -- every tensor of
    the call equal bit for bit after each of the two (so whatever a case must not touch is untouched: the state of a table
    that sits out, the count and score of a finished table that did not move, the RNN states when the pointers are NULL),
    the two kernel runs equal to each other, the NaN / pattern canaries around every allocation intact.  Width k of
    ``WIDTHS`` is the legal-move row's with agent index k % A, the RNN row's is another one: both take every offset from a
    16-byte boundary, every agent index occurs.  Every (status, can_move) of {0, 1, 2, 255} x {0, 1} occurs in every case:
    at n < 8 over 8 variants of the inputs, else in each of 2."""
    from onpolicy.runner.shared import hanabi_eval
    widths = WIDTHS if n <= 193 else (1, 6, 7, 64)
    for i, avail_w in enumerate(widths):
        agent, rnn_w = i % A, widths[(i + len(widths) // 2) % len(widths)]
        for variant in range(8 if n < 8 else 2):
            runs = []
            for form in ("kernel", "kernel", "ops"):
                monkeypatch.setenv("MAPPO_TURN_KERNELS", "0" if form == "ops" else "1")
                o, policy, flags, arena = _synthetic(n, A, avail_w, rnn_w, recurrent, variant, seed=11 * n + variant + i)
                before = {k: v.clone() for k, v in _everything(o, policy, flags).items()}
                _native.count_calls(True)
                hanabi_eval.eval_begin(o, agent, *policy)
                after_begin = {k: v.clone() for k, v in _everything(o, policy, flags).items()}
                hanabi_eval.eval_end(o, agent, flags)
                calls = _native.calls()
                _native.count_calls(False)
                assert calls == ({"mappo_hanabi_eval_begin": 1, "mappo_hanabi_eval_end": 1} if form == "kernel" else {})
                torch.cuda.synchronize()
                assert arena.canaries_intact(), (form, agent, variant)
                runs.append((after_begin, _everything(o, policy, flags), before))
            what = "agent %d, widths %d / %d, variant %d" % (agent, avail_w, rnn_w, variant)
            for stage, name in ((0, "eval_begin"), (1, "eval_end")):
                common.same_bits(runs[0][stage], runs[2][stage], "%s, %s: kernel vs tensor ops" % (what, name))
                common.same_bits(runs[0][stage], runs[1][stage], "%s, %s: kernel twice" % (what, name))
            # what the specification itself must say (so that equality with it means something)
            before, begun, spec = runs[2][2], runs[2][0], runs[2][1]
            m, st = before["can_move"] != 0, before["flags"] & 0xff
            idle_done = ~m & (st == 1)              # finished per the flags word, but the table did not move: not counted
            assert torch.equal(spec["games"][idle_done], before["games"][idle_done])
            assert torch.equal(spec["scores"][idle_done], before["scores"][idle_done])
            assert torch.equal(spec["use_available_actions"][idle_done], before["use_available_actions"][idle_done])
            assert torch.equal(spec["games"][m & (st == 1)], before["games"][m & (st == 1)] + 1)
            assert bool((begun["env_actions"][~m] == -1).all()) and bool((spec["can_move"][~m | (st != 0)] == 0).all())
            rows = before["rnn_states"].view(torch.int32)
            if recurrent:
                assert torch.equal(spec["rnn_states"][m, agent].view(torch.int32), before["rnn_new"][m].view(torch.int32))
                rows = rows[~m]
                assert torch.equal(spec["rnn_states"][~m].view(torch.int32), rows)
            else:
                assert torch.equal(spec["rnn_states"].view(torch.int32), rows)
            if n >= 8:      # the ground the case claims to cover
                assert all(bool(((st == s) & (m == c)).any()) for s in (0, 1, 2, 255) for c in (False, True))
                assert bool(spec["refused"].any()) and bool((spec["env_actions"] == -1).any())
            if n >= 64:
                assert {int(v) for v in (spec["flags"] >> 16).unique()} == set(range(26))


# ------------------------------------------------------------------------------------------- the route
def _device_tables(players, recurrent=False, **over):
    from onpolicy.envs.hanabi.device import HanabiDeviceVecEnv
    return HanabiDeviceVecEnv(ec.eval_args(players, True, recurrent, **over), ec.EVAL_SEEDS, DEV)


def _replays(runner):
    return sum(g.replays for g in runner.device_eval.graphs)


@pytest.mark.parametrize("players", [2, 3])
def test_host_eager_and_captured_evaluations_agree_with_a_batch_independent_policy(tmp_path, monkeypatch, players):
    """Two evaluations in a row with the recurrent stub policy (lowest legal move; RNN state += action + 1: exact and
    elementwise, so CPU and GPU agree): the untouched host ``_eval_games``, the device eval's eager loop and its captured
    moves -- sorted scores, mean, number of moves and every (table, player)'s final RNN state identical; every table
    finished exactly once; building the graphs does not show in the games."""
    host = ec.play_host(tmp_path / "host", players, True, DEV)
    assert all(h["moves"] > 0 for h in host)
    monkeypatch.setenv("MAPPO_EVAL_GRAPH", "0")
    envs = _device_tables(players, True)
    runner, eager = ec.play_device(tmp_path / "eager", players, True, DEV, envs)
    assert runner.device_eval.graphs is None
    envs.close()
    monkeypatch.setenv("MAPPO_EVAL_GRAPH", "1")
    envs = _device_tables(players, True)
    runner, captured = ec.play_device(tmp_path / "captured", players, True, DEV, envs)
    assert runner.device_eval.graphs is not None and _replays(runner) == players * sum(c["rounds"] for c in captured)
    envs.close()
    ec.assert_same_evaluations(host, eager, "host vs device eval (eager)")
    ec.assert_same_evaluations(host, captured, "host vs device eval (captured)")
    for run in (eager, captured):
        for ev in run:
            assert (ev["games"] == 1).all() and (ev["by_table"] >= 0).all()
    for a, b in zip(eager, captured):
        assert np.array_equal(a["by_table"], b["by_table"])


REAL_POLICIES = [("mlp64", False, dict(hidden=64)), ("rnn64", True, dict(hidden=64)), ("mlp512", False, dict(hidden=512, layer_N=2))]


@pytest.mark.parametrize("tag,recurrent,shape", REAL_POLICIES, ids=[p[0] for p in REAL_POLICIES])
def test_captured_equals_eager_and_kernels_equal_tensor_ops_with_the_real_policy(tmp_path, monkeypatch, tag, recurrent, shape):
    """The real policy (K14 mode for the deterministic action; at hidden 512 K15, its row threshold lowered to the test's 7
    rows), two evaluations in a row: captured moves against the eager loop (``MAPPO_EVAL_GRAPH=0``) and K18 against
    ``MAPPO_TURN_KERNELS=0`` -- scores per table, counters and final RNN states bit for bit.  Equality with the host loop is
    NOT asserted: there the policy's rows are computed in another batch (the movers only), and whether the last bit of a
    row is independent of the batch is unmeasured; the two means are printed."""
    monkeypatch.setenv("MAPPO_LINEAR512_MIN_ROWS", "1")
    runs = {}
    for way, graph, kernels in (("captured", "1", "1"), ("eager", "0", "1"), ("ops", "0", "0")):
        monkeypatch.setenv("MAPPO_EVAL_GRAPH", graph)
        monkeypatch.setenv("MAPPO_TURN_KERNELS", kernels)
        envs = _device_tables(2, recurrent, **shape)
        _native.count_calls(True)
        runner, runs[way] = ec.play_device(tmp_path / way, 2, recurrent, DEV, envs, stub=False, **shape)
        calls = _native.calls()
        _native.count_calls(False)
        assert (runner.device_eval.graphs is not None) == (way == "captured")
        assert calls.get("mappo_categorical_mode", 0) > 0, sorted(calls)
        assert (calls.get("mappo_hanabi_eval_begin", 0) > 0) == (kernels == "1")
        if way == "captured":
            assert _replays(runner) == 2 * sum(c["rounds"] for c in runs[way])
        if tag == "mlp512" and way == "eager":
            assert any(k.startswith("mappo_linear512_forward") for k in calls), sorted(calls)
        assert runner.device_eval.ops.recurrent == recurrent
        envs.close()
    for other in ("captured", "ops"):
        ec.assert_same_evaluations(runs["eager"], runs[other], "eager vs %s (%s)" % (other, tag))
        for a, b in zip(runs["eager"], runs[other]):
            assert np.array_equal(a["by_table"], b["by_table"]) and np.array_equal(a["games"], b["games"])
    assert all((ev["games"] == 1).all() for ev in runs["eager"])
    if recurrent:
        assert runs["eager"][0]["rnn"].any()
    monkeypatch.setenv("MAPPO_TURN_KERNELS", "1")
    host = ec.play_host(tmp_path / "host", 2, recurrent, DEV, stub=False, **shape)
    print("%s: mean score host %s, device %s" % (tag, [h["mean"] for h in host], [e["mean"] for e in runs["eager"]]))


def test_an_evaluation_in_the_middle_of_training_touches_nothing_else_and_reads_only_counters(tmp_path, monkeypatch):
    """Training tables on the device too (the default device route), three buffer steps played, then ``eval()``: the buffer,
    the training tables' ``table_state`` and torch's device generator are as before.  During the evaluation ``read_flags``
    raises -- nothing but the counter block is read back -- and the reads are counted: at most ceil(rounds / P) + 1."""
    from onpolicy.envs.hanabi.device import HanabiDeviceBatch, HanabiDeviceVecEnv
    from onpolicy.runner.shared import hanabi_eval
    poll = 2
    monkeypatch.setenv("MAPPO_HANABI_EVAL_POLL", str(poll))
    args = ec.eval_args(2, True)
    envs, eval_envs = HanabiDeviceVecEnv(args, common.SEEDS, DEV), HanabiDeviceVecEnv(args, ec.EVAL_SEEDS, DEV)
    runner = ec.make_runner(args, envs, eval_envs, DEV, tmp_path / "run")
    assert runner.route.name == "device_tables"
    runner.begin_rollout()
    for step in range(3):
        runner.collect(step)
        runner.insert_and_restart()
    reads = {"n": 0}
    read_counters = hanabi_eval.EvalOperands.read_counters

    def no_readback(self, rows=None):
        raise AssertionError("the device evaluation read the flags words back")

    def counting(self):
        reads["n"] += 1
        return read_counters(self)
    monkeypatch.setattr(HanabiDeviceBatch, "read_flags", no_readback)
    monkeypatch.setattr(hanabi_eval.EvalOperands, "read_counters", counting)
    for evaluation in range(2):         # the first builds the graphs, the second only replays
        torch.cuda.synchronize()
        before = {k: getattr(runner.buffer, k).clone() for k in common.BUFFER_FIELDS}
        tables, rng = envs.table_state.clone(), torch.cuda.get_rng_state(DEV).clone()
        reads["n"] = 0
        runner.eval(0)
        torch.cuda.synchronize()
        route = runner.device_eval
        assert route.graphs is not None and (route.counters["games"] == 1).all()
        assert reads["n"] == route.readbacks <= math.ceil(route.rounds / float(poll)) + 1
        for k, v in before.items():
            assert torch.equal(getattr(runner.buffer, k).view(torch.int32), v.view(torch.int32)), k
        assert torch.equal(envs.table_state, tables) and torch.equal(torch.cuda.get_rng_state(DEV), rng)
    logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    assert [r["tag"] for r in logged].count("eval_average_score") == 2
    envs.close()
    eval_envs.close()


def test_train_and_eval_scripts_with_device_eval(tmp_path, monkeypatch):
    """train_hanabi_forward --use_eval --use_device_eval end to end, with and without --use_device_env (the flags are
    independent); then eval_hanabi --use_device_eval --eval_games 14 on the model the second run saved."""
    from onpolicy.scripts.eval import eval_hanabi
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    common_argv = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Small", "--num_agents", "2", "--algorithm_name", "mappo",
                   "--hidden_size", "64", "--use_wandb", "--n_training_threads", "1", "--use_eval", "--n_eval_rollout_threads", "7",
                   "--seed", "3", "--use_device_eval"]
    argv = common_argv + ["--n_rollout_threads", "7", "--episode_length", "8", "--num_env_steps", str(3 * 7 * 8), "--ppo_epoch", "2",
                          "--log_interval", "1", "--eval_interval", "2"]
    for extra, tables in ((["--use_device_env"], "HanabiDeviceVecEnv"), ([], "HanabiBatchVecEnv")):
        runner = train_hanabi_forward.main(argv + extra)
        assert type(runner.envs).__name__ == tables and type(runner.eval_envs).__name__ == "HanabiDeviceVecEnv"
        assert runner.device_eval is not None and runner.device_eval.graphs is not None
        assert (runner.device_eval.counters["games"] == 1).all()
        logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
        assert {"value_loss", "eval_average_score"} <= {r["tag"] for r in logged}
        assert [r["tag"] for r in logged].count("eval_average_score") == 2          # episodes 0 and 2
        runner.envs.close()
        runner.eval_envs.close()
    assert os.path.exists(os.path.join(runner.save_dir, "actor.pt"))
    score = eval_hanabi.main(common_argv + ["--n_rollout_threads", "1", "--eval_games", "14", "--model_dir", str(runner.save_dir)])
    assert 0.0 <= float(score) <= 10.0
