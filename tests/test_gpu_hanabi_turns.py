"""-m gpu: the host-free Hanabi route ("device turns").  K17's two kernels (csrc/mappo_turn.hip) against their tensor-op
specification (runner/shared/hanabi_turns.py) bit for bit on synthetic inputs; then the route through ``HanabiRunner`` --
default device route, device turns eager, device turns captured -- and the train script.  Nothing here feeds illegal moves
in bulk: status 255 appears only as a synthetic flags word, which the kernels merely read."""
import ctypes
import json
import os
import types

import pytest
import torch

from onpolicy import _native
from onpolicy.envs.hanabi import batch as hb

import hanabi_turns_common as common

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _widths(game, players):
    """(obs, share_obs, available_actions) row widths of the named game in the default share mode."""
    r = hb.Rules(**hb.rules_for(game, players))
    rules = tuple(int(getattr(r, name)) for name, _ in hb.Rules._fields_)
    dims = (ctypes.c_int32 * 5)()
    _native.check(_native.lib().mappo_hanabi_dims(*(rules + (ctypes.addressof(dims),))), "mappo_hanabi_dims")
    P, moves, obs_len, own_len = (int(v) for v in dims[:4])
    return obs_len + P, own_len + obs_len + P, moves


def _synthetic(n, A, widths, variant, seed):
    """-> (operands, policy outputs, env outputs, arena): turn tensors pre-filled with random values; table k has
    (status, can_move) number (k + variant) % 8 of {0, 1, 2, 255} x {0, 1} and score (7 k + variant) % 26."""
    from onpolicy.runner.shared import hanabi_turns
    g = torch.Generator().manual_seed(seed)
    arena = common.Arena(DEV)
    rnd = lambda *shape: arena.put(torch.randn(*shape, generator=g))        # noqa: E731
    turn = types.SimpleNamespace()
    for name, w in zip(hanabi_turns.ROW_FIELDS, widths):
        setattr(turn, name, rnd(n, A, w))
    for name in hanabi_turns.SCALAR_FIELDS:
        setattr(turn, name, rnd(n, A, 1))
    use = [rnd(n, w) for w in widths]
    with torch.cuda.device(DEV):
        o = hanabi_turns.TurnOperands(turn, *use)
    k = torch.arange(n)
    combo = (k + variant) % 8
    status = torch.tensor([0, 1, 2, 255])[combo % 4].to(torch.int32)
    score = ((7 * k + variant) % 26).to(torch.int32)
    movable = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    flags = arena.put(status | (movable << 8) | (score << 16))
    o.can_move = arena.put((combo // 4).to(torch.int32))
    o.reset_choose = arena.put(torch.randint(0, 2, (n,), generator=g).to(torch.uint8))
    o.env_actions = arena.put(torch.full((n,), 77, dtype=torch.int32))
    o.moves = arena.put(torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64))
    o.games = arena.put(torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32))
    o.score_sum = arena.put(torch.randint(0, 25000, (n,), generator=g, dtype=torch.int32))
    o.refused = arena.put(torch.zeros(n, dtype=torch.uint8))
    policy = (rnd(n, 1), arena.put(torch.randint(0, widths[2], (n, 1), generator=g, dtype=torch.int64)), rnd(n, 1))
    env = (flags, rnd(n))
    return o, policy, env, arena


def _everything(o, policy, env):
    from onpolicy.runner.shared import hanabi_turns
    t = o.turn
    named = {k: getattr(t, k) for k in hanabi_turns.ROW_FIELDS + hanabi_turns.SCALAR_FIELDS}
    named.update(use_obs=o.use_obs, use_share_obs=o.use_share_obs, use_available_actions=o.use_available_actions,
                 can_move=o.can_move, reset_choose=o.reset_choose, env_actions=o.env_actions, moves=o.moves,
                 games=o.games, score_sum=o.score_sum, refused=o.refused, value=policy[0], action=policy[1],
                 logp=policy[2], flags=env[0], rewards_env=env[1])
    return named


KERNEL_CASES = [(game, A, n) for game, A in (("Hanabi-Small", 2), ("Hanabi-Full", 2), ("Hanabi-Small", 5), ("Hanabi-Full", 5))
                for n in (1, 63, 64, 65, 193)] + [("Hanabi-Small", 2, common.CAP_TABLES + 1), ("synthetic", 2, 65)]


def test_row_widths_cover_every_offset_from_a_16_byte_boundary():
    widths = {w for game, A, _ in KERNEL_CASES for w in (_widths(game, A) if game != "synthetic" else (6, 8, 3))}
    assert {w % 4 for w in widths} == {0, 1, 2, 3}, sorted(widths)


@pytest.mark.parametrize("game,A,n", KERNEL_CASES, ids=["%s-%dp-%d" % c for c in KERNEL_CASES])
def test_turn_kernels_equal_their_tensor_op_form(monkeypatch, game, A, n):
    """``turn_begin`` then ``turn_end`` for agent first / middle / last: K17 on two copies of the inputs and the framework
    ops on a third -- every tensor of the call equal bit for bit after each of the two (so whatever a case must not touch
    is untouched), the two kernel runs equal to each other, the NaN / pattern canaries around every allocation intact.
    Every (status, can_move) of {0, 1, 2, 255} x {0, 1} and the scores 0..25 occur in every case: at n < 8 over 8 variants
    of the inputs, else in each of 2."""
    from onpolicy.runner.shared import hanabi_turns
    widths = (6, 8, 3) if game == "synthetic" else _widths(game, A)
    for agent in sorted({0, A // 2, A - 1}):
        for variant in range(8 if n < 8 else 2):
            runs = []
            for form in ("kernel", "kernel", "ops"):
                monkeypatch.setenv("MAPPO_TURN_KERNELS", "0" if form == "ops" else "1")
                o, policy, env, arena = _synthetic(n, A, widths, variant, seed=11 * n + variant)
                _native.count_calls(True)
                hanabi_turns.turn_begin(o, agent, *policy)
                after_begin = {k: v.clone() for k, v in _everything(o, policy, env).items()}
                hanabi_turns.turn_end(o, agent, *env)
                calls = _native.calls()
                _native.count_calls(False)
                assert calls == ({"mappo_hanabi_turn_begin": 1, "mappo_hanabi_turn_end": 1} if form == "kernel" else {})
                torch.cuda.synchronize()
                assert arena.canaries_intact(), (form, agent, variant)
                runs.append((after_begin, _everything(o, policy, env), arena))
            what = "agent %d, variant %d" % (agent, variant)
            for stage, name in ((0, "turn_begin"), (1, "turn_end")):
                common.same_bits(runs[0][stage], runs[2][stage], "%s, %s: kernel vs tensor ops" % (what, name))
                common.same_bits(runs[0][stage], runs[1][stage], "%s, %s: kernel twice" % (what, name))
            if n >= 8:      # the ground the case claims to cover
                spec = runs[2][1]
                st = spec["flags"] & 0xff
                assert all(bool(((st == s) & (runs[2][0]["can_move"] == m)).any()) for s in (0, 1, 2, 255) for m in (0, 1))
                assert bool(spec["refused"].any()) and bool((spec["env_actions"] == -1).any())
            if n >= 64:
                assert {int(v) for v in (runs[2][1]["flags"] >> 16).unique()} == set(range(26))


# ------------------------------------------------------------------------------------------- the route
def _device_runner(tmp_path, tag, turns, stub, players=2, **arg_over):
    from onpolicy.envs.hanabi.device import HanabiDeviceVecEnv
    args = common.hanabi_args(players, **arg_over)
    if turns:
        args.use_device_turns = True
    envs = HanabiDeviceVecEnv(args, common.SEEDS, DEV)
    return common.make_runner(args, envs, DEV, tmp_path / tag, stub=stub)


def test_three_routes_agree_with_a_batch_independent_policy(tmp_path, monkeypatch, gold):
    """Default device route, device turns eager, device turns captured, all with the CPU test's stub policy (lowest legal
    move): buffers, current rows, move / game counters and the mean score bit-identical -- with each other and with the
    recording of the host-tables route on the CPU (tests/golden/hanabi_route_cases.npz: the stub's arithmetic is exact
    and elementwise, so CPU and GPU agree)."""
    default = common.play(_device_runner(tmp_path, "default", False, True))
    assert default[1]["games"] >= 20
    common.assert_same(common.recorded(gold, 2), default, "recorded host-tables route (CPU) vs default device route")
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    runner = _device_runner(tmp_path, "eager", True, True)
    eager = common.play(runner)
    assert runner.route.name == "device_turns" and runner.turn_graphs is None
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "1")
    runner = _device_runner(tmp_path, "captured", True, True)
    captured = common.play(runner)
    assert runner.turn_graphs is not None and runner.turn_graphs.replays == common.T * 2
    common.assert_same(default, eager, "default device route vs device turns (eager)")
    common.assert_same(default, captured, "default device route vs device turns (captured)")


def _two_episodes(tmp_path, tag, **arg_over):
    """``run()`` over two episodes, the update between them included -> (buffers + rows + parameters, counters, logged)."""
    runner = _device_runner(tmp_path, tag, True, False, **arg_over)
    runner.run()
    torch.cuda.synchronize()
    out, counters = common.outcome(runner)
    out["params"] = torch.cat([p.detach().reshape(-1) for p in runner.policy.actor.parameters()] +
                              [p.detach().reshape(-1) for p in runner.policy.critic.parameters()]).cpu().numpy()
    logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    graphs = runner.turn_graphs
    runner.envs.close()
    return (out, counters), [sorted(r.items()) for r in logged if "score" in r["tag"]], graphs


def test_captured_equals_eager_and_kernels_equal_tensor_ops_with_the_real_policy(tmp_path, monkeypatch):
    """The real policy and sampler, hidden 64: captured moves against the eager loop (``MAPPO_TURN_GRAPH=0``), and K17
    against ``MAPPO_TURN_KERNELS=0``, over two episodes with the update between them -- buffers, rows, counters, logged
    scores and the parameters bit for bit.  Building the graphs does not show in the trajectories."""
    captured, captured_log, graphs = _two_episodes(tmp_path, "captured")
    assert graphs is not None and graphs.replays == 2 * common.T * 2
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    eager, eager_log, graphs = _two_episodes(tmp_path, "eager")
    assert graphs is None
    monkeypatch.setenv("MAPPO_TURN_KERNELS", "0")
    ops, ops_log, _ = _two_episodes(tmp_path, "ops")
    assert captured[1]["moves"] > 0 and captured[1]["games"] > 0
    common.assert_same(eager, captured, "eager vs captured")
    common.assert_same(eager, ops, "K17 vs tensor ops")
    assert captured_log == eager_log == ops_log and len(eager_log) > 0


def test_captured_equals_eager_at_hidden_512(tmp_path, monkeypatch):
    """Hidden 512 x 2 (K15 inside the captured move; its row threshold lowered to the test's 7 rows)."""
    monkeypatch.setenv("MAPPO_LINEAR512_MIN_ROWS", "1")
    captured, captured_log, graphs = _two_episodes(tmp_path, "captured", hidden=512, layer_N=2)
    assert graphs is not None and graphs.replays == 2 * common.T * 2
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    _native.count_calls(True)
    eager, eager_log, _ = _two_episodes(tmp_path, "eager", hidden=512, layer_N=2)
    calls = _native.calls()
    _native.count_calls(False)
    assert any(k.startswith("mappo_linear512_forward") for k in calls), sorted(calls)
    common.assert_same(eager, captured, "eager vs captured, hidden 512")
    assert captured_log == eager_log


def test_a_captured_episode_reads_nothing_back(tmp_path, monkeypatch):
    """``read_flags`` raises; one whole episode on the captured route replays T x A graphs.  The T buffer steps also run
    under ``torch.cuda.set_sync_debug_mode("error")`` where this build implements it (a synchronising call raises then);
    where it does not -- the call itself fails -- the patched ``read_flags`` and the replay count are the check."""
    from onpolicy.envs.hanabi.device import HanabiDeviceBatch

    def no_readback(self, rows=None):
        raise AssertionError("the device-turns route read the flags words back")
    runner = _device_runner(tmp_path, "captured", True, False)
    runner.begin_rollout()
    assert runner.turn_graphs is not None
    monkeypatch.setattr(HanabiDeviceBatch, "read_flags", no_readback)
    try:
        torch.cuda.set_sync_debug_mode("error")
        guarded = True
    except Exception as exc:
        print("set_sync_debug_mode is not available on this build: %r" % (exc,))
        guarded = False
    try:
        for step in range(common.T):
            runner.collect(step)
            runner.insert_and_restart()
    finally:
        if guarded:
            torch.cuda.set_sync_debug_mode("default")
    print("buffer steps ran under sync debug mode 'error': %s" % guarded)
    assert runner.turn_graphs.replays == common.T * 2
    counters = runner.read_turn_counters()
    assert runner.true_total_num_steps > 0 and counters["games"] >= 0
    runner.envs.close()


def test_train_script_with_device_turns(tmp_path, monkeypatch):
    """train_hanabi_forward --use_device_env --use_device_turns end to end at the sizes of
    test_train_script_with_device_tables: value_loss and average_score logged, moves counted; a second run with
    ``MAPPO_TURN_GRAPH=0`` logs the same scores and ends with the same parameters."""
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    argv = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Small", "--num_agents", "2", "--algorithm_name", "mappo",
            "--n_rollout_threads", "7", "--episode_length", "8", "--num_env_steps", str(3 * 7 * 8), "--ppo_epoch", "2",
            "--hidden_size", "64", "--use_wandb", "--log_interval", "1", "--n_training_threads", "1", "--use_eval",
            "--n_eval_rollout_threads", "2", "--eval_interval", "2", "--seed", "3", "--use_device_env", "--use_device_turns"]
    runs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("MAPPO_TURN_GRAPH", graph)
        runner = train_hanabi_forward.main(argv)
        assert runner.route.name == "device_turns" and (runner.turn_graphs is not None) == (graph == "1")
        assert type(runner.envs).__name__ == "HanabiDeviceVecEnv" and type(runner.eval_envs).__name__ == "HanabiBatchVecEnv"
        assert runner.true_total_num_steps > 0
        logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
        assert {"value_loss", "average_score", "eval_average_score"} <= {r["tag"] for r in logged}
        params = torch.cat([p.detach().reshape(-1) for p in runner.policy.actor.parameters()]).cpu()
        runs.append(([sorted(r.items()) for r in logged if "score" in r["tag"]], params, runner.true_total_num_steps))
        runner.envs.close()
        runner.eval_envs.close()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] and torch.equal(runs[0][1], runs[1][1])
