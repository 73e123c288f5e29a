"""-m gpu: the host-free Hanabi route for RECURRENT policies (``--use_device_turns --use_device_turns_rnn``).  The two
``_rnn`` entry points of K17 (csrc/mappo_turn.hip) against their tensor-op specification (runner/shared/hanabi_turns.py)
bit for bit on synthetic inputs; then the route through ``HanabiRunner`` -- default device route, device turns eager,
device turns captured -- with a recurrent stub and with the real recurrent policies, and the train script.  Nothing here
feeds illegal moves: status 255 appears only as a synthetic flags word, which the kernels merely read."""
import json
import os

import pytest
import torch

from onpolicy import _native

import hanabi_turns_common as common
import test_gpu_hanabi_turns as k17                   # the synthetic operands of K17's own test: built once, there
from hanabi_turns_rnn_common import recurrent_stub_get_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
WIDTHS = (6, 8, 3)                  # obs, share_obs, available_actions: K17's test covers the games' real widths
RNN_WIDTHS = (1, 6, 7, 64, 130)
KERNEL_CASES = [(n, A, w) for n in (1, 3, 65, 193, common.CAP_TABLES + 1) for A in (2, 3, 5) for w in RNN_WIDTHS]
RNN_CALLS = {"mappo_hanabi_turn_begin_rnn": 1, "mappo_hanabi_turn_end_rnn": 1}
K17_CALLS = {"mappo_hanabi_turn_begin": 1, "mappo_hanabi_turn_end": 1}


def test_state_rows_fall_on_every_offset_from_a_16_byte_boundary():
    """A slot row sits at (n * players + agent) * rnn_w floats of a 16-byte aligned array."""
    for w, expect in ((1, {0, 1, 2, 3}), (6, {0, 2}), (7, {0, 1, 2, 3}), (64, {0}), (130, {0, 2})):
        for A in (2, 3, 5):
            assert {((n * A + a) * w) % 4 for n in range(65) for a in range(A)} == expect, (w, A)
    assert {((n * A + a) * w) % 4 for n, A, w in KERNEL_CASES for a in range(A)} == {0, 1, 2, 3}
    assert {w % 4 for w in RNN_WIDTHS} == {0, 1, 2, 3}


def _synthetic(n, A, rnn_w, variant, seed):
    """K17's synthetic operands (tables with every (status, can_move), random turn tensors), made recurrent: random state
    tensors [n, A, 1, rnn_w] and new states [n, 1, rnn_w], drawn on the device (the same for the same seed)."""
    from onpolicy.runner.shared import hanabi_turns
    plain, policy, env, arena = k17._synthetic(n, A, WIDTHS, variant, seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: arena.put(torch.randn(*shape, generator=g, device=DEV))        # noqa: E731
    turn = plain.turn
    turn.rnn_states, turn.rnn_states_critic = rnd(n, A, 1, rnn_w), rnd(n, A, 1, rnn_w)
    with torch.cuda.device(DEV):
        o = hanabi_turns.TurnOperands(turn, plain.use_obs, plain.use_share_obs, plain.use_available_actions, recurrent=True)
    for name in ("can_move", "reset_choose", "env_actions", "moves", "games", "score_sum", "refused"):
        setattr(o, name, getattr(plain, name))
    return o, policy + (rnd(n, 1, rnn_w), rnd(n, 1, rnn_w)), env, arena


def _everything(o, policy, env):
    named = k17._everything(o, policy[:3], env)
    named.update(rnn_states=o.turn.rnn_states, rnn_states_critic=o.turn.rnn_states_critic, rnn_new=policy[3],
                 rnn_new_critic=policy[4])
    return named


@pytest.mark.parametrize("n,A,rnn_w", KERNEL_CASES, ids=["%d-%dp-w%d" % c for c in KERNEL_CASES])
def test_rnn_turn_kernels_equal_their_tensor_op_form(monkeypatch, n, A, rnn_w):
    """``turn_begin`` then ``turn_end`` on recurrent operands for EVERY agent index: the ``_rnn`` kernels on two copies of
    the inputs and the framework ops on a third -- every tensor of the call (all of K17's and both state tensors) equal
    bit for bit after each of the two, the two kernel runs equal to each other, exactly one ``_rnn`` launch per operation
    and no K17 call, the NaN / pattern canaries around every allocation intact.  Every (status, can_move) of
    {0, 1, 2, 255} x {0, 1} occurs in every case: at n < 8 over 8 variants of the inputs, else in each of 2."""
    from onpolicy.runner.shared import hanabi_turns
    for agent in range(A):
        for variant in range(8 if n < 8 else 2):
            runs = []
            for form in ("kernel", "kernel", "ops"):
                monkeypatch.setenv("MAPPO_TURN_KERNELS", "0" if form == "ops" else "1")
                o, policy, env, arena = _synthetic(n, A, rnn_w, variant, seed=11 * n + variant)
                before = {k: getattr(o.turn, k).clone() for k in hanabi_turns.STATE_FIELDS}
                _native.count_calls(True)
                hanabi_turns.turn_begin(o, agent, *policy)
                after_begin = {k: v.clone() for k, v in _everything(o, policy, env).items()}
                hanabi_turns.turn_end(o, agent, *env)
                calls = _native.calls()
                _native.count_calls(False)
                assert calls == (RNN_CALLS if form == "kernel" else {})
                torch.cuda.synchronize()
                assert arena.canaries_intact(), (form, agent, variant)
                runs.append((after_begin, _everything(o, policy, env), before))
            what = "agent %d, variant %d" % (agent, variant)
            for stage, name in ((0, "turn_begin"), (1, "turn_end")):
                common.same_bits(runs[0][stage], runs[2][stage], "%s, %s: kernel vs tensor ops" % (what, name))
                common.same_bits(runs[0][stage], runs[1][stage], "%s, %s: kernel twice" % (what, name))
            if n >= 8:      # the ground the case claims to cover: movers and sitters, running / finished / refused tables
                begun, ended, before = runs[0]
                moved = begun["can_move"] != 0            # (turn_begin leaves can_move as it read it)
                st = ended["flags"] & 0xff
                assert all(bool(((st == s) & (moved == m)).any()) for s in (0, 1, 2, 255) for m in (False, True))
                for k, new in (("rnn_states", "rnn_new"), ("rnn_states_critic", "rnn_new_critic")):
                    slot, old = begun[k][:, agent], before[k][:, agent]
                    assert torch.equal(slot[moved], begun[new][moved]) and torch.equal(slot[~moved], old[~moved]), k
                    others = [a for a in range(A) if a != agent]
                    assert torch.equal(begun[k][:, others], before[k][:, others]), k
                    assert bool((ended[k][st == 1] == 0).all()) and torch.equal(ended[k][st != 1], begun[k][st != 1]), k


# ------------------------------------------------------------------------------------------- the route
def _device_runner(tmp_path, tag, turns, stub, kind="use_recurrent_policy", **arg_over):
    from onpolicy.envs.hanabi.device import HanabiDeviceVecEnv
    args = common.hanabi_args(2, **dict({kind: True} if kind else {}, **arg_over))
    if turns:
        args.use_device_turns = args.use_device_turns_rnn = True
    envs = HanabiDeviceVecEnv(args, common.SEEDS, DEV)
    runner = common.make_runner(args, envs, DEV, tmp_path / tag, stub=False)
    if stub:
        runner.trainer.policy.get_actions = recurrent_stub_get_actions
    return runner


def _turn_calls():
    return {k: v for k, v in _native.calls().items() if k.startswith("mappo_hanabi_turn")}


def test_a_move_issues_one_launch_per_operation(tmp_path, monkeypatch):
    """A recurrent move: exactly one ``mappo_hanabi_turn_begin_rnn`` and one ``_end_rnn``, no K17 call; a feed-forward
    move (the second flag given all the same: it changes nothing there): exactly the two K17 calls."""
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    for kind, want in (("use_recurrent_policy", RNN_CALLS), (None, K17_CALLS)):
        runner = _device_runner(tmp_path, "calls_%s" % kind, True, False, kind=kind)
        runner.begin_rollout()
        assert runner.route.name == "device_turns" and runner.turn_graphs is None
        assert runner.route.ops.recurrent == (kind is not None)
        runner.trainer.prep_rollout()
        _native.count_calls(True)
        runner.route.move(1)
        calls = _turn_calls()
        _native.count_calls(False)
        torch.cuda.synchronize()
        assert calls == want, kind
        runner.envs.close()


def test_three_routes_agree_with_a_recurrent_batch_independent_policy(tmp_path, monkeypatch):
    """Default device route, device turns eager, device turns captured, all with the CPU test's recurrent stub: buffers
    (both RNN state fields among them), current rows, move / game counters and the mean score bit-identical."""
    default = common.play(_device_runner(tmp_path, "default", False, True))
    assert default[1]["games"] >= 20 and abs(default[0]["rnn_states"]).max() > 0
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    runner = _device_runner(tmp_path, "eager", True, True)
    eager = common.play(runner)
    assert runner.route.name == "device_turns" and runner.turn_graphs is None and runner.route.ops.recurrent
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "1")
    runner = _device_runner(tmp_path, "captured", True, True)
    captured = common.play(runner)
    assert runner.turn_graphs is not None and runner.turn_graphs.replays == common.T * 2
    common.assert_same(default, eager, "default device route vs recurrent device turns (eager)")
    common.assert_same(default, captured, "default device route vs recurrent device turns (captured)")


def _two_episodes(tmp_path, tag, **arg_over):
    """``run()`` over two episodes, the update between them included -> (buffers + rows + parameters, counters, logged)."""
    runner = _device_runner(tmp_path, tag, True, False, **arg_over)
    assert runner.route.name == "device_turns"
    runner.run()
    torch.cuda.synchronize()
    out, counters = common.outcome(runner)
    out["params"] = torch.cat([p.detach().reshape(-1) for p in runner.policy.actor.parameters()] +
                              [p.detach().reshape(-1) for p in runner.policy.critic.parameters()]).cpu().numpy()
    logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    graphs = runner.turn_graphs
    runner.envs.close()
    return (out, counters), [sorted(r.items()) for r in logged if "score" in r["tag"]], graphs


def test_captured_equals_eager_and_kernels_equal_tensor_ops_with_the_real_recurrent_policy(tmp_path, monkeypatch):
    """The real recurrent policy and sampler, hidden 64, chunks of 4: captured moves against the eager loop
    (``MAPPO_TURN_GRAPH=0``), and the ``_rnn`` kernels against ``MAPPO_TURN_KERNELS=0``, over two episodes with the update
    between them -- buffers, rows, counters, logged scores and the parameters after the update bit for bit."""
    captured, captured_log, graphs = _two_episodes(tmp_path, "captured", data_chunk_length=4)
    assert graphs is not None and graphs.replays == 2 * common.T * 2
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    _native.count_calls(True)
    eager, eager_log, graphs = _two_episodes(tmp_path, "eager", data_chunk_length=4)
    calls = _turn_calls()
    _native.count_calls(False)
    assert graphs is None
    assert calls == {k: 2 * common.T * 2 for k in RNN_CALLS}
    monkeypatch.setenv("MAPPO_TURN_KERNELS", "0")
    ops, ops_log, _ = _two_episodes(tmp_path, "ops", data_chunk_length=4)
    assert captured[1]["moves"] > 0 and captured[1]["games"] > 0
    assert abs(captured[0]["rnn_states"]).max() > 0 and abs(captured[0]["rnn_states_critic"]).max() > 0
    common.assert_same(eager, captured, "eager vs captured")
    common.assert_same(eager, ops, "K17 (recurrent) vs tensor ops")
    assert captured_log == eager_log == ops_log and len(eager_log) > 0


def test_captured_equals_eager_at_hidden_512(tmp_path, monkeypatch):
    """Hidden 512 x 2, recurrent (the eval script's model; K15's row threshold lowered to the test's 7 rows)."""
    monkeypatch.setenv("MAPPO_LINEAR512_MIN_ROWS", "1")
    captured, captured_log, graphs = _two_episodes(tmp_path, "captured", hidden=512, layer_N=2, data_chunk_length=4)
    assert graphs is not None and graphs.replays == 2 * common.T * 2
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    eager, eager_log, _ = _two_episodes(tmp_path, "eager", hidden=512, layer_N=2, data_chunk_length=4)
    assert abs(captured[0]["rnn_states"]).max() > 0
    common.assert_same(eager, captured, "eager vs captured, hidden 512, recurrent")
    assert captured_log == eager_log


def test_captured_equals_eager_with_the_naive_recurrent_policy(tmp_path, monkeypatch):
    captured, captured_log, graphs = _two_episodes(tmp_path, "captured", kind="use_naive_recurrent_policy")
    assert graphs is not None and graphs.replays == 2 * common.T * 2
    monkeypatch.setenv("MAPPO_TURN_GRAPH", "0")
    eager, eager_log, _ = _two_episodes(tmp_path, "eager", kind="use_naive_recurrent_policy")
    assert abs(captured[0]["rnn_states"]).max() > 0
    common.assert_same(eager, captured, "eager vs captured, naive recurrent")
    assert captured_log == eager_log


def test_a_captured_recurrent_episode_reads_nothing_back(tmp_path, monkeypatch):
    """The method of test_a_captured_episode_reads_nothing_back (tests/test_gpu_hanabi_turns.py): ``read_flags`` raises; one
    whole episode on the captured route replays T x A graphs, under ``torch.cuda.set_sync_debug_mode("error")`` where
    this build implements it."""
    from onpolicy.envs.hanabi.device import HanabiDeviceBatch

    def no_readback(self, rows=None):
        raise AssertionError("the device-turns route read the flags words back")
    runner = _device_runner(tmp_path, "captured", True, False)
    runner.begin_rollout()
    assert runner.turn_graphs is not None and runner.route.ops.recurrent
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


def test_train_script_with_recurrent_device_turns(tmp_path, monkeypatch):
    """train_hanabi_forward --use_device_env --use_device_turns --use_device_turns_rnn --use_recurrent_policy end to end
    at ``ARGV``'s sizes: the host-free route with captured moves, value_loss and average_score logged, moves counted.
    (As in the reference's scripts the algorithm name decides the recurrent flags -- ``mappo`` clears them whatever is
    given -- so the recurrent run is ``--algorithm_name rmappo``: the later of two occurrences counts.)"""
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    argv = common.ARGV + ["--algorithm_name", "rmappo", "--ppo_epoch", "2", "--hidden_size", "64", "--log_interval", "1",
                          "--n_training_threads", "1", "--seed", "3", "--data_chunk_length", "4", "--use_device_env",
                          "--use_device_turns", "--use_device_turns_rnn", "--use_recurrent_policy"]
    runner = train_hanabi_forward.main(argv)
    assert runner.route.name == "device_turns" and runner.turn_graphs is not None and runner.route.ops.recurrent
    assert runner.all_args.use_recurrent_policy and runner.policy.actor._recurrent
    assert runner.turn_graphs.replays == 2 * common.T * 2 and runner.true_total_num_steps > 0
    logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    assert {"value_loss", "average_score"} <= {r["tag"] for r in logged}
    runner.envs.close()
