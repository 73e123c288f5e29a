"""Hanabi evaluation on the device (``--use_device_eval``: runner/shared/hanabi_eval.py) without a GPU: its eager loop on CPU
tensors against the untouched host ``_eval_games`` on the same stepper, the argument checks and struct layout of K18's C ABI
(include/mappo_hip.h), the scripts' flag and the move bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

from onpolicy import _native

import hanabi_eval_common as ec
import hanabi_turns_common as common
from hanabi_turns_common import host_buffer      # noqa: F401  (a fixture)

CPU = torch.device("cpu")


@pytest.mark.parametrize("players", [2, 3])
def test_device_eval_equals_host_eval_on_host_tables(host_buffer, tmp_path, monkeypatch, players):
    """Hanabi-Small, N = 7, two evaluations in a row (the tables' generators continue), the recurrent stub policy (lowest
    legal move; RNN state += action + 1): the eager device evaluation on the host stepper behind the device env's contract
    against ``HanabiRunner._eval_games`` as it stands -- sorted scores, mean, number of moves and the final RNN state of every
    (table, player) identical; every table finished exactly once; P = 1 and P = 4 alike.  The ground is covered (asserted):
    moves with some tables sitting out while others move, and games of different lengths."""
    host = ec.play_host(tmp_path / "host", players, True, CPU)
    sitters = [sum(1 for m in h["moved"] if m.any() and not m.all()) for h in host]
    lengths = [np.sum(np.stack(h["moved"]), axis=0) for h in host]
    print("A = %d: moves %s, moves with sitters %s, game lengths %s, means %s"
          % (players, [h["moves"] for h in host], sitters, [sorted(set(l.tolist())) for l in lengths], [h["mean"] for h in host]))
    assert all(s >= 1 for s in sitters) and all(len(set(l.tolist())) >= 2 for l in lengths)
    assert all(h["moves"] > 0 for h in host)
    for poll in (1, 4):
        monkeypatch.setenv("MAPPO_HANABI_EVAL_POLL", str(poll))
        envs = common.HostTablesWithDeviceContract(ec.eval_args(players, True, True), ec.EVAL_SEEDS)
        runner, got = ec.play_device(tmp_path / ("device%d" % poll), players, True, CPU, envs)
        assert runner.device_eval.graphs is None            # a CPU device: the eager loop
        ec.assert_same_evaluations(host, got, "host vs device eval (eager, CPU), P = %d" % poll)
        for h, g, length in zip(host, got, lengths):
            assert (g["games"] == 1).all() and (g["by_table"] >= 0).all()
            assert g["readbacks"] <= math.ceil(g["rounds"] / float(poll)) + 1
            assert g["rounds"] * players >= length.max()          # nothing stopped early
        assert envs.moves_with_sitters == sum(sitters)
        envs.close()


def test_feed_forward_policy_carries_no_state(host_buffer, tmp_path):
    envs = common.HostTablesWithDeviceContract(ec.eval_args(2, True), ec.EVAL_SEEDS)
    runner, got = ec.play_device(tmp_path / "ff", 2, False, CPU, envs, evaluations=1)
    host = ec.play_host(tmp_path / "host", 2, False, CPU, evaluations=1)
    ec.assert_same_evaluations(host, got, "feed-forward", rnn=False)
    assert not runner.device_eval.ops.recurrent and not got[0]["rnn"].any()
    envs.close()


def _fake_descriptor():
    return common.fake_descriptor(_native.HanabiEval, n_tables=7, players=3, avail_w=11, rnn_w=64)


def test_eval_entry_points_check_their_arguments_before_enqueueing():
    """NULL / SHAPE / ALIGN by return code (nothing reaches a device: every call below is refused)."""
    lib = _native.lib()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
    for fn, own, other in ((lib.mappo_hanabi_eval_begin, ("action", "can_move", "env_actions"), "flags"),
                           (lib.mappo_hanabi_eval_end, ("use_available_actions", "flags", "can_move", "moves", "games",
                                                        "scores", "refused"), "action")):
        assert fn(None, 0, None) == E_NULL
        for name in own + ("rnn_states", "rnn_new"):          # (one RNN pointer without the other)
            d = _fake_descriptor()
            setattr(d, name, None)
            assert fn(ctypes.byref(d), 0, None) == E_NULL, name
        for agent, players, n in ((-1, 3, 7), (3, 3, 7), (0, 6, 7), (0, 0, 7), (0, 3, 0), (5, 5, 7)):
            d = _fake_descriptor()
            d.players, d.n_tables = players, n
            assert fn(ctypes.byref(d), agent, None) == E_SHAPE, (agent, players, n)
        for field in ("avail_w", "rnn_w"):
            d = _fake_descriptor()
            setattr(d, field, 0)
            assert fn(ctypes.byref(d), 0, None) == E_SHAPE, field
        for name, off in (("use_available_actions", 4), ("rnn_states", 8), ("rnn_new", 4), ("can_move", 2), ("action", 4),
                          ("moves", 4), ("flags", 2), ("scores", 2)):
            d = _fake_descriptor()
            setattr(d, name, getattr(d, name) + off)
            assert fn(ctypes.byref(d), 0, None) == E_ALIGN, name
        # a NULL the OTHER entry point needs comes after this one's checks: the shape error is what is reported
        d = _fake_descriptor()
        setattr(d, other, None)
        d.players = 6
        assert fn(ctypes.byref(d), 0, None) == E_SHAPE
        # a feed-forward policy: both RNN pointers NULL, rnn_w ignored -- the next check (here: the shape) is what answers
        d = _fake_descriptor()
        d.rnn_states = d.rnn_new = None
        d.rnn_w, d.n_tables = 0, 0
        assert fn(ctypes.byref(d), 0, None) == E_SHAPE


def test_eval_descriptor_layout_matches_the_header():
    src, pointers = common.header_layout(_native.HanabiEval, "mappo_hanabi_eval")
    assert pointers == 11 and _native.HanabiEval.n_tables.offset == 8 * pointers
    assert _native.HanabiEval.rnn_w.offset == 8 * pointers + 8 + 2 * 4
    assert ctypes.sizeof(_native.HanabiEval) == 8 * pointers + 8 + 4 * 4        # three int32 and the padding to 8 bytes
    assert "K18" in src and "hanabi_runner_forward.py:229" in src


def test_flag_is_absent_by_default_and_its_refusals_fire(monkeypatch, tmp_path):
    from onpolicy.config import get_config
    from onpolicy.scripts.eval import eval_hanabi
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    for script in (train_hanabi_forward, eval_hanabi):
        plain = script.parse_args(common.ARGV, get_config())
        assert not hasattr(plain, "use_device_eval")
        given = script.parse_args(common.ARGV + ["--use_eval", "--use_device_eval"], get_config())
        assert given.use_device_eval is True
        rest = {k: v for k, v in vars(given).items() if k not in ("use_device_eval", "use_eval")}
        assert rest == {k: v for k, v in vars(plain).items() if k != "use_eval"}
    with pytest.raises(NotImplementedError, match="--use_eval"):
        train_hanabi_forward.main(common.ARGV + ["--use_device_eval"])
    with pytest.raises(NotImplementedError, match="--use_subproc_envs"):
        train_hanabi_forward.main(common.ARGV + ["--use_eval", "--use_device_eval", "--use_subproc_envs"])
    with pytest.raises(NotImplementedError, match="--use_subproc_envs"):
        eval_hanabi.main(common.ARGV + ["--use_eval", "--use_device_eval", "--use_subproc_envs", "--model_dir", str(tmp_path)])
    given = train_hanabi_forward.parse_args(common.ARGV + ["--use_eval", "--use_device_eval"], get_config())
    assert train_hanabi_forward.check_device_eval(given) is True
    with pytest.raises(NotImplementedError, match="GPU device"):
        train_hanabi_forward.check_device_eval(given, CPU)
    assert train_hanabi_forward.check_device_eval(train_hanabi_forward.parse_args(common.ARGV, get_config()), CPU) is False


def test_move_bound_follows_from_the_rules_and_stops_an_endless_evaluation(host_buffer, tmp_path, monkeypatch):
    """2 * cards + 2 * players + information tokens + colours; with ``eval_end`` made to forget every finished game the
    evaluation raises at that bound and names the tables -- after ceil(bound / A) rounds, not after a guessed number."""
    from onpolicy.envs.hanabi.batch import rules_for
    from onpolicy.runner.shared import hanabi_eval
    assert hanabi_eval.move_bound(rules_for("Hanabi-Full", 2)) == 2 * 50 + 4 + 8 + 5
    assert hanabi_eval.move_bound(rules_for("Hanabi-Small", 3)) == 2 * 20 + 6 + 3 + 2
    assert hanabi_eval.move_bound(rules_for("Hanabi-Very-Small", 5)) == 2 * 10 + 10 + 3 + 1
    real = hanabi_eval.eval_end

    def never_finished(o, agent, flags):
        real(o, agent, flags)
        o.games.zero_()
    monkeypatch.setattr(hanabi_eval, "eval_end", never_finished)
    monkeypatch.setenv("MAPPO_HANABI_EVAL_POLL", "4")
    envs = common.HostTablesWithDeviceContract(ec.eval_args(2, True), ec.EVAL_SEEDS)
    with pytest.raises(RuntimeError, match=r"tables \[0, 1, 2, 3, 4, 5, 6\] have not finished"):
        ec.play_device(tmp_path / "endless", 2, False, CPU, envs, evaluations=1)
    assert envs.step_calls == 2 * math.ceil((2 * 20 + 4 + 3 + 2) / 2.0)
    envs.close()
