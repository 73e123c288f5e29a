"""The host-free Hanabi route for RECURRENT policies (``--use_device_turns --use_device_turns_rnn``) without a GPU: struct
layout and argument checks of the two ``_rnn`` entry points of K17 (include/mappo_hip.h), the route's eager loop on CPU
tensors against the default route with a recurrent stub policy, and the train script's second flag."""
import ctypes

import numpy as np
import pytest
import torch

from onpolicy import _native
from onpolicy.envs.hanabi import batch as hb

import hanabi_turns_common as common
from hanabi_turns_common import host_buffer      # noqa: F401  (a fixture)
from hanabi_turns_rnn_common import recurrent_stub_get_actions

CPU = torch.device("cpu")
STATE_POINTERS = ("rnn_states", "rnn_states_critic", "rnn_new", "rnn_new_critic")


# ------------------------------------------------------------------------------------------- layout and argument checks
def test_rnn_descriptor_layout_matches_the_header():
    src, pointers = common.header_layout(_native.HanabiTurnRnn, "mappo_hanabi_turn_rnn")
    assert pointers == 29
    assert _native.HanabiTurnRnn.n_tables.offset == 232
    assert _native.HanabiTurnRnn.rnn_w.offset == 232 + 8 + 4 * 4
    assert ctypes.sizeof(_native.HanabiTurnRnn) == 264
    k17 = [name for name, kind in _native.HanabiTurn._fields_ if kind is ctypes.c_void_p]
    assert len(k17) == 25 and [name for name, _ in _native.HanabiTurnRnn._fields_[:25]] == k17
    assert [name for name, _ in _native.HanabiTurnRnn._fields_[25:29]] == list(STATE_POINTERS)
    # K17's own descriptor is as it was
    assert ctypes.sizeof(_native.HanabiTurn) == 8 * 25 + 8 + 4 * 4
    assert "int mappo_hanabi_turn_begin_rnn(const mappo_hanabi_turn_rnn_t* args, int agent, mappo_stream_t stream);" in src
    assert "int mappo_hanabi_turn_end_rnn(const mappo_hanabi_turn_rnn_t* args, int agent, mappo_stream_t stream);" in src


def _fake_descriptor():
    return common.fake_descriptor(_native.HanabiTurnRnn, n_tables=7, players=3, obs_w=13, share_w=21, avail_w=11, rnn_w=6)


def test_rnn_entry_points_check_their_arguments_before_enqueueing():
    """NULL / SHAPE / ALIGN by return code (nothing reaches a device: every call below is refused)."""
    lib = _native.lib()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
    begin_own = ("value", "action", "logp", "env_actions", "use_obs") + STATE_POINTERS
    end_own = ("flags", "rewards_env", "moves", "refused", "reset_choose", "rnn_states", "rnn_states_critic")
    for fn, own, others in ((lib.mappo_hanabi_turn_begin_rnn, begin_own, ("flags", "rewards_env", "moves")),
                            (lib.mappo_hanabi_turn_end_rnn, end_own, ("logp", "rnn_new", "rnn_new_critic"))):
        assert fn(None, 0, None) == E_NULL
        for name in own + ("obs", "share_obs", "can_move"):
            d = _fake_descriptor()
            setattr(d, name, None)
            assert fn(ctypes.byref(d), 0, None) == E_NULL, name
        for agent, players, n in ((-1, 3, 7), (3, 3, 7), (0, 6, 7), (0, 0, 7), (0, 3, 0), (5, 5, 7)):
            d = _fake_descriptor()
            d.players, d.n_tables = players, n
            assert fn(ctypes.byref(d), agent, None) == E_SHAPE, (agent, players, n)
        for name in ("rnn_w", "avail_w", "obs_w"):
            d = _fake_descriptor()
            setattr(d, name, 0)
            assert fn(ctypes.byref(d), 0, None) == E_SHAPE, name
        d = _fake_descriptor()
        d.rnn_w = -3
        assert fn(ctypes.byref(d), 0, None) == E_SHAPE
        for name, off in (("rnn_states", 4), ("rnn_states_critic", 4), ("rnn_new", 4), ("rnn_new_critic", 8), ("obs", 4),
                          ("use_available_actions", 4), ("can_move", 2)):
            d = _fake_descriptor()
            setattr(d, name, getattr(d, name) + off)
            assert fn(ctypes.byref(d), 0, None) == E_ALIGN, name
        # a NULL the OTHER entry point needs is accepted up to the next check: the shape error is what is reported
        for other in others:
            d = _fake_descriptor()
            setattr(d, other, None)
            d.players = 6
            assert fn(ctypes.byref(d), 0, None) == E_SHAPE, other
            d = _fake_descriptor()
            setattr(d, other, None)
            d.obs += 4
            assert fn(ctypes.byref(d), 0, None) == E_ALIGN, other
    d = _fake_descriptor()
    d.action += 4                           # int64: 8-byte aligned
    assert lib.mappo_hanabi_turn_begin_rnn(ctypes.byref(d), 0, None) == E_ALIGN
    d = _fake_descriptor()
    d.moves += 4
    assert lib.mappo_hanabi_turn_end_rnn(ctypes.byref(d), 0, None) == E_ALIGN
    assert lib.mappo_abi_version() == 2


# ------------------------------------------------------------------------------------------- the route on CPU tensors
def test_operands_check_the_state_tensors():
    """``TurnOperands(recurrent=True)``: the descriptor is a ``HanabiTurnRnn`` with both state tensors bound; a state
    tensor of another shape or a non-contiguous one is refused; ``state_tensors()`` lists both only when recurrent."""
    import types
    from onpolicy.runner.shared import hanabi_turns
    n, A, L, H = 5, 3, 2, 4
    turn = types.SimpleNamespace(rnn_states=torch.zeros(n, A, L, H), rnn_states_critic=torch.zeros(n, A, L, H))
    for name, w in zip(hanabi_turns.ROW_FIELDS, (6, 8, 3)):
        setattr(turn, name, torch.zeros(n, A, w))
    for name in hanabi_turns.SCALAR_FIELDS:
        setattr(turn, name, torch.zeros(n, A, 1))
    use = [torch.zeros(n, w) for w in (6, 8, 3)]
    plain = hanabi_turns.TurnOperands(turn, *use)
    assert isinstance(plain.descriptor(), _native.HanabiTurn) and not plain.recurrent
    assert not any(t is turn.rnn_states or t is turn.rnn_states_critic for t in plain.state_tensors())
    o = hanabi_turns.TurnOperands(turn, *use, recurrent=True)
    d = o.descriptor()
    assert isinstance(d, _native.HanabiTurnRnn) and d.rnn_w == L * H and d.n_tables == n and d.players == A
    assert d.rnn_states == turn.rnn_states.data_ptr() and d.rnn_states_critic == turn.rnn_states_critic.data_ptr()
    assert d.obs == turn.obs.data_ptr() and d.can_move == o.can_move.data_ptr() and d.moves == o.moves.data_ptr()
    listed = o.state_tensors()
    assert any(t is turn.rnn_states for t in listed) and any(t is turn.rnn_states_critic for t in listed)
    assert len(listed) == len(plain.state_tensors()) + 2
    turn.rnn_states_critic = torch.zeros(n, A, L, H + 1)
    with pytest.raises(ValueError, match="rnn_states_critic"):
        hanabi_turns.TurnOperands(turn, *use, recurrent=True).descriptor()
    turn.rnn_states_critic = torch.zeros(n, A, L, H)
    turn.rnn_states = torch.zeros(n, A, H, L).transpose(2, 3)
    with pytest.raises(ValueError, match="rnn_states"):
        hanabi_turns.TurnOperands(turn, *use, recurrent=True).descriptor()
    with pytest.raises(ValueError, match="new RNN states"):
        hanabi_turns.turn_begin(o, 0, torch.zeros(n, 1), torch.zeros(n, 1, dtype=torch.int64), torch.zeros(n, 1))


@pytest.mark.parametrize("players", [2, 3])
def test_recurrent_device_turns_route_equals_default_route_on_host_tables(host_buffer, tmp_path, players):
    """Hanabi-Small, N = 7, T = 8, a recurrent policy (the stub above): the default route on ``HanabiBatchVecEnv`` and the
    eager device-turns route on the same stepper behind the device env's contract -- every buffer field (both RNN state
    fields among them), the current rows and the counters bit-identical.  The run has finished games (all states of the
    table cleared) and moves with a table sitting out (its states kept), and the states it stores are not all zero."""
    args = common.hanabi_args(players, use_recurrent_policy=True)
    host_envs = hb.HanabiBatchVecEnv(args, common.SEEDS, copy=False)
    default = common.make_runner(args, host_envs, CPU, tmp_path / "default", stub=False)
    default.trainer.policy.get_actions = recurrent_stub_get_actions
    assert default.route.name == "host_tables"
    expected = common.play(default)
    assert expected[1]["games"] > 0 and expected[1]["moves"] > 0
    for k in ("rnn_states", "rnn_states_critic"):
        assert np.abs(expected[0][k]).max() > 0, k
        # a finished game shows as all-zero states of a table in a row that follows non-zero ones
        per_table = np.abs(expected[0][k]).reshape(expected[0][k].shape[0], common.N, -1).max(axis=2)
        assert ((per_table[1:] == 0) & (per_table[:-1] > 0)).any(), k
    assert not np.array_equal(expected[0]["rnn_states"], expected[0]["rnn_states_critic"])

    turn_args = common.hanabi_args(players, use_recurrent_policy=True)
    turn_args.use_device_turns = turn_args.use_device_turns_rnn = True
    envs = common.HostTablesWithDeviceContract(turn_args, common.SEEDS)
    turns = common.make_runner(turn_args, envs, CPU, tmp_path / "turns", stub=False)
    turns.trainer.policy.get_actions = recurrent_stub_get_actions
    assert turns.route.name == "device_turns"
    got = common.play(turns)
    assert turns.turn_graphs is None and turns.route.ops.recurrent            # a CPU device: the eager loop
    assert envs.step_calls == common.T * players
    print("A = %d: %d finished games, %d moves with sitters" % (players, got[1]["games"], envs.moves_with_sitters))
    assert envs.moves_with_sitters > 0 and got[1]["games"] > 0
    common.assert_same(expected, got, "recurrent device turns (eager, CPU) vs default route")
    host_envs.close()
    envs.close()


# ------------------------------------------------------------------------------------------- the flag
def test_rnn_flag_is_absent_by_default_and_needs_device_turns(monkeypatch, tmp_path):
    from onpolicy.config import get_config
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    plain = train_hanabi_forward.parse_args(common.ARGV, get_config())
    assert not hasattr(plain, "use_device_turns_rnn")
    flags = ("use_device_env", "use_device_turns", "use_device_turns_rnn")
    given = train_hanabi_forward.parse_args(common.ARGV + ["--" + f for f in flags], get_config())
    assert all(getattr(given, f) is True for f in flags)
    assert {k: v for k, v in vars(given).items() if k not in flags} == vars(plain)
    with pytest.raises(NotImplementedError, match="--use_device_turns"):
        train_hanabi_forward.main(common.ARGV + ["--use_device_turns_rnn"])
    with pytest.raises(NotImplementedError, match="--use_device_turns"):
        train_hanabi_forward.main(common.ARGV + ["--use_device_env", "--use_device_turns_rnn"])


@pytest.mark.parametrize("kind", ["use_recurrent_policy", "use_naive_recurrent_policy"])
def test_recurrent_policy_takes_the_route_with_both_flags(host_buffer, tmp_path, capsys, kind):
    def runner_of(tag, **flags):
        args = common.hanabi_args(2, **{kind: True})
        for k, v in flags.items():
            setattr(args, k, v)
        return common.make_runner(args, envs, CPU, tmp_path / tag, stub=False)
    envs = common.HostTablesWithDeviceContract(common.hanabi_args(2), common.SEEDS)
    capsys.readouterr()
    runner = runner_of("both", use_device_turns=True, use_device_turns_rnn=True)
    assert runner.route.name == "device_turns"
    assert not [l for l in capsys.readouterr().out.splitlines() if "device turns" in l]
    # the new flag alone asks for nothing: the default device route, no line
    assert runner_of("rnn_only", use_device_turns_rnn=True).route.name == "device_tables"
    assert not [l for l in capsys.readouterr().out.splitlines() if "device turns" in l]
    # without it: the existing sentence, verbatim
    runner = runner_of("turns_only", use_device_turns=True)
    assert runner.route.name == "device_tables"
    assert runner._device_turns_refusal() == "a recurrent policy carries per-table state through the moves"
    envs.close()


def test_host_sampler_rng_still_refuses_the_recurrent_route(host_buffer, tmp_path, capsys):
    from onpolicy.algorithms.utils import distributions
    args = common.hanabi_args(2, use_recurrent_policy=True, sampler_rng="host")
    args.use_device_turns = args.use_device_turns_rnn = True
    envs = common.HostTablesWithDeviceContract(args, common.SEEDS)
    capsys.readouterr()
    try:        # (the runner's constructor sets the sampler's generator, process-wide, from its arguments)
        runner = common.make_runner(args, envs, CPU, tmp_path / "host_rng", stub=False)
    finally:
        distributions.set_sampling_rng("device")
    lines = [l for l in capsys.readouterr().out.splitlines() if "device turns" in l]
    assert runner.route.name == "device_tables"
    assert lines == ["device turns: --sampler_rng host draws on the CPU generator; the rollout stays on the default device route"]
    envs.close()
