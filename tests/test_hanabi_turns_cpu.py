"""The host-free Hanabi route ("device turns": runner/shared/hanabi_turns.py, hanabi_runner_forward.py) without a GPU: its
eager loop on CPU tensors against the default route on the same host stepper, the argument checks and struct layout of
K17's C ABI (include/mappo_hip.h), and the train script's flag."""
import ctypes

import numpy as np
import pytest
import torch

from onpolicy import _native
from onpolicy.envs.hanabi import batch as hb

import hanabi_turns_common as common
from hanabi_turns_common import host_buffer      # noqa: F401  (a fixture)

CPU = torch.device("cpu")


@pytest.mark.parametrize("players", [2, 3])
def test_device_turns_route_equals_default_route_on_host_tables(host_buffer, tmp_path, gold, players):
    """Hanabi-Small, N = 7, T = 8: the default route on ``HanabiBatchVecEnv`` and the eager device-turns route on the same
    stepper behind the device env's contract, both with the stub policy (lowest legal move): every buffer field, the
    current rows, the move count, the number of finished games and the mean score are bit-identical.  The stub loses its
    one life quickly, so the ground is covered -- asserted below; on the host stepper with these seeds: A = 2: 52 finished
    games, 6 moves with a table sitting out, 2 buffer steps in which every table had finished before the last player's
    move; A = 3: 55 / 10 / 5.  Both outcomes also equal, bit for bit, the recording of the host-tables route made before the
    routes came to share their bookkeeping (tests/golden/hanabi_route_cases.npz)."""
    args = common.hanabi_args(players)
    host_envs = hb.HanabiBatchVecEnv(args, common.SEEDS, copy=False)
    step, seen = host_envs.step, {"sitters": 0, "calls": 0}

    def counting_step(actions):
        a = np.asarray(actions).reshape(common.N, -1)[:, 0]
        seen["sitters"] += int((a == -1).any() and (a != -1).any())
        seen["calls"] += 1
        return step(actions)
    host_envs.step = counting_step
    default = common.make_runner(args, host_envs, CPU, tmp_path / "default")
    assert default.route.name == "host_tables"
    calls_per_step = []
    expected = common.play(default, each_step=lambda s: calls_per_step.append(seen["calls"]))
    all_out = sum(1 for a, b in zip([0] + calls_per_step, calls_per_step) if b - a < players)
    print("A = %d: %d finished games, %d moves with sitters, %d steps with all tables out"
          % (players, expected[1]["games"], seen["sitters"], all_out))
    assert expected[1]["games"] >= 20 and seen["sitters"] >= 3 and all_out >= 1
    assert expected[1]["moves"] > 0
    common.assert_same(common.recorded(gold, players), expected, "recorded host-tables route vs default route")

    turn_args = common.hanabi_args(players)
    turn_args.use_device_turns = True
    envs = common.HostTablesWithDeviceContract(turn_args, common.SEEDS)
    turns = common.make_runner(turn_args, envs, CPU, tmp_path / "turns")
    assert turns.route.name == "device_turns" and turns.turn_graphs is None
    got = common.play(turns)
    assert turns.turn_graphs is None            # a CPU device: the eager loop
    assert envs.step_calls == common.T * players and envs.moves_with_sitters == seen["sitters"]
    common.assert_same(expected, got, "device turns (eager, CPU) vs default route")
    common.assert_same(common.recorded(gold, players), got, "recorded host-tables route vs device turns (eager, CPU)")
    host_envs.close()
    envs.close()


def _fake_descriptor():
    return common.fake_descriptor(_native.HanabiTurn, n_tables=7, players=3, obs_w=13, share_w=21, avail_w=11)


def test_turn_entry_points_check_their_arguments_before_enqueueing():
    """NULL / SHAPE / ALIGN by return code (nothing reaches a device: every call below is refused)."""
    lib = _native.lib()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
    for fn, own, other in ((lib.mappo_hanabi_turn_begin, ("value", "action", "logp", "env_actions", "use_obs"), "flags"),
                           (lib.mappo_hanabi_turn_end, ("flags", "rewards_env", "moves", "refused", "reset_choose"), "logp")):
        assert fn(None, 0, None) == E_NULL
        for name in own + ("obs", "share_obs", "can_move"):
            d = _fake_descriptor()
            setattr(d, name, None)
            assert fn(ctypes.byref(d), 0, None) == E_NULL, name
        for agent, players, n in ((-1, 3, 7), (3, 3, 7), (0, 6, 7), (0, 0, 7), (0, 3, 0), (5, 5, 7)):
            d = _fake_descriptor()
            d.players, d.n_tables = players, n
            assert fn(ctypes.byref(d), agent, None) == E_SHAPE, (agent, players, n)
        d = _fake_descriptor()
        d.avail_w = 0
        assert fn(ctypes.byref(d), 0, None) == E_SHAPE
        for name, off in (("obs", 4), ("share_obs", 8), ("use_available_actions", 4), ("can_move", 2)):
            d = _fake_descriptor()
            setattr(d, name, getattr(d, name) + off)
            assert fn(ctypes.byref(d), 0, None) == E_ALIGN, name
        # a NULL the OTHER entry point needs comes after this one's checks: the shape error is what is reported
        d = _fake_descriptor()
        setattr(d, other, None)
        d.players = 6
        assert fn(ctypes.byref(d), 0, None) == E_SHAPE
    d = _fake_descriptor()
    d.action += 4                           # int64: 8-byte aligned
    assert lib.mappo_hanabi_turn_begin(ctypes.byref(d), 0, None) == E_ALIGN
    d = _fake_descriptor()
    d.moves += 4
    assert lib.mappo_hanabi_turn_end(ctypes.byref(d), 0, None) == E_ALIGN
    assert lib.mappo_abi_version() == 2


def test_turn_descriptor_layout_matches_the_header():
    src, pointers = common.header_layout(_native.HanabiTurn, "mappo_hanabi_turn")
    assert pointers == 25 and _native.HanabiTurn.n_tables.offset == 8 * pointers
    assert ctypes.sizeof(_native.HanabiTurn) == 8 * pointers + 8 + 4 * 4
    assert "#define MAPPO_TURN_MAX_BLOCKS %d\n" % _native.TURN_MAX_BLOCKS in src
    assert "#define MAPPO_TURN_MAX_PLAYERS %d\n" % _native.TURN_MAX_PLAYERS in src


def test_flag_is_absent_by_default_and_needs_device_tables(monkeypatch, tmp_path):
    from onpolicy.config import get_config
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    plain = train_hanabi_forward.parse_args(common.ARGV, get_config())
    assert not hasattr(plain, "use_device_turns") and not hasattr(plain, "use_device_env")
    given = train_hanabi_forward.parse_args(common.ARGV + ["--use_device_env", "--use_device_turns"], get_config())
    assert given.use_device_turns is True and given.use_device_env is True
    rest = {k: v for k, v in vars(given).items() if k not in ("use_device_turns", "use_device_env")}
    assert rest == vars(plain)
    with pytest.raises(NotImplementedError, match="--use_device_env"):
        train_hanabi_forward.main(common.ARGV + ["--use_device_turns"])


def test_recurrent_policy_stays_on_the_default_device_route(host_buffer, tmp_path, capsys):
    args = common.hanabi_args(2)
    args.use_device_turns = True
    args.use_recurrent_policy = True
    envs = common.HostTablesWithDeviceContract(args, common.SEEDS)
    capsys.readouterr()
    runner = common.make_runner(args, envs, CPU, tmp_path / "rnn", stub=False)
    lines = [l for l in capsys.readouterr().out.splitlines() if "device turns" in l]
    assert len(lines) == 1 and "recurrent" in lines[0] and "default device route" in lines[0]
    assert runner.route.name == "device_tables"
    # ... and the flag with a feed-forward policy takes the route
    args = common.hanabi_args(2)
    args.use_device_turns = True
    assert common.make_runner(args, envs, CPU, tmp_path / "mlp").route.name == "device_turns"
    envs.close()
