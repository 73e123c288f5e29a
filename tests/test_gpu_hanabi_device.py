"""-m gpu: Hanabi tables in device memory (K16: csrc/mappo_hanabi.hip, onpolicy/envs/hanabi/device.py) against the
reference engine's recorded games and against the host stepper (libhanabi_batch.so), bit for bit; then the turn-based
runner and the train script on them.  No test feeds illegal moves in bulk: the one refused move below is one call."""
import json
import os
import types

import numpy as np
import pytest
import torch

from onpolicy.envs.hanabi import batch as hb

import hanabi_turns_common as common

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RULE_KEYS = ("colors", "ranks", "players", "hand_size", "max_information_tokens", "max_life_tokens",
             "observation_type", "random_start_player")
# rule cases of the fixture that draw a random start player: the device stepper refuses such rules (that draw is a
# std::uniform_int_distribution, not reproducible across library versions), so these cannot be replayed on it.
# random_start4 is the case recorded for that switch; no_tokens3 (no information tokens, three ranks, two lives) was
# recorded with the switch on as well -- its rule set runs against the host stepper, switch off, in
# test_device_equals_host_stepper_under_random_play.
NEEDS_RANDOM_START = ("random_start4", "no_tokens3")


def _np(t):
    return t.cpu().numpy()


def _args(game, players, all_obs):
    return types.SimpleNamespace(hanabi_name=game, num_agents=int(players), use_obs_instead_of_state=bool(all_obs))


def test_device_tables_replay_the_reference_games(gold):
    """Every recorded game of the reference's HanabiEnv (``cases``) on one device table: rows, rewards, dones and scores
    equal, resets and the idle protocol included; then the rule sets outside the named games (``rule_cases``) in both
    share modes -- every player's view through "all players", the mover's own hand through "own hand"."""
    from onpolicy.envs.hanabi.device import HanabiDeviceBatch, HanabiDeviceVecEnv
    from onpolicy import _native
    z = gold.npz("hanabi_cases")
    cases = [c.split("|") for c in z["cases"]]
    assert len(cases) >= 12
    for name, game in cases:
        players, all_obs, seed, n_moves, obs_len, share_len = (int(v) for v in z[name + "_meta"])
        env = HanabiDeviceVecEnv(_args(game, players, all_obs), [seed], DEV)
        assert env.action_space[0].n == n_moves
        assert env.observation_space == [[obs_len + players]] * players
        assert env.share_observation_space == [[share_len + players]] * players
        exp = (z[name + "_obs"], z[name + "_share"], z[name + "_avail"])
        resets = set(int(t) for t in z[name + "_resets"])
        row = 0

        def check(got, what):
            for g, e, k in zip(got, exp, ("obs", "share_obs", "available")):
                g = _np(g)
                assert g.dtype == np.float32 and g.shape == (1,) + e[row].shape
                assert np.array_equal(g[0], e[row]), "%s: %s differs at %s" % (name, k, what)

        check(env.reset(np.array([True])), "the first reset")
        for t, a in enumerate(z[name + "_actions"]):
            obs, share, rewards, dones, infos, avail = env.step(np.array([[int(a)]]))
            row += 1
            check((obs, share, avail), "step %d" % t)
            assert np.array_equal(_np(rewards), np.full((1, players, 1), z[name + "_rewards"][t], dtype=np.float32))
            assert dones[0] is bool(z[name + "_dones"][t]) and infos[0] == {"score": int(z[name + "_scores"][t])}
            if dones[0]:
                assert t in resets
                row += 1
                check(env.reset(np.array([True])), "the reset after step %d" % t)
        assert row + 1 == len(exp[0])
        # idle protocol (Hanabi_Env.py:460-468, :307-311)
        obs, share, rewards, dones, infos, avail = env.step(np.array([[-1]]))
        assert dones[0] is None and not _np(obs).any() and not _np(share).any() and not _np(avail).any()
        assert not _np(rewards).any() and infos[0] == {"score": int(z[name + "_idle_score"])}
        assert not any(_np(x).any() for x in env.reset(np.array([False])))
        env.close()

    replayed = 0
    for name in z["rule_cases"]:
        k = "rules_%s_" % name
        config = [int(v) for v in z[k + "config"]]
        rules, seed = dict(zip(RULE_KEYS, config[:8])), config[8]
        if rules["random_start_player"]:
            assert str(name) in NEEDS_RANDOM_START
            assert _native.lib().mappo_hanabi_state_bytes(*config[:8]) == -2
            with pytest.raises(ValueError, match="random_start_player"):
                HanabiDeviceBatch(rules, [seed], device=DEV)
            continue
        assert str(name) not in NEEDS_RANDOM_START
        own_mode = HanabiDeviceBatch(rules, [seed], hb.SHARE_OWN_HAND, DEV)
        all_mode = HanabiDeviceBatch(rules, [seed], hb.SHARE_ALL_PLAYERS, DEV)
        n_moves, obs_len, own_len, hand = (int(v) for v in z[k + "dims"])
        for b in (own_mode, all_mode):
            assert (b.num_moves, b.obs_len, b.own_hand_len) == (n_moves, obs_len, own_len)
        P = own_mode.players
        views, own, legal, to_move = z[k + "views"], z[k + "own"], z[k + "legal"], z[k + "to_move"]
        resets = set(int(t) for t in z[k + "resets"])
        row = 0

        def check(what):
            cur = int(to_move[row])
            turn = np.eye(P, dtype=np.float32)[cur]
            for b in (own_mode, all_mode):
                assert int(b.to_move[0]) == cur, "%s: player to move at %s" % (name, what)
                assert np.array_equal(_np(b.available_actions)[0], legal[row]), "%s: legal moves at %s" % (name, what)
                assert np.array_equal(_np(b.obs)[0], np.concatenate([views[row, cur], turn])), (name, what)
            share = _np(all_mode.share_obs)[0]
            for p in range(P):
                assert np.array_equal(share[p * obs_len:(p + 1) * obs_len], views[row, p]), \
                    "%s: view of player %d at %s" % (name, p, what)
            assert np.array_equal(share[P * obs_len:], turn)
            share = _np(own_mode.share_obs)[0]
            assert np.array_equal(share[:own_len], own[row, cur]), "%s: own hand at %s" % (name, what)
            assert np.array_equal(share[own_len:], np.concatenate([views[row, cur], turn]))

        for b in (own_mode, all_mode):
            b.reset()
        check("the first deal")
        for t, a in enumerate(z[k + "actions"]):
            for b in (own_mode, all_mode):
                b.step([int(a)])
            row += 1
            check("move %d" % t)
            for b in (own_mode, all_mode):
                assert int(b.scores[0]) == int(z[k + "scores"][t])
                assert bool(b.status[0]) == (int(z[k + "status"][t]) != 0)
            if t in resets:
                for b in (own_mode, all_mode):
                    assert int(b.status[0]) == 1
                    b.reset()
                row += 1
                check("the deal after move %d" % t)
        assert row + 1 == len(views)
        replayed += 1
    assert replayed == len(z["rule_cases"]) - len(NEEDS_RANDOM_START) >= 3


NO_TOKENS3 = dict(colors=2, ranks=3, players=3, hand_size=2, max_information_tokens=0, max_life_tokens=2,
                  observation_type=1, random_start_player=0)
PLAY_RULES = [("full2", hb.rules_for("Hanabi-Full", 2)), ("full5", hb.rules_for("Hanabi-Full", 5)),
              ("small2", hb.rules_for("Hanabi-Small", 2)), ("verysmall2", hb.rules_for("Hanabi-Very-Small", 2)),
              ("no_tokens3", NO_TOKENS3)]


@pytest.mark.parametrize("share_mode", [hb.SHARE_OWN_HAND, hb.SHARE_ALL_PLAYERS], ids=["own_hand", "all_players"])
@pytest.mark.parametrize("rules", [r for _, r in PLAY_RULES], ids=[n for n, _ in PLAY_RULES])
def test_device_equals_host_stepper_under_random_play(rules, share_mode):
    """193 tables (three 64-thread workgroups of the per-table kernels and a tail) beside the host HanabiBatch with the same
    seeds: uniformly random legal moves drawn on the host, every 7th table sitting the move out, finished tables reset
    selectively -- every output array equal after every call, until some table's generator has produced more than
    1,248 words (twice through its 624 words).  Then ONE out-of-range uid on one table: ValueError naming it, and that
    table unchanged."""
    from onpolicy.envs.hanabi.device import HanabiDeviceBatch
    n = 193
    seeds = [7 + 1000 * i for i in range(n)]
    seeds[3], seeds[4] = -5, (1 << 32) + 11                 # seeds wrap modulo 2^32, as std::mt19937's do
    host, dev = hb.HanabiBatch(rules, seeds, share_mode), HanabiDeviceBatch(rules, seeds, share_mode, DEV)
    assert (host.players, host.num_moves, host.obs_len, host.own_hand_len, host.share_len) == \
        (dev.players, dev.num_moves, dev.obs_len, dev.own_hand_len, dev.share_len)
    rng = np.random.default_rng(11)

    def same_rows(what):
        for k in ("obs", "share_obs", "available_actions", "to_move"):
            g, e = _np(getattr(dev, k)), getattr(host, k)
            assert g.dtype == e.dtype and g.shape == e.shape
            assert np.array_equal(g, e), "%s differs after %s" % (k, what)

    # never reset: encode gives zero rows on the device (the host call refuses)
    dev.encode()
    assert not _np(dev.obs).any() and not _np(dev.share_obs).any() and (_np(dev.to_move) == -1).all()
    first = np.arange(n) % 3 != 1                          # a selective first deal, the rest next
    for choose in (first, ~first):
        host.reset(choose)
        host.encode(choose)
        flags = dev.reset(choose)
        same_rows("reset")
        assert np.array_equal((flags & 0xff) == 0, choose) and np.array_equal((flags & 0xff) == 2, ~choose)
        assert np.array_equal((flags >> 8) & 1, host.available_actions.any(axis=1))
    assert (dev.draws() <= 2 * host.players * 5).all()

    calls, finished, limit = 0, 0, 4000
    while dev.draws().max() <= 1248:
        assert calls < limit, "no table reached two passes over its generator within %d calls" % limit
        host.encode()                                      # the legal moves of every table, to choose from
        if calls % 16 == 0:
            dev.encode()
            same_rows("encode of all tables")
        legal = host.available_actions
        assert legal.any(axis=1).all()
        moves = (legal * (rng.random(legal.shape) + 1e-3)).argmax(axis=1).astype(np.int32)   # uniform over the legal uids
        moves[(np.arange(n) + calls) % 7 == 0] = -1
        host.step(moves)
        host.encode(moves != -1)
        flags = dev.step(torch.from_numpy(moves).to(DEV) if calls % 2 else moves)
        calls += 1
        same_rows("step %d" % calls)
        for k in ("rewards", "status", "scores"):
            g, e = _np(getattr(dev, k)), getattr(host, k)
            assert g.dtype == e.dtype and np.array_equal(g, e), "%s differs after step %d" % (k, calls)
        assert np.array_equal(flags & 0xff, host.status) and np.array_equal(flags >> 16, host.scores)
        assert np.array_equal((flags >> 8) & 1, host.available_actions.any(axis=1))
        done = host.status == 1
        finished += int(done.sum())
        if done.any():
            host.reset(done)
            host.encode(done)
            dev.reset(done)
            same_rows("reset after step %d" % calls)
    assert finished >= 20

    # one refused move: table 5 gets a uid out of range, everybody else sits out
    dev.encode()
    before = [_np(getattr(dev, k)).copy() for k in ("obs", "share_obs", "available_actions", "to_move")], dev.draws()
    moves = np.full(n, -1, dtype=np.int32)
    moves[5] = dev.num_moves
    with pytest.raises(ValueError, match="table 5 "):
        dev.step(moves)
    assert int(dev.status[5]) == 255 and float(dev.rewards[5]) == 0.0 and not _np(dev.obs)[5].any()
    dev.encode()
    after = [_np(getattr(dev, k)) for k in ("obs", "share_obs", "available_actions", "to_move")], dev.draws()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    host.close()


def _rollout(tmp_path, tag, on_device, all_obs):
    from onpolicy.envs.hanabi.device import HanabiDeviceVecEnv
    args = common.hanabi_args(2, all_obs=all_obs)
    envs = HanabiDeviceVecEnv(args, common.SEEDS, DEV) if on_device else hb.HanabiBatchVecEnv(args, common.SEEDS, copy=False)
    runner = common.make_runner(args, envs, DEV, tmp_path / tag, stub=False)
    scores = []
    collect = runner.collect

    def collect_and_keep(step):                             # run() starts a fresh score list every episode
        collect(step)
        if step == common.T - 1:
            scores.append(list(runner.scores))
    runner.collect = collect_and_keep
    runner.run()
    torch.cuda.synchronize()
    out = {k: _np(getattr(runner.buffer, k)) for k in common.BUFFER_FIELDS}
    out["params"] = _np(torch.cat([p.detach().reshape(-1) for p in runner.policy.actor.parameters()] +
                                  [p.detach().reshape(-1) for p in runner.policy.critic.parameters()]))
    out["use_rows"] = np.concatenate([_np(t).reshape(-1) for t in (runner.use_obs, runner.use_share_obs,
                                                                  runner.use_available_actions)])
    logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    envs.close()
    return out, scores, runner.true_total_num_steps, [sorted(r.items()) for r in logged if "score" in r["tag"]]


@pytest.mark.parametrize("all_obs", [False, True], ids=["state", "obs_instead_of_state"])
def test_device_rollout_equals_host_rollout(tmp_path, all_obs):
    """HanabiRunner over two episodes, the update between them included, on host tables and on device tables with the same
    seeds: every buffer field, the parameters, the runner's current rows and the score lists are bit-identical (the
    policy samples on the device both times, so equal rows give equal actions).  Covers the reset that must not write
    into the rows the runner still reads: restarted games are merged in, the other tables keep their step rows."""
    host, host_scores, host_steps, host_logged = _rollout(tmp_path, "host", False, all_obs)
    dev, dev_scores, dev_steps, dev_logged = _rollout(tmp_path, "device", True, all_obs)
    assert host_steps == dev_steps > 0
    assert host_scores == dev_scores and len(host_scores) == 2 and sum(len(s) for s in host_scores) > 0
    assert host_logged == dev_logged
    for k in sorted(host):
        assert host[k].shape == dev[k].shape and np.array_equal(host[k], dev[k]), k
    assert host["rewards"].any() or host["masks"].min() == 0.0     # games were played and finished


def test_train_script_with_device_tables(tmp_path, monkeypatch):
    """train_hanabi_forward --use_device_env end to end: training tables on the device, evaluation on the host stepper,
    the same logged scores and parameters as the default layout; the flag refuses --use_subproc_envs."""
    from onpolicy.scripts.train import train_hanabi_forward
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    argv = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Small", "--num_agents", "2", "--algorithm_name", "mappo",
            "--n_rollout_threads", "7", "--episode_length", "8", "--num_env_steps", str(3 * 7 * 8), "--ppo_epoch", "2",
            "--hidden_size", "64", "--use_wandb", "--log_interval", "1", "--n_training_threads", "1", "--use_eval",
            "--n_eval_rollout_threads", "2", "--eval_interval", "2", "--seed", "3"]
    runs = []
    for extra in (["--use_device_env"], []):
        runner = train_hanabi_forward.main(argv + extra)
        assert type(runner.envs).__name__ == ("HanabiDeviceVecEnv" if extra else "HanabiBatchVecEnv")
        assert type(runner.eval_envs).__name__ == "HanabiBatchVecEnv"
        assert runner.true_total_num_steps > 0
        logged = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
        assert {"value_loss", "average_score", "eval_average_score"} <= {r["tag"] for r in logged}
        params = torch.cat([p.detach().reshape(-1) for p in runner.policy.actor.parameters()]).cpu()
        runs.append(([sorted(r.items()) for r in logged if "score" in r["tag"]], params, runner.true_total_num_steps))
        runner.envs.close()
        runner.eval_envs.close()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] and torch.equal(runs[0][1], runs[1][1])
    with pytest.raises(NotImplementedError, match="use_subproc_envs"):
        train_hanabi_forward.main(argv + ["--use_device_env", "--use_subproc_envs"])
