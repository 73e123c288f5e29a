"""TEST INFRASTRUCTURE shared by tests/test_hanabi_eval_cpu.py and tests/test_gpu_hanabi_eval.py: a stub ``policy.act`` whose
outputs do not depend on the batch and whose RNN state is observable, a runner factory with eval envs, and the loop that plays
evaluations on either route.  Shapes, seeds and arguments are those of hanabi_turns_common.py."""
import numpy as np
import torch

from onpolicy.envs.hanabi import batch as hb

import hanabi_turns_common as common

N = common.N
EVAL_SEEDS = [5 + 10000 * i for i in range(N)]


class StubAct(object):
    """``policy.act``: action = the lowest legal move (0 for a row without one); new RNN state = old state + (action + 1),
    elementwise and exact in float32, so equal rows give equal bits whatever else is in the batch.  Takes the host loop's
    numpy slices and the device route's tensors; keeps every state it returned (``states``: one entry per call)."""

    def __init__(self, record=False):
        self.record, self.states = record, []           # (recording copies to the host: not inside a graph capture)

    def __call__(self, obs, rnn_states, masks, available_actions=None, deterministic=False):
        assert deterministic
        available_actions, rnn_states = torch.as_tensor(available_actions), torch.as_tensor(rnn_states)
        legal = available_actions > 0
        rows, moves = legal.shape
        lowest = (legal.to(torch.int64).cumsum(1) == 0).sum(1)          # illegal moves in front of the first legal one
        idx = torch.where(lowest < moves, lowest, torch.zeros_like(lowest))
        new = rnn_states + (idx + 1).to(torch.float32).view(rows, 1, 1)
        if self.record:
            self.states.append(new.detach().cpu().numpy().copy())
        return idx.view(rows, 1), new


def eval_args(players, device_eval, recurrent=False, **over):
    args = common.hanabi_args(players, use_eval=True, n_eval_rollout_threads=N, use_recurrent_policy=recurrent, **over)
    if device_eval:
        args.use_device_eval = True
    return args


def make_runner(args, envs, eval_envs, device, run_dir, stub=None):
    """``HanabiRunner`` with eval envs; ``stub``: a ``StubAct`` to put in the policy's place."""
    runner = common.make_runner(args, envs, device, run_dir, stub=False, eval_envs=eval_envs)
    if stub is not None:
        runner.trainer.policy.act = stub
    return runner


class CountingHostEnvs(object):
    """The host stepper as eval envs, recording which tables moved in every ``step`` (``moved``: bool [N] per call)."""

    def __init__(self, args, seeds):
        self.host = hb.HanabiBatchVecEnv(args, seeds, copy=False)
        self.moved = []

    def __getattr__(self, name):
        return getattr(self.host, name)

    def step(self, actions):
        self.moved.append(np.asarray(actions).reshape(N, -1)[:, 0] != -1)
        return self.host.step(actions)


def host_rnn_states(moved, states, players, shape):
    """What the host loop's local ``rnn_states`` held at the end of one evaluation: call k is player k % players' move on the
    tables ``moved[k]``, and ``states[k]`` what the policy returned for them."""
    out = np.zeros(shape, dtype=np.float32)
    for k, (m, s) in enumerate(zip(moved, states)):
        out[m, k % players] = s
    return out


def play_host(run_dir, players, recurrent, device, evaluations=2, stub=True, **over):
    """``evaluations`` x the untouched host ``_eval_games`` on ``HanabiBatchVecEnv`` -> one record per evaluation."""
    args = eval_args(players, False, recurrent, **over)
    envs, eval_envs = hb.HanabiBatchVecEnv(args, common.SEEDS, copy=False), CountingHostEnvs(args, EVAL_SEEDS)
    act = StubAct(record=True) if stub else None
    runner = make_runner(args, envs, eval_envs, device, run_dir, act)
    assert runner.device_eval is None
    out = []
    for _ in range(evaluations):
        k0 = len(eval_envs.moved)
        scores = np.asarray(runner._eval_games())
        moved = eval_envs.moved[k0:]
        rec = {"scores": np.sort(scores), "mean": float(np.mean(scores)), "moves": int(sum(m.sum() for m in moved)),
               "moved": moved}
        if stub:
            rec["rnn"] = host_rnn_states(moved, act.states[k0:], players, (N, players, args.recurrent_N, args.hidden_size))
        out.append(rec)
    envs.close()
    eval_envs.close()
    return out


def play_device(run_dir, players, recurrent, device, eval_envs, evaluations=2, stub=True, each=None, **over):
    """``evaluations`` x ``_eval_games`` with ``--use_device_eval`` on ``eval_envs`` -> (runner, one record per evaluation)."""
    args = eval_args(players, True, recurrent, **over)
    envs = hb.HanabiBatchVecEnv(args, common.SEEDS, copy=False)
    runner = make_runner(args, envs, eval_envs, device, run_dir, StubAct() if stub else None)
    route = runner.device_eval
    assert route is not None
    out = []
    for k in range(evaluations):
        if each is not None:
            each(runner, k)
        scores = runner._eval_games()
        assert isinstance(scores, np.ndarray) and scores.shape == (N,)
        c = route.counters
        out.append({"scores": np.sort(scores), "mean": float(np.mean(scores)), "moves": int(c["moves"].sum()),
                    "games": c["games"].copy(), "by_table": scores.copy(), "rnn": route.ops.rnn_states.cpu().numpy().copy(),
                    "rounds": route.rounds, "readbacks": route.readbacks})
    envs.close()
    return runner, out


def assert_same_evaluations(a, b, what, rnn=True):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["scores"], y["scores"]), (what, k, x["scores"], y["scores"])
        assert x["mean"] == y["mean"] and x["moves"] == y["moves"], (what, k)
        if rnn:
            assert np.array_equal(x["rnn"].view(np.int32), y["rnn"].view(np.int32)), "%s: RNN states of evaluation %d" % (what, k)
