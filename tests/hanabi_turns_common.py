"""TEST INFRASTRUCTURE shared by the Hanabi runner tests (tests/test_hanabi_{turns,eval}_cpu.py, tests/test_gpu_hanabi_*.py):
the stub policy whose outputs do not depend on the batch, the adapter that gives the host stepper the device env's host-free
contract, the loop that drives ``HanabiRunner`` like ``run()`` does between two updates, and what the K17 / K18 tests share:
fake descriptors, the header-struct parser, bitwise comparison, the grid cap, allocations with canaries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from host_buffer import HostSharedBuffer
from onpolicy import _native
from onpolicy.envs.hanabi import batch as hb

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mappo_hip.h")
CAP_TABLES = _native.TURN_MAX_BLOCKS * 4        # K17 / K18: one wave per table, four waves a workgroup
BUFFER_FIELDS = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "actions",
                 "action_log_probs", "rewards", "masks", "bad_masks", "active_masks", "available_actions")
T, N = 8, 7
SEEDS = [3 + 1000 * i for i in range(N)]
ARGV = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Small", "--num_agents", "2", "--algorithm_name", "mappo",
        "--n_rollout_threads", "7", "--episode_length", "8", "--num_env_steps", "112", "--use_wandb"]      # (the scripts)


@pytest.fixture
def host_buffer(monkeypatch):
    """Runners on a CPU device: the rollout buffer on host tensors."""
    import onpolicy.runner.shared.base_runner as base
    monkeypatch.setattr(base, "SharedReplayBuffer", HostSharedBuffer)


def stub_get_actions(cent_obs, obs, rnn_states_actor, rnn_states_critic, masks, available_actions=None,
                     deterministic=False):
    """action = the lowest legal move (0 for a row without one); value and log-prob are elementwise functions of that
    index and of single observation entries: equal rows give equal bits whatever else is in the batch."""
    legal = available_actions > 0
    rows, moves = legal.shape
    lowest = (legal.to(torch.int64).cumsum(1) == 0).sum(1)          # illegal moves in front of the first legal one
    idx = torch.where(lowest < moves, lowest, torch.zeros_like(lowest))
    f = idx.to(torch.float32).view(rows, 1)
    value = f * 0.125 + obs[:, 1:2] * 0.5 - cent_obs[:, 0:1] * 0.25
    logp = -(f + 1.0) * 0.0625 - obs[:, 2:3] * 0.5
    return value, idx.view(rows, 1), logp, rnn_states_actor, rnn_states_critic


class HostTablesWithDeviceContract(object):
    """``HanabiBatchVecEnv`` (the host stepper) behind the host-free contract of ``HanabiDeviceVecEnv``: rows as tensors
    that every call rewrites in place, a flags word built from status, legal-moves-any and score, ``step_device`` on an
    int32 action tensor, ``reset_device`` on a mask.  CPU tensors: what lets the route's logic run without a GPU."""

    device_resident = True

    def __init__(self, all_args, seeds):
        self.host = hb.HanabiBatchVecEnv(all_args, seeds, copy=False)
        b = self.host.batch
        self.num_envs, self.players = b.n, b.players
        self.action_space, self.observation_space = self.host.action_space, self.host.observation_space
        self.share_observation_space = self.host.share_observation_space
        rows = lambda: (torch.zeros(b.n, b.obs.shape[1]), torch.zeros(b.n, b.share_obs.shape[1]),       # noqa: E731
                        torch.zeros(b.n, b.num_moves), torch.full((b.n,), 2, dtype=torch.int32))
        self.step_obs, self.step_share_obs, self.step_available_actions, self.step_flags = rows()
        self._reset_rows = rows()
        self.step_rewards = torch.zeros(b.n)
        self.moves_with_sitters, self.step_calls = 0, 0

    def _fill(self, out, status):
        b = self.host.batch
        for dst, src in zip(out[:3], (b.obs, b.share_obs, b.available_actions)):
            dst.copy_(torch.from_numpy(src))
        flags = status.astype(np.int32) | (b.available_actions.any(axis=1).astype(np.int32) << 8) | \
            (b.scores.astype(np.int32) << 16)
        out[3].copy_(torch.from_numpy(flags))

    def step_device(self, env_actions):
        assert env_actions.dtype == torch.int32 and env_actions.shape == (self.num_envs,)
        b = self.host.batch
        a = env_actions.numpy().copy()
        self.step_calls += 1
        self.moves_with_sitters += int((a == -1).any() and (a != -1).any())
        b.step(a)
        b.encode(a != -1)
        self._fill((self.step_obs, self.step_share_obs, self.step_available_actions, self.step_flags), b.status)
        self.step_rewards.copy_(torch.from_numpy(b.rewards))

    def reset_device(self, mask):
        assert mask.dtype == torch.uint8 and mask.shape == (self.num_envs,)
        b = self.host.batch
        choose = mask.numpy().astype(bool)
        b.reset(choose)
        b.encode(choose)
        self._fill(self._reset_rows, np.where(choose, 0, 2))
        return self._reset_rows

    def close(self):
        self.host.close()


def hanabi_args(players, hidden=64, layer_N=1, all_obs=False, episodes=2, **over):
    from helpers import make_args
    args = make_args(env_name="Hanabi", episode_length=T, n_rollout_threads=N, num_env_steps=episodes * T * N,
                     hidden_size=hidden, layer_N=layer_N, ppo_epoch=2, num_mini_batch=1, algorithm_name="mappo",
                     log_interval=1, use_wandb=False, use_obs_instead_of_state=all_obs, **over)
    args.hanabi_name, args.num_agents = "Hanabi-Small", players
    return args


def make_runner(args, envs, device, run_dir, stub=True, eval_envs=None):
    from onpolicy.runner.shared.hanabi_runner_forward import HanabiRunner
    torch.manual_seed(1)
    np.random.seed(1)
    run_dir.mkdir()
    runner = HanabiRunner({"all_args": args, "envs": envs, "eval_envs": eval_envs, "num_agents": args.num_agents,
                           "device": device, "run_dir": run_dir})
    if stub:
        runner.trainer.policy.get_actions = stub_get_actions
    return runner


def play(runner, steps=T, each_step=None):
    """``begin_rollout`` then ``steps`` x (collect, insert, restart), as ``run()`` does between two updates.
    -> {buffer fields, current rows, counters} as numpy / Python values."""
    runner.begin_rollout()
    for step in range(steps):
        runner.collect(step)
        if each_step is not None:
            each_step(step)
        runner.insert_and_restart()
    return outcome(runner)


def outcome(runner):
    np_ = lambda t: t.detach().cpu().numpy()       # noqa: E731
    out = {k: np_(getattr(runner.buffer, k)).copy() for k in BUFFER_FIELDS}
    out["use_rows"] = np.concatenate([np_(t).reshape(-1) for t in (runner.use_obs, runner.use_share_obs,
                                                                  runner.use_available_actions)])
    c = runner.route.score_summary()
    return out, {"moves": runner.true_total_num_steps, "games": c["games"], "mean_score": float(c["average_score"])}


def recorded(gold, players):
    """The host-tables route as commit 184a686 played it (tools/make_golden_hanabi_routes.py), in ``outcome``'s form: the
    anchor that shares no code with the routes."""
    z, key = gold.npz("hanabi_route_cases"), "a%d_" % players
    fields = {k: z[key + k] for k in BUFFER_FIELDS + ("use_rows",)}
    return fields, {"moves": int(z[key + "moves"]), "games": int(z[key + "games"]), "mean_score": float(z[key + "mean_score"])}


def fake_descriptor(struct_cls, **ints):
    """A ``struct_cls`` of onpolicy._native: every pointer a distinct, never dereferenced, 16-byte aligned address; ``ints`` set."""
    d = struct_cls()
    for i, (name, kind) in enumerate(struct_cls._fields_):
        if kind is ctypes.c_void_p:
            setattr(d, name, 0x10000 + 0x100 * i)
    for name, value in ints.items():
        setattr(d, name, value)
    return d


def header_layout(struct_cls, c_name):
    """``struct_cls`` against ``typedef struct <c_name> { ... } <c_name>_t;`` of include/mappo_hip.h: the same fields in the
    same order, pointer for pointer and integer for integer.  -> (the header's text, the number of pointers)."""
    src = open(HEADER).read()
    body = src[src.index("typedef struct %s {" % c_name):src.index("} %s_t;" % c_name)]
    declared = re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(\w+);", body, flags=re.M)
    assert [name for _, name in declared] == [name for name, _ in struct_cls._fields_]
    for (ctype, name), (_, kind) in zip(declared, struct_cls._fields_):
        want = ctypes.c_void_p if "*" in ctype else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[ctype.strip()]
        assert kind is want, name
    return src, sum(1 for _, kind in struct_cls._fields_ if kind is ctypes.c_void_p)


def same_bits(a, b, what):
    """Two dicts of tensors: the same dtypes, shapes and bits."""
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        if x.dtype.is_floating_point:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), "%s: %s differs" % (what, k)


def assert_same(a, b, what):
    (fa, ca), (fb, cb) = a, b
    assert ca == cb, (what, ca, cb)
    for k in sorted(fa):
        assert fa[k].shape == fb[k].shape and fa[k].dtype == fb[k].dtype, (what, k)
        assert np.array_equal(fa[k], fb[k], equal_nan=True), "%s: %s differs" % (what, k)


class Arena(object):
    """Tensors on ``device`` cut out of allocations with ``PAD`` canary elements on either side (NaN for floats, a bit
    pattern for integers)."""
    PAD = 64

    def __init__(self, device):
        self.device, self.whole = device, []

    def put(self, values):
        values = values.to(self.device)
        fill = float("nan") if values.dtype.is_floating_point else 0x5a
        whole = torch.full((values.numel() + 2 * self.PAD,), fill, dtype=values.dtype, device=self.device)
        inner = whole[self.PAD:self.PAD + values.numel()]
        inner.copy_(values.reshape(-1))
        self.whole.append((whole, fill))
        assert inner.data_ptr() % 16 == 0
        return inner.view(values.shape)

    def canaries_intact(self):
        edges = [(edge, fill) for whole, fill in self.whole for edge in (whole[:self.PAD], whole[-self.PAD:])]
        return all(bool((torch.isnan(e) if e.dtype.is_floating_point else e == fill).all()) for e, fill in edges)
