"""Hanabi tables in device memory (K16 of libmappo_hip.so, include/mappo_hip.h) and the vectorised env built on them.

``HanabiDeviceBatch`` mirrors ``batch.HanabiBatch`` -- same fields, same methods, same results bit for bit (both run
csrc/hanabi_rules.h) -- but its tables, and the tensors the kernels fill, live on the policy's device: a move is two
launches (apply + deal by one thread per table, encode by one workgroup per table) and the rows never cross PCIe.
``HanabiDeviceVecEnv`` gives them the ``reset(reset_choose)`` / ``step(actions)`` contract of ``HanabiBatchVecEnv``.

What still crosses to the host is one int32 *flags word* per table and move (status | can-move << 8 | score << 16,
``flag_*`` below): the turn-based runner decides on the host who moves and which games restart.  Its opt-in "device
turns" route reads those words on the device instead (K17, runner/shared/hanabi_turns.py) and drives the tables through
``HanabiDeviceVecEnv.step_device`` / ``reset_device``, which launch and read nothing back.

One difference to the host stepper: ``hanabi_batch_step`` validates every move before it applies any, so an illegal move
leaves ALL tables untouched.  The device step leaves only the offending table untouched (status 255); by the time the
flags are read back and ``ValueError`` is raised the other tables have advanced.
"""
import ctypes

import numpy as np
import torch

from onpolicy import _native
from onpolicy.envs.hanabi.batch import (SHARE_ALL_PLAYERS, SHARE_OWN_HAND, Rules, _DONE_OF_STATUS, _ScoreInfos,
                                         rules_for)
from onpolicy.envs.spaces import Discrete

STATUS_RUNNING, STATUS_FINISHED, STATUS_IDLE, STATUS_REFUSED = 0, 1, 2, 255
REFUSED_MOVE = ("mappo_hanabi_step: illegal move on table %d (or the table was never reset); that table is unchanged, the "
                "other tables have advanced")


def flag_status(flags):
    return flags & 0xff


def flag_can_move(flags):
    return (flags >> 8) & 1


def flag_score(flags):
    return flags >> 16


class _Rows(object):
    """One set of tensors an encode writes: the three row arrays, the player to move and the flags words."""

    def __init__(self, n, obs_w, share_w, moves, device):
        z = lambda w: torch.zeros((n, w), dtype=torch.float32, device=device)
        self.obs, self.share_obs, self.available_actions = z(obs_w), z(share_w), z(moves)
        self.to_move = torch.full((n,), -1, dtype=torch.int32, device=device)
        self.flags = torch.full((n,), STATUS_IDLE, dtype=torch.int32, device=device)


class HanabiDeviceBatch(object):
    """N tables under one set of rules in device memory; every tensor below is written in place by the kernels."""

    def __init__(self, rules, seeds, share_mode=SHARE_OWN_HAND, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("HanabiDeviceBatch needs a GPU device (the host stepper is batch.HanabiBatch)")
        self._lib = _native.lib()
        r = Rules(**rules)
        self._rules = tuple(int(getattr(r, name)) for name, _ in Rules._fields_)
        per_table = self._lib.mappo_hanabi_state_bytes(*self._rules)
        if per_table <= 0:
            raise ValueError("invalid Hanabi rules %r for the device stepper (random_start_player is host-only)" % (rules,))
        dims = (ctypes.c_int32 * 5)()
        _native.check(self._lib.mappo_hanabi_dims(*(self._rules + (ctypes.addressof(dims),))), "mappo_hanabi_dims")
        self.players, self.num_moves, self.obs_len, self.own_hand_len = (int(v) for v in dims[:4])
        # std::mt19937 takes the seed modulo 2^32: wider Python ints wrap the same way
        seeds = (np.asarray(seeds, dtype=np.int64).reshape(-1) % (1 << 32)).astype(np.uint32).view(np.int32)
        self.n = len(seeds)
        self.share_mode = share_mode
        self.share_len = self.own_hand_len + self.obs_len if share_mode == SHARE_OWN_HAND else self.players * self.obs_len
        with torch.cuda.device(self.device):
            self._state = torch.zeros((self.n * per_table + 3) // 4, dtype=torch.int32, device=self.device)
            self.rows = self.new_rows()
            self.rewards = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            self.status = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            self.scores = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            self._draws = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            self._flags_pinned = torch.zeros(self.n, dtype=torch.int32, pin_memory=True)
            self.flags_host = self._flags_pinned.numpy()          # page-locked; rewritten by every readback
            seeds_d = torch.from_numpy(np.ascontiguousarray(seeds)).to(self.device)
            _native.check(self._lib.mappo_hanabi_seed(self._state.data_ptr(), seeds_d.data_ptr(), self.n, self._stream()),
                          "mappo_hanabi_seed")
            torch.cuda.current_stream(self.device).synchronize()   # seeds_d may go

    # the fields of HanabiBatch: the rows most callers want are those of the batch's own set
    obs = property(lambda self: self.rows.obs)
    share_obs = property(lambda self: self.rows.share_obs)
    available_actions = property(lambda self: self.rows.available_actions)
    to_move = property(lambda self: self.rows.to_move)

    def new_rows(self):
        """A further set of output tensors (``reset(into=...)``): a caller that still reads what ``step`` handed out
        lets ``reset`` -- which zeroes the rows of every table it does not restart -- write somewhere else."""
        return _Rows(self.n, self.obs_len + self.players, self.share_len + self.players, self.num_moves, self.device)

    def _stream(self):
        return _native.stream_of(self.device)

    def _mask(self, m):
        if m is None:
            return torch.ones(self.n, dtype=torch.uint8, device=self.device)
        if not torch.is_tensor(m):
            m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8))
        return m.to(device=self.device, dtype=torch.uint8).reshape(self.n).contiguous()

    def read_flags(self, rows=None):
        """The flags words of ``rows`` -> the page-locked host array (one small copy, then a wait for the stream)."""
        self._flags_pinned.copy_((rows or self.rows).flags, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.flags_host

    def reset(self, choose=None, into=None, readback=True):
        """New game on the chosen tables (None: all) and their rows; zero rows, to_move -1 for the others."""
        rows, mask = into or self.rows, self._mask(choose)
        with torch.cuda.device(self.device):
            _native.check(self._lib.mappo_hanabi_reset(
                self._state.data_ptr(), mask.data_ptr(), rows.obs.data_ptr(), rows.share_obs.data_ptr(),
                rows.available_actions.data_ptr(), rows.to_move.data_ptr(), rows.flags.data_ptr(), self.n,
                self.share_mode, *(self._rules + (self._stream(),))), "mappo_hanabi_reset")
            return self.read_flags(rows) if readback else None

    def step(self, actions):
        """actions [n] int (move uid, -1 = leave alone; a device tensor is used where it is) -> fills rewards / status /
        scores and the rows of the players now to move.  Raises ValueError naming the table whose move was refused --
        after the other tables have advanced (see the module docstring)."""
        if not torch.is_tensor(actions):
            actions = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32).reshape(-1))
        a = actions.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        assert a.shape[0] == self.n
        flags = self.read_flags(self._launch_step(a))
        refused = np.flatnonzero(flag_status(flags) == STATUS_REFUSED)
        if refused.size:
            raise ValueError(REFUSED_MOVE % int(refused[0]))
        return flags

    def _launch_step(self, a):
        """The two launches of a move on ``a`` ([n] int32, contiguous, on the device) -> the rows they wrote."""
        rows = self.rows
        with torch.cuda.device(self.device):
            _native.check(self._lib.mappo_hanabi_step(
                self._state.data_ptr(), a.data_ptr(), self.rewards.data_ptr(), self.status.data_ptr(),
                self.scores.data_ptr(), rows.obs.data_ptr(), rows.share_obs.data_ptr(),
                rows.available_actions.data_ptr(), rows.to_move.data_ptr(), rows.flags.data_ptr(), self.n,
                self.share_mode, *(self._rules + (self._stream(),))), "mappo_hanabi_step")
        return rows

    def encode(self, active=None):
        """Fills obs / share_obs / available_actions / to_move (zero rows where ``active`` is False or the table was
        never reset)."""
        rows = self.rows
        mask = None if active is None else self._mask(active)
        with torch.cuda.device(self.device):
            _native.check(self._lib.mappo_hanabi_encode(
                self._state.data_ptr(), None if mask is None else mask.data_ptr(), rows.obs.data_ptr(),
                rows.share_obs.data_ptr(), rows.available_actions.data_ptr(), rows.to_move.data_ptr(), self.n,
                self.share_mode, *(self._rules + (self._stream(),))), "mappo_hanabi_encode")

    def draws(self):
        """32-bit words each table's generator has produced so far -> numpy [n] (624 words are one pass over its state)."""
        with torch.cuda.device(self.device):
            _native.check(self._lib.mappo_hanabi_draws(self._state.data_ptr(), self._draws.data_ptr(), self.n,
                                                       self._stream()), "mappo_hanabi_draws")
        return self._draws.cpu().numpy()

    def close(self):
        pass


class HanabiDeviceVecEnv(object):
    """All rollout threads of the turn-based Hanabi runner as one device batch.  Same contract as
    ``HanabiBatchVecEnv`` -- ``reset(reset_choose)`` -> (obs, share_obs, available_actions), ``step(actions)`` ->
    (obs, share_obs, rewards, dones, infos, available_actions) -- except that the rows and rewards are device tensors
    (``device_resident``), ``step`` takes the action tensor as it comes from the policy, and what reaches the host is
    ``self.flags``: the page-locked array of flags words of the call just made (``dones`` / ``infos`` are read off it).

    ``step`` and ``reset`` write different tensors: the rows ``step`` returned stay valid through the next ``reset``
    (which zeroes the rows of the tables it does not restart) and are overwritten by the next ``step``."""

    device_resident = True

    def __init__(self, all_args, seeds, device):
        rules = rules_for(all_args.hanabi_name, all_args.num_agents)
        share = SHARE_ALL_PLAYERS if all_args.use_obs_instead_of_state else SHARE_OWN_HAND
        self.batch = HanabiDeviceBatch(rules, seeds, share, device)
        b = self.batch
        self.device = b.device
        self._reset_rows = b.new_rows()
        self.num_envs = b.n
        self.players = b.players
        self.action_space = [Discrete(b.num_moves) for _ in range(b.players)]
        self.observation_space = [[b.obs_len + b.players] for _ in range(b.players)]
        self.share_observation_space = [[b.share_len + b.players] for _ in range(b.players)]
        self.flags = np.full(b.n, STATUS_IDLE, dtype=np.int32)
        self.flags_device = b.rows.flags

    def can_move(self):
        """[n, 1] float32 on the host: 1 where the table's player to move has a legal move (after the last call)."""
        return flag_can_move(self.flags).astype(np.float32)[:, None]

    def reset(self, reset_choose=None):
        b, rows = self.batch, self._reset_rows
        choose = np.ones(b.n, dtype=bool) if reset_choose is None else np.asarray(reset_choose, dtype=bool)
        any_chosen = bool(choose.any())
        flags = b.reset(choose, into=rows, readback=any_chosen)
        # nothing restarted: every table reports idle, and there is nothing to read back
        self.flags = flags if any_chosen else np.full(b.n, STATUS_IDLE, dtype=np.int32)
        self.flags_device = rows.flags
        return rows.obs, rows.share_obs, rows.available_actions

    def step(self, actions):
        b = self.batch
        if not torch.is_tensor(actions):
            actions = torch.from_numpy(np.asarray(actions))
        self.flags = b.step(actions.reshape(b.n, -1)[:, 0])
        self.flags_device = b.rows.flags
        rewards = b.rewards.view(b.n, 1, 1).expand(b.n, b.players, 1)
        dones = _DONE_OF_STATUS[flag_status(self.flags)]
        infos = _ScoreInfos(flag_score(self.flags))
        return b.obs, b.share_obs, rewards, dones, infos, b.available_actions

    # ---- the host-free contract of the "device turns" route (runner/shared/hanabi_turns.py): launches only, no readback.
    # ``self.flags`` / ``flags_device`` / ``can_move()`` belong to the calls above and are NOT kept current by these.
    graph_safe = True       # step_device advances the tensors ``state_names`` lists in place: a capture can replay it
    state_names = ("table_state", "step_obs", "step_share_obs", "step_available_actions", "step_to_move", "step_flags",
                   "step_rewards", "step_status", "step_scores")
    table_state = property(lambda self: self.batch._state)      # the tables and their generators
    step_obs = property(lambda self: self.batch.rows.obs)
    step_share_obs = property(lambda self: self.batch.rows.share_obs)
    step_available_actions = property(lambda self: self.batch.rows.available_actions)
    step_to_move = property(lambda self: self.batch.rows.to_move)
    step_flags = property(lambda self: self.batch.rows.flags)
    step_rewards = property(lambda self: self.batch.rewards)      # [n]: every player of a table gets the same reward
    step_status = property(lambda self: self.batch.status)
    step_scores = property(lambda self: self.batch.scores)

    def step_device(self, env_actions):
        """``env_actions`` [n] int32 on the device, taken as it is (-1: the table sits out) -> the two launches of a move.
        Results: ``step_obs`` / ``step_share_obs`` / ``step_available_actions`` / ``step_flags`` / ``step_rewards`` -- the same
        tensors every call.  A refused move shows as status 255 in ``step_flags``; nothing is read back, nothing raised."""
        b = self.batch
        assert env_actions.dtype == torch.int32 and env_actions.shape == (b.n,) and env_actions.is_contiguous() \
            and env_actions.device == b.device
        b._launch_step(env_actions)

    def reset_device(self, mask):
        """``mask`` [n] uint8 on the device: new games where it is set -- none where it is all zero; the two launches run
        either way.  -> (obs, share_obs, available_actions, flags) of the reset: the same tensors every call, zero rows
        and status idle for the tables it left alone.  Nothing is read back."""
        b, rows = self.batch, self._reset_rows
        assert mask.dtype == torch.uint8 and mask.shape == (b.n,) and mask.is_contiguous() and mask.device == b.device
        b.reset(mask, into=rows, readback=False)
        return rows.obs, rows.share_obs, rows.available_actions, rows.flags

    def close(self):
        self.batch.close()
