"""The rollout routes of ``HanabiRunner`` (runner/shared/hanabi_runner_forward.py), which picks one per run: ``HostTables``
(the default), ``DeviceTables`` (``--use_device_env``) and ``DeviceTurns`` (``--use_device_env --use_device_turns``).

A route has ``name``, ``warmup()`` (the first deal), ``begin_episode()``, ``collect(step)`` (the A moves of a buffer step; it
clears its own restart marks), ``restart()`` (new games on the tables ``collect`` marked; after ``chooseinsert``),
``score_summary()`` (-> {"games", "average_score"} of the episode so far; ``runner.true_total_num_steps`` up to date) and the
current rows ``use_obs`` / ``use_share_obs`` / ``use_available_actions``.  All write the turn tensors ``runner.turn``.
"""
import os

import numpy as np
import torch

from onpolicy.envs.hanabi.device import STATUS_FINISHED, STATUS_RUNNING, flag_status
from onpolicy.runner.shared import hanabi_moves, hanabi_turns
from onpolicy.runner.shared.base_runner import _t2n


class _HostStage(object):
    """Host arrays of one env call -> device tensors through one pinned staging buffer and one async copy (two
    buffers alternate; an event per buffer guards reuse).  On a CPU device: plain tensor views of copies."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs, self.turn = None, 0

    def upload(self, arrays):
        """arrays: list of numpy arrays -> list of float32 device tensors of the same shapes."""
        arrays = [np.asarray(a) for a in arrays]
        if self.device.type != "cuda":
            return [torch.from_numpy(np.array(a, dtype=np.float32)) for a in arrays]
        total = sum(a.size for a in arrays)
        if self.bufs is None or self.bufs[0][0].numel() < total:
            self.bufs = [(torch.empty(total, dtype=torch.float32, pin_memory=True),
                          torch.empty(total, dtype=torch.float32, device=self.device), [None]) for _ in range(2)]
        pin, dev, done = self.bufs[self.turn]
        self.turn = 1 - self.turn
        if done[0] is not None:
            done[0].synchronize()
        pin_np, out, off = pin.numpy(), [], 0
        for a in arrays:
            np.copyto(pin_np[off:off + a.size].reshape(a.shape), a, casting="unsafe")
            out.append(dev[off:off + a.size].view(a.shape))
            off += a.size
        dev[:off].copy_(pin[:off], non_blocking=True)
        done[0] = torch.cuda.Event()
        done[0].record(torch.cuda.current_stream(self.device))
        return out


def recurrent_policy(all_args):
    """Whether the run's policy carries RNN states (either recurrent flag)."""
    return bool(getattr(all_args, "use_recurrent_policy", False) or getattr(all_args, "use_naive_recurrent_policy", False))


class _Route(object):
    def __init__(self, runner):
        self.r = runner
        self.scores, self.turn_graphs = [], None


class _HostDecided(_Route):
    """The move loop both host-decided routes share.  Within one buffer step the agents act one after the other, only the
    envs whose current player has a legal move take part (``choose``), and a reward arrives only after the *other* players
    have moved.  The host keeps what decides control flow -- the legal-move table (``avail_host``: who moves), the done
    flags (``reset_choose``: which games restart) and the scores -- in the reference's order (:138-220).  The policy runs
    on the movers' rows only; the reference's masked numpy assignments are ``index_put`` / ``where`` updates (no boolean
    indexing on the device: that would synchronise).  A route says how rows and actions cross: the three ``_`` methods."""

    def warmup(self):
        r = self.r
        self.reset_choose = np.ones(r.n_rollout_threads, dtype=bool)
        obs, share_obs, available_actions = r.envs.reset(self.reset_choose)
        self._take_rows(obs, share_obs if r.use_centralized_V else obs, available_actions)

    def begin_episode(self):
        self.scores = []

    def score_summary(self):
        return {"games": len(self.scores), "average_score": np.mean(self.scores) if len(self.scores) > 0 else 0.0}

    def restart(self):
        r, rc = self.r, self.reset_choose
        obs, share_obs, available_actions = r.envs.reset(rc)
        if rc.any():
            self._merge_restarted(rc, obs, share_obs if r.use_centralized_V else obs, available_actions)

    @torch.no_grad()
    def collect(self, step):
        r, turn = self.r, self.r.turn
        n, A, dev = r.n_rollout_threads, r.num_agents, r.buffer.device
        self.reset_choose = np.zeros(n, dtype=bool)
        for agent_id in range(A):
            choose = np.any(self.avail_host == 1, axis=1)    # envs whose player can move
            if not np.any(choose):
                self.reset_choose = np.ones(n, dtype=bool)
                break
            # rows of the envs that move: a plain slice (views, no gather) when every env does; else ONE upload carries
            # their indices and, behind them, the mask ``settle_move`` takes
            sel_host, sel, moved = slice(None), slice(None), None
            if not choose.all():
                sel_host = np.flatnonzero(choose)
                up = torch.as_tensor(np.concatenate([sel_host, choose]), device=dev)
                sel, moved = up[:sel_host.size], up[sel_host.size:] != 0
            obs_c, share_c, avail_c = self.use_obs[sel], self.use_share_obs[sel], self.use_available_actions[sel]
            r.trainer.prep_rollout()
            value, action, action_log_prob, rnn_state, rnn_state_critic = r.trainer.policy.get_actions(
                share_c, obs_c, turn.rnn_states[sel, agent_id], turn.rnn_states_critic[sel, agent_id],
                turn.masks[sel, agent_id], avail_c)
            env_actions = self._env_actions((n,) + tuple(r.buffer.actions.shape[3:]), sel, sel_host, action)
            for field, new in ((turn.obs, obs_c), (turn.share_obs, share_c), (turn.available_actions, avail_c),
                               (turn.values, value), (turn.actions, action), (turn.action_log_probs, action_log_prob),
                               (turn.rnn_states, rnn_state), (turn.rnn_states_critic, rnn_state_critic)):
                field[sel, agent_id] = new.to(device=dev, dtype=torch.float32)
            obs, share_obs, rewards, dones, infos, available_actions = r.envs.step(env_actions)
            r.true_total_num_steps += int(choose.sum())
            done = np.asarray(dones) == True   # noqa: E712  (dones may hold None for idle envs)
            alive = np.asarray(dones) == False  # noqa: E712
            rewards_d, done_d, alive_d = self._take_rows(obs, share_obs if r.use_centralized_V else obs, available_actions,
                                                         rewards, done, alive)
            hanabi_turns.settle_move(turn, agent_id, moved, alive_d, rewards_d)
            self.reset_choose[done] = True
            if not done.any():
                continue
            # finished games: nobody may act, states restart, players after the current one are inactive
            hanabi_turns.settle_finished(turn, agent_id, done_d, self.use_available_actions)
            for states in (turn.rnn_states, turn.rnn_states_critic):
                states.masked_fill_(done_d.view(n, 1, 1, 1), 0.0)
            self.avail_host[done] = 0.0
            for i in np.flatnonzero(done):
                if 'score' in infos[i].keys():
                    self.scores.append(infos[i]['score'])


class HostTables(_HostDecided):
    """Per player move the only host -> device traffic is what the env just produced -- the observation / centralised
    observation / legal-move rows, the rewards and the done flags -- packed into one page-locked staging buffer and sent
    as ONE asynchronous copy (``_HostStage``); the actions come back as one device -> host transfer."""
    name = "host_tables"

    def __init__(self, runner):
        super(HostTables, self).__init__(runner)
        self._stage = _HostStage(runner.buffer.device)

    def _env_actions(self, shape, sel, sel_host, action):
        env_actions = -np.ones(shape, dtype=np.float32)
        env_actions[sel_host] = _t2n(action)     # the one device -> host transfer of a move: the env needs the actions
        return env_actions

    def _take_rows(self, obs, share_obs, available_actions, *after_step):
        """The env's rows -> ``use_*``; the legal-move table also stays on the host.  after_step: (rewards, done, alive)."""
        up = self._stage.upload([obs, share_obs, available_actions] + list(after_step))
        # clones: the staging area is reused two uploads later, these rows live until the next move
        self.use_obs, self.use_share_obs, self.use_available_actions = (t.clone() for t in up[:3])
        self.avail_host = np.array(available_actions, dtype=np.float32)
        return (up[3], up[4] > 0, up[5] > 0) if after_step else None

    def _merge_restarted(self, rc, obs, share_obs, available_actions):
        """Only the restarted games' rows cross to the device."""
        rows = torch.as_tensor(np.flatnonzero(rc), device=self.r.buffer.device)
        up = self._stage.upload([obs[rc], share_obs[rc], available_actions[rc]])
        for use, new in zip((self.use_obs, self.use_share_obs, self.use_available_actions), up):
            use[rows] = new
        self.avail_host[rc] = available_actions[rc]


class DeviceTables(_HostDecided):
    """``envs.device_resident`` (``HanabiDeviceVecEnv``): the current rows ARE the env's tensors (valid until its next
    step), the actions reach the env as a device tensor (-1 everywhere, the policy's action where a player moves), and
    ``avail_host`` shrinks to the [N, 1] "can move" column.  One small device -> host copy per move remains -- one int32
    flags word per table (status, can move, score): the host still decides who moves and which games restart."""
    name = "device_tables"

    def _env_actions(self, shape, sel, sel_host, action):
        env_actions = torch.full(shape, -1, dtype=torch.int32, device=self.r.buffer.device)
        env_actions[sel] = action.to(torch.int32).reshape((-1,) + shape[1:])
        return env_actions

    def _take_rows(self, obs, share_obs, available_actions, rewards=None, *host_flags):
        """-> (rewards, done, alive) of the call just made, on the device: the last two read off the flags words."""
        self.use_obs, self.use_share_obs, self.use_available_actions = obs, share_obs, available_actions
        self.avail_host = self.r.envs.can_move()
        status = flag_status(self.r.envs.flags_device)
        return rewards, status == STATUS_FINISHED, status == STATUS_RUNNING

    def _merge_restarted(self, rc, obs, share_obs, available_actions):
        """Restarted games' rows replace the old ones, on the device."""
        restarted = torch.as_tensor(rc, device=self.r.buffer.device).view(-1, 1)
        self.use_obs = torch.where(restarted, obs, self.use_obs)
        self.use_share_obs = torch.where(restarted, share_obs, self.use_share_obs)
        self.use_available_actions = torch.where(restarted, available_actions, self.use_available_actions)
        self.avail_host[rc] = self.r.envs.can_move()[rc]


class DeviceTurns(_Route):
    """Who moves and which games restart are read off the flags words ON the device (K17's two launches around the env
    step), the policy runs on ALL N rows of static current-row tensors (a table that sits out has an all-zero legal-move
    row; what is drawn for it is discarded and the env gets -1), and a move is replayed from a captured graph, one per
    agent index (hanabi_moves.py).  A buffer step copies nothing to the host and never synchronises: the restart
    marks are a device mask that ``restart()`` consumes and clears, the counters per-table accumulators.  NOT the
    host-decided routes' trajectories: the sampler's noise tensor is [N, moves] instead of [movers, moves], so from the
    first move with a table sitting out the same generator state gives other draws (hence opt-in); with a policy whose
    outputs do not depend on the batch the routes agree bit for bit (tests/test_hanabi_turns_cpu.py).  A recurrent policy
    (``--use_device_turns_rnn``) has its two RNN states per (table, player) kept by the same two launches: recurrent
    operands, whose state tensors a captured move snapshots with the rest (tests/test_hanabi_turns_rnn_cpu.py)."""
    name = "device_turns"

    def warmup(self):
        """Static current rows: the tensors the env's step writes; the first deal restarts every table; then the capture."""
        r, e = self.r, self.r.envs
        self.use_obs, self.use_available_actions = e.step_obs, e.step_available_actions
        self.use_share_obs = e.step_share_obs if r.use_centralized_V else e.step_obs
        self.ops = hanabi_turns.TurnOperands(r.turn, self.use_obs, self.use_share_obs, self.use_available_actions,
                                             recurrent=recurrent_policy(r.all_args))
        self.ops.reset_choose.fill_(1)
        self.restart()
        self.turn_graphs = hanabi_moves.build(r, self, e, r.n_rollout_threads, r.buffer.device, with_value_head=True,
                                              enabled=os.environ.get("MAPPO_TURN_GRAPH", "1") != "0", what="Hanabi move")

    def begin_episode(self):
        """The score list of the host-decided routes starts empty every episode: so do the games and their scores."""
        self.ops.games.zero_()
        self.ops.score_sum.zero_()

    def restart(self):
        """Always, whether or not any table is marked: reads nothing back."""
        obs, share_obs, available_actions, flags = self.r.envs.reset_device(self.ops.reset_choose)
        hanabi_turns.merge_restarted(self.ops, obs, share_obs if self.r.use_centralized_V else obs, available_actions, flags)

    @torch.no_grad()
    def collect(self, step):
        """A moves, each a graph replay or the same launches eagerly."""
        if self.turn_graphs is not None:
            return self.turn_graphs.buffer_step()
        self.r.trainer.prep_rollout()
        for agent_id in range(self.r.num_agents):
            self.move(agent_id)

    def move(self, agent_id):
        """Forward on all N rows, ``turn_begin``, the env step, ``turn_end``: launches only (what the graphs capture).  A
        recurrent policy's new states go where its outputs go: the movers' into slot ``agent_id`` (recurrent operands)."""
        r, turn, o, e = self.r, self.r.turn, self.ops, self.r.envs
        value, action, action_log_prob, rnn_state, rnn_state_critic = r.trainer.policy.get_actions(
            self.use_share_obs, self.use_obs, turn.rnn_states[:, agent_id], turn.rnn_states_critic[:, agent_id],
            turn.masks[:, agent_id], self.use_available_actions)
        hanabi_turns.turn_begin(o, agent_id, value, action, action_log_prob, rnn_state, rnn_state_critic)
        e.step_device(o.env_actions)
        hanabi_turns.turn_end(o, agent_id, e.step_flags, e.step_rewards)

    def score_summary(self):
        """The one readback of the route: moves / finished games / their scores / refused moves, summed over the tables."""
        c = self.ops.read_counters()
        hanabi_moves.raise_if_refused(c)
        self.r.true_total_num_steps = int(c["moves"].sum())
        games, score_sum = int(c["games"].sum()), int(c["score_sum"].sum())
        return {"games": games, "average_score": score_sum / games if games else 0.0}
