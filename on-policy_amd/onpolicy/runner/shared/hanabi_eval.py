"""Hanabi evaluation on the device (``--use_device_eval``): the bookkeeping of an evaluation move (reference
onpolicy/runner/shared/hanabi_runner_forward.py:229 onwards) on tensors, and the route that plays a whole evaluation with it.

Evaluation bookkeeping is not training bookkeeping (runner/shared/hanabi_turns.py): no buffer slots, rewards or masks, but a
final score per table, the actor's RNN state carried per (table, player) through a whole game, and finished tables that are
never restarted.  Who moves and which games ended are read off the flags word K16 writes per table, so a move is two
operations around the env step:

  ``eval_begin``  the env's actions (-1: the table sits out); the movers' new RNN states -> slot ``agent`` of the carried states
  ``eval_end``    moves, finished games and their scores, refused moves, the finished tables' legal-move rows cleared, who can
                  move next

For HIP tensors each is ONE launch of libmappo_hip.so (K18: csrc/mappo_turn.hip, ``mappo_hanabi_eval_begin`` / ``_end``).  On
any other device -- and on the GPU with ``MAPPO_TURN_KERNELS=0`` -- the same thing is done with framework ops: the
specification the kernels are tested against bit for bit (tests/test_gpu_hanabi_eval.py), which also lets the route's logic
run without a GPU (tests/test_hanabi_eval_cpu.py).  Neither form reads anything back.

``DeviceEval`` is the route: ``HanabiRunner._eval_games`` hands over to its ``games()`` when the eval envs are device tables
and the flag is given.  A move -- the actor's forward on ALL N rows, its deterministic action (K14 mode), ``eval_begin``, the
env's two launches (K16), ``eval_end`` -- is launches only, and is replayed from a captured graph, one per agent index
(hanabi_moves.py).  The host reads ONE block of counters every ``MAPPO_HANABI_EVAL_POLL`` rounds of A moves and stops
when every table has finished.
"""
import os

import numpy as np
import torch

from onpolicy import _native
from onpolicy.envs.hanabi.batch import rules_for
from onpolicy.envs.hanabi.device import STATUS_FINISHED, STATUS_REFUSED, STATUS_RUNNING, flag_can_move, flag_score, flag_status
from onpolicy.runner.shared import eval_graph, hanabi_moves
from onpolicy.runner.shared.hanabi_moves import launch, use_kernels

# rounds of A moves between two reads of the counter block (``MAPPO_HANABI_EVAL_POLL``)
DEFAULT_POLL = 4


class EvalOperands(hanabi_moves.MoveOperands):
    """Everything an evaluation move reads and writes besides the policy's and the env's outputs: the static current rows
    [N, W], who can move and the env's actions [N], the actor's RNN states [N, A, recurrent_N, hidden] and the per-table
    counters."""

    COUNTERS = (("moves", torch.int64), ("games", torch.int32), ("scores", torch.int32), ("refused", torch.uint8))

    def __init__(self, use_obs, use_available_actions, players, recurrent_N, hidden, recurrent):
        super(EvalOperands, self).__init__(use_obs.shape[0], players, use_obs.device)
        self.use_obs, self.use_available_actions, self.recurrent = use_obs, use_available_actions, bool(recurrent)
        f32 = dict(dtype=torch.float32, device=self.device)
        # (feed-forward policies hand the states back as they got them: these stay zero)
        self.rnn_states = torch.zeros(self.n, self.players, recurrent_N, hidden, **f32)
        self.masks = torch.ones(self.n, 1, **f32)

    def begin(self, flags):
        """The state an evaluation starts from; ``flags``: the words of the reset just made."""
        self.can_move.copy_(flag_can_move(flags.reshape(self.n)))
        self.env_actions.fill_(-1)
        self.rnn_states.zero_()
        self.counter_block.zero_()
        self.scores.fill_(-1)

    def state_tensors(self):
        """What a move changes in place besides the env's own tensors (a graph capture saves and restores these)."""
        return [self.use_available_actions, self.can_move, self.env_actions, self.rnn_states, self.counter_block]

    def _describe(self):
        """The ``mappo_hanabi_eval`` (K18) of these operands: the legal-move rows and the carried RNN states."""
        o, avail, rnn = self, self.use_available_actions, self.rnn_states
        for name, x in (("use_available_actions", avail), ("rnn_states", rnn)):
            if x.dtype != torch.float32 or not x.is_contiguous() or x.device != o.device:
                raise ValueError("%s: K18 takes contiguous float32 tensors on one device" % name)
        if avail.dim() != 2 or avail.shape[0] != o.n or rnn.shape[:2] != (o.n, o.players):
            raise ValueError("K18: rows %s / states %s do not match %d tables of %d players"
                             % (tuple(avail.shape), tuple(rnn.shape), o.n, o.players))
        d = _native.HanabiEval()
        d.use_available_actions = avail.data_ptr()
        d.rnn_states = rnn.data_ptr() if o.recurrent else None
        d.avail_w, d.rnn_w = avail.shape[1], rnn.shape[2] * rnn.shape[3]
        return d


# ---------------------------------------------------------------------------------------- the two operations
@torch.no_grad()
def eval_begin(o, agent, action, rnn_new):
    """Before the env step of player ``agent``'s move.  action (int64, [N, 1]) / rnn_new ([N, recurrent_N, hidden]; read for
    a recurrent policy only): the actor's outputs on ALL N rows; what it computed for a table that sits out is discarded."""
    if use_kernels(o.can_move):
        dynamic = dict(action=(action, o.n, torch.int64))
        if o.recurrent:
            dynamic["rnn_new"] = (rnn_new, o.rnn_states[:, agent].numel(), torch.float32)
        return launch(o, "mappo_hanabi_eval_begin", agent, **dynamic)
    n = o.n
    m = o.can_move != 0
    o.env_actions.copy_(torch.where(m, action.reshape(n).to(torch.int32), torch.full_like(o.env_actions, -1)))
    if o.recurrent:
        slot = o.rnn_states[:, agent]
        slot.copy_(torch.where(m.view(n, 1, 1), rnn_new.reshape(slot.shape).to(torch.float32), slot))


@torch.no_grad()
def eval_end(o, agent, flags):
    """After the env step.  flags [N] int32: K16's words of that step.  ``o.can_move`` still holds what ``eval_begin`` read;
    it leaves with who can move next.  A finished table is counted once and never moves again."""
    if use_kernels(o.can_move):
        return launch(o, "mappo_hanabi_eval_end", agent, flags=(flags, o.n, torch.int32))
    n = o.n
    flags = flags.reshape(n)
    m = o.can_move != 0
    status = flag_status(flags)
    done = m & (status == STATUS_FINISHED)
    o.moves.add_(m.to(torch.int64))
    o.scores.copy_(torch.where(done, flag_score(flags), o.scores))
    o.games.add_(done.to(torch.int32))
    o.use_available_actions.masked_fill_(done.view(n, 1), 0.0)
    o.refused.copy_(torch.where(status == STATUS_REFUSED, torch.ones_like(o.refused), o.refused))
    o.can_move.copy_(torch.where(m & (status == STATUS_RUNNING), flag_can_move(flags), torch.zeros_like(flags)))


# ---------------------------------------------------------------------------------------------- the route
def move_bound(rules):
    """No game under ``rules`` has more moves than this.  With D cards left after the deal at most D + players moves play
    or discard (each draws while the deck lasts; after the last card everybody moves once more); a hint costs a token, and
    tokens come from the initial ``max_information_tokens``, a discard or a completed colour: at most that many hints.  So
    moves <= 2 (D + players) + max_information_tokens + colours <= 2 * cards + 2 * players + tokens + colours."""
    colours, ranks = int(rules["colors"]), int(rules["ranks"])
    per_colour = sum(3 if k == 0 else (1 if k == ranks - 1 else 2) for k in range(ranks))    # csrc/hanabi_rules.h: copies
    return 2 * per_colour * colours + 2 * int(rules["players"]) + int(rules["max_information_tokens"]) + colours


def poll_rounds():
    return max(1, int(os.environ.get("MAPPO_HANABI_EVAL_POLL", DEFAULT_POLL)))


class DeviceEval(object):
    """One evaluation on the runner's device-resident eval tables: ``games()`` -> the final scores, numpy [N]."""

    def __init__(self, runner):
        self.r, self.envs = runner, runner.eval_envs
        self.n, self.players = runner.n_eval_rollout_threads, runner.num_agents
        self.max_moves = move_bound(rules_for(runner.all_args.hanabi_name, runner.num_agents))
        self.ops = None
        # what the last evaluation did (tests, tools): rounds of A moves played, reads of the counter block, its counters
        self.rounds, self.readbacks, self.counters = 0, 0, None

    def _begin(self):
        """New games on every table (their generators continue), the operands back to their beginning."""
        e = self.envs
        if self.ops is None:
            actor = self.r.trainer.policy.actor
            # static current rows: the tensors the env's step writes
            self.ops = EvalOperands(e.step_obs, e.step_available_actions, self.players, self.r.recurrent_N, self.r.hidden_size,
                                    actor._recurrent)
            self._all = torch.ones(self.n, dtype=torch.uint8, device=self.ops.device)
        o = self.ops
        obs, _, available_actions, flags = e.reset_device(self._all)
        o.use_obs.copy_(obs)
        o.use_available_actions.copy_(available_actions)
        o.begin(flags)

    def move(self, agent_id):
        """Forward on all N rows, ``eval_begin``, the env step, ``eval_end``: launches only (what the graphs capture)."""
        o, e = self.ops, self.envs
        action, rnn_new = self.r.trainer.policy.act(o.use_obs, o.rnn_states[:, agent_id], o.masks, o.use_available_actions,
                                                    deterministic=True)
        eval_begin(o, agent_id, action, rnn_new)
        e.step_device(o.env_actions)
        eval_end(o, agent_id, e.step_flags)

    def _poll(self):
        self.readbacks += 1
        c = self.counters = self.ops.read_counters()
        hanabi_moves.raise_if_refused(c)
        return bool((c["games"] > 0).all())

    @torch.no_grad()
    def games(self):
        self.r.trainer.prep_rollout()
        self._begin()
        if not hasattr(self, "graphs"):         # tried once per runner, on the first evaluation
            self.graphs = hanabi_moves.build(self.r, self, self.envs, self.n, self.r.device, with_value_head=False,
                                             enabled=eval_graph.enabled(), what="Hanabi eval move")
        poll = poll_rounds()
        self.rounds, self.readbacks = 0, 0
        while True:
            for agent_id in range(self.players):
                if self.graphs is not None:
                    self.graphs[agent_id].step()
                else:
                    self.move(agent_id)
            self.rounds += 1
            # overshooting is harmless: a finished table has an all-zero legal-move row, gets -1, and is counted once
            past = self.rounds * self.players >= self.max_moves
            if self.rounds % poll == 0 or past:
                if self._poll():
                    return self.counters["scores"].copy()
                if past:
                    running = np.flatnonzero(self.counters["games"] == 0)
                    raise RuntimeError("Hanabi evaluation: after %d moves (no game under these rules has more than %d) "
                                       "tables %s have not finished" % (self.rounds * self.players, self.max_moves,
                                                                        running.tolist()))
