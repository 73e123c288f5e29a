"""The turn bookkeeping of a Hanabi move (reference onpolicy/runner/shared/hanabi_runner_forward.py:138-220) on tensors.

What follows an env step is the same on every route of ``HanabiRunner`` (runner/shared/hanabi_routes.py) and stands here
once: ``settle_move`` and ``settle_finished``, on explicit masks.  The host-decided routes call them with what the host saw.
The host-free route ("device turns", ``--use_device_turns``) reads who moves and which games restart off the flags word K16
writes per table, so there the whole bookkeeping is two operations, one before the env step and one after it:

  ``turn_begin``  the movers' rows and the policy's outputs -> slot ``agent`` of the turn tensors; the env's actions (-1: sits out)
  ``turn_end``    the settling, the counters the host used to keep (moves, finished games, their scores), who can move next

For HIP tensors each is ONE launch of libmappo_hip.so (K17: csrc/mappo_turn.hip, ``mappo_hanabi_turn_begin`` / ``_end``).
A recurrent policy (``--use_device_turns_rnn``) also carries its two RNN states per (table, player) through the moves:
``turn_begin`` puts the movers' new states into slot ``agent``, ``turn_end`` clears every player's at a finished table --
the same two operations on operands that know the states (``TurnOperands(recurrent=True)``), the same one launch each
(``mappo_hanabi_turn_begin_rnn`` / ``_end_rnn``).
On any other device -- and on the GPU with ``MAPPO_TURN_KERNELS=0`` -- the same thing is done with framework ops: the
specification the kernels are tested against bit for bit (tests/test_gpu_hanabi_turns.py, test_gpu_hanabi_turns_rnn.py), which also lets the route's
logic run without a GPU (tests/test_hanabi_turns_cpu.py).  Neither form reads anything back.  ``merge_restarted`` is the
per-buffer-step counterpart (framework ops): the rows ``reset`` just dealt go into the static current rows in place.
"""
import torch

from onpolicy import _native
from onpolicy.envs.hanabi.device import STATUS_FINISHED, STATUS_REFUSED, STATUS_RUNNING, flag_can_move, flag_score, flag_status
from onpolicy.runner.shared import hanabi_moves
from onpolicy.runner.shared.hanabi_moves import launch, use_kernels

ROW_FIELDS = ("obs", "share_obs", "available_actions")
SCALAR_FIELDS = ("values", "actions", "action_log_probs", "rewards", "rewards_since_last_action", "masks", "active_masks")
STATE_FIELDS = ("rnn_states", "rnn_states_critic")      # [N, A, recurrent_N, H]: a recurrent route's only


class TurnOperands(hanabi_moves.MoveOperands):
    """Everything a move of the route reads and writes besides the policy's and the env's outputs: the turn tensors
    (``turn``: a ``_TurnState``, [N, A, W] each), the static current rows [N, W] and the route's own state [N].
    ``recurrent``: the moves also keep ``turn.rnn_states`` / ``turn.rnn_states_critic`` (the ``_rnn`` entry points)."""

    COUNTERS = (("moves", torch.int64), ("games", torch.int32), ("score_sum", torch.int32), ("refused", torch.uint8))

    def __init__(self, turn, use_obs, use_share_obs, use_available_actions, recurrent=False):
        super(TurnOperands, self).__init__(use_obs.shape[0], turn.obs.shape[1], use_obs.device)
        self.turn, self.recurrent = turn, bool(recurrent)
        self.use_obs, self.use_share_obs, self.use_available_actions = use_obs, use_share_obs, use_available_actions
        self.reset_choose = torch.zeros(self.n, dtype=torch.uint8, device=self.device)

    def state_tensors(self):
        """What a move changes in place besides the env's own tensors (a graph capture saves and restores these)."""
        t = self.turn
        return [getattr(t, k) for k in ROW_FIELDS + SCALAR_FIELDS + (STATE_FIELDS if self.recurrent else ())] + \
            [self.use_available_actions, self.can_move, self.reset_choose, self.env_actions, self.counter_block]

    def _describe(self):
        """The ``mappo_hanabi_turn`` (K17) of these operands: the turn tensors, the current rows and the restart marks;
        for a recurrent route the ``mappo_hanabi_turn_rnn``: the same and the two state tensors."""
        o, t, n, A = self, self.turn, self.n, self.players
        d = _native.HanabiTurnRnn() if o.recurrent else _native.HanabiTurn()
        for name, use in zip(ROW_FIELDS, (o.use_obs, o.use_share_obs, o.use_available_actions)):
            field = getattr(t, name)
            w = use.shape[1]
            if tuple(field.shape) != (n, A, w) or tuple(use.shape) != (n, w):
                raise ValueError("turn tensor %s %s does not match its current rows %s" % (name, tuple(field.shape), tuple(use.shape)))
            for x in (field, use):
                if x.dtype != torch.float32 or not x.is_contiguous() or x.device != o.device:
                    raise ValueError("%s: K17 takes contiguous float32 tensors on one device" % name)
            setattr(d, name, field.data_ptr())
            setattr(d, "use_" + name, use.data_ptr())
        for name in SCALAR_FIELDS:
            field = getattr(t, name)
            if tuple(field.shape) != (n, A, 1) or field.dtype != torch.float32 or not field.is_contiguous():
                raise ValueError("turn tensor %s: expected contiguous float32 %s, got %s" % (name, (n, A, 1), tuple(field.shape)))
            setattr(d, name, field.data_ptr())
        if o.recurrent:
            shape = tuple(t.rnn_states.shape)
            for name in STATE_FIELDS:
                field = getattr(t, name)
                if field.dim() != 4 or tuple(field.shape) != shape or shape[:2] != (n, A) or field.dtype != torch.float32 or \
                        not field.is_contiguous() or field.device != o.device:
                    raise ValueError("turn tensor %s: expected contiguous float32 (%d, %d, recurrent_N, hidden) on %s, got %s"
                                     % (name, n, A, o.device, tuple(field.shape)))
                setattr(d, name, field.data_ptr())
            d.rnn_w = shape[2] * shape[3]
        d.reset_choose = o.reset_choose.data_ptr()
        d.obs_w, d.share_w, d.avail_w = o.use_obs.shape[1], o.use_share_obs.shape[1], o.use_available_actions.shape[1]
        return d


# ---------------------------------------------------------------------------------------- the two operations
@torch.no_grad()
def turn_begin(o, agent, value, action, logp, rnn_new=None, rnn_new_critic=None):
    """Before the env step of player ``agent``'s move.  value / action (int64) / logp: the policy's outputs on ALL N
    rows ([N, 1]); what it drew for a table that sits out is discarded.  rnn_new / rnn_new_critic ([N, recurrent_N, H]):
    its new states on all rows, read by recurrent operands only."""
    if o.recurrent and (rnn_new is None or rnn_new_critic is None):
        raise ValueError("turn_begin: recurrent operands take the policy's new RNN states")
    if use_kernels(o.can_move):
        dynamic = dict(value=(value, o.n, torch.float32), action=(action, o.n, torch.int64), logp=(logp, o.n, torch.float32))
        if o.recurrent:
            numel = o.turn.rnn_states[:, agent].numel()
            dynamic.update(rnn_new=(rnn_new, numel, torch.float32), rnn_new_critic=(rnn_new_critic, numel, torch.float32))
        return launch(o, "mappo_hanabi_turn_begin_rnn" if o.recurrent else "mappo_hanabi_turn_begin", agent, **dynamic)
    t, n = o.turn, o.n
    m = o.can_move != 0
    mc = m.view(n, 1)
    act = action.reshape(n)
    o.env_actions.copy_(torch.where(m, act.to(torch.int32), torch.full_like(o.env_actions, -1)))
    for name, use in zip(ROW_FIELDS, (o.use_obs, o.use_share_obs, o.use_available_actions)):
        slot = getattr(t, name)[:, agent]
        slot.copy_(torch.where(mc, use, slot))
    for slot, new in ((t.values[:, agent], value), (t.actions[:, agent], act), (t.action_log_probs[:, agent], logp)):
        slot.copy_(torch.where(mc, new.reshape(n, 1).to(torch.float32), slot))
    if o.recurrent:
        for name, new in zip(STATE_FIELDS, (rnn_new, rnn_new_critic)):
            slot = getattr(t, name)[:, agent]
            slot.copy_(torch.where(m.view(n, 1, 1), new.reshape(slot.shape).to(torch.float32), slot))


@torch.no_grad()
def turn_end(o, agent, flags, rewards_env):
    """After the env step.  flags [N] int32: K16's words of that step; rewards_env [N]: its rewards.  ``o.can_move`` still
    holds what ``turn_begin`` read; it leaves with who can move next."""
    if use_kernels(o.can_move):
        return launch(o, "mappo_hanabi_turn_end_rnn" if o.recurrent else "mappo_hanabi_turn_end", agent,
                      flags=(flags, o.n, torch.int32), rewards_env=(rewards_env, o.n, torch.float32))
    t, n = o.turn, o.n
    flags = flags.reshape(n)
    m = o.can_move != 0
    status = flag_status(flags)
    done = status == STATUS_FINISHED
    settle_move(t, agent, m, status == STATUS_RUNNING, rewards_env)
    settle_finished(t, agent, done, o.use_available_actions)
    if o.recurrent:         # the states restart with the game, every player's
        for name in STATE_FIELDS:
            getattr(t, name).masked_fill_(done.view(n, 1, 1, 1), 0.0)
    # what the host used to keep: moves, games flagged for restart and counted, refused moves, who can move next
    o.moves.add_(m.to(torch.int64))
    o.reset_choose.copy_(torch.where(done, torch.ones_like(o.reset_choose), o.reset_choose))
    o.games.add_(done.to(torch.int32))
    o.score_sum.add_(torch.where(done, flag_score(flags), torch.zeros_like(flags)))
    o.refused.copy_(torch.where(status == STATUS_REFUSED, torch.ones_like(o.refused), o.refused))
    o.can_move.copy_(torch.where(done, torch.zeros_like(flags), flag_can_move(flags)))


@torch.no_grad()
def settle_move(turn, agent, moved, alive, rewards):
    """The acting player collects what accumulated since its previous move and everybody at a table that moved accrues the
    new reward (the reward of buffer step 0 is discarded by the shift in ``run()``); in running games the current player
    stays live.  moved: bool [N] on the device, or None for "every table"; alive: bool [N]; rewards: [N] or [N, A, 1]."""
    rsla = turn.rewards_since_last_action
    n = rsla.shape[0]
    rewards = rewards.reshape(n, -1, 1)
    if moved is None:
        turn.rewards[:, agent] = rsla[:, agent]
        rsla[:, agent] = 0.0
        rsla += rewards
    else:
        mc = moved.view(n, 1)
        turn.rewards[:, agent] = torch.where(mc, rsla[:, agent], turn.rewards[:, agent])
        rsla[:, agent] = torch.where(mc, torch.zeros_like(rsla[:, agent]), rsla[:, agent])
        rsla.copy_(torch.where(moved.view(n, 1, 1), rsla + rewards, rsla))
    live, one = alive.view(n, 1), torch.ones_like(turn.masks[:, agent])
    turn.masks[:, agent] = torch.where(live, one, turn.masks[:, agent])
    turn.active_masks[:, agent] = torch.where(live, one, turn.active_masks[:, agent])


@torch.no_grad()
def settle_finished(turn, agent, done, use_available_actions):
    """Finished games (done: bool [N]): nobody may act; the current player is active, the players after it are inactive,
    their accrued rewards are flushed and their values and rows zeroed."""
    t, rsla = turn, turn.rewards_since_last_action
    n, A = rsla.shape[:2]
    dc, d3 = done.view(n, 1), done.view(n, 1, 1)
    use_available_actions.masked_fill_(dc, 0.0)
    t.masks.masked_fill_(d3, 0.0)
    t.active_masks[:, agent] = torch.where(dc, torch.ones_like(t.active_masks[:, agent]), t.active_masks[:, agent])
    if agent + 1 < A:
        rest = slice(agent + 1, A)
        t.rewards[:, rest] = torch.where(d3, rsla[:, rest], t.rewards[:, rest])
        for field in (t.active_masks, rsla, t.values, t.obs, t.share_obs):
            field[:, rest] = torch.where(d3, torch.zeros_like(field[:, rest]), field[:, rest])


@torch.no_grad()
def merge_restarted(o, obs, share_obs, available_actions, flags):
    """Once per buffer step, after ``reset`` on the tables ``o.reset_choose`` marks: their new rows (the reset's tensors)
    replace the old ones in the static current rows, they can move as the reset's flags say, and the marks are cleared."""
    n = o.n
    rc = o.reset_choose != 0
    rcc = rc.view(n, 1)
    torch.where(rcc, obs, o.use_obs, out=o.use_obs)
    if o.use_share_obs.data_ptr() != o.use_obs.data_ptr():
        torch.where(rcc, share_obs, o.use_share_obs, out=o.use_share_obs)
    torch.where(rcc, available_actions, o.use_available_actions, out=o.use_available_actions)
    torch.where(rc, flag_can_move(flags.reshape(n)), o.can_move, out=o.can_move)
    o.reset_choose.zero_()
