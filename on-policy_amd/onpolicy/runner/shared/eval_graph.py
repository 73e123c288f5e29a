"""One evaluation step of the device-resident eval loop as ONE graph launch (``train_mpe.py --use_device_eval``).

With the eval worlds on the GPU a step of ``MPERunner.eval`` (reference onpolicy/runner/shared/mpe_runner.py:142-190) --
the actor's forward, its deterministic action (K14 mode), the env step (K11 family), mask / RNN-state bookkeeping and the
running reward totals -- depends on nothing on the host, like a rollout step without critic, sampling and slab write.
It is captured once per runner, on the first ``eval()``, with the warm-up / capture / snapshot-restore /
pointer-stability / fall-back machinery of rollout_graph.py, and replayed ``episode_length`` times per evaluation.

Carried state, in static tensors: the current observation, masks, the actor's RNN states (recurrent policies) and the
totals the captured step adds the rewards to.  Everything is recorded on one stream: there is no critic branch.  An
evaluation begins with ``reset_in_place()`` on the eval worlds -- ``reset()`` rebinds the state tensors whose addresses the
graph holds -- zero totals and RNN states, masks of 1.  Building the graph consumes nothing: the eval worlds' generator is
put back, and neither the training worlds, the buffer nor torch's default device generator is touched (the deterministic
action draws nothing).

``MAPPO_EVAL_GRAPH=0`` keeps the eager tensor loop of ``MPERunner.eval``, which is also what runs where
``rollout_graph.capturable`` says no (a CPU device, ``MAPPO_ROLLOUT_GRAPH=0``) or capture fails.
"""
import os

import torch

from onpolicy.runner.shared import rollout_graph


class EvalGraph(rollout_graph.RolloutGraph):
    def __init__(self, runner):
        dev = torch.device(runner.device)
        self._init_common(runner, dev)
        self.envs = runner.eval_envs
        self.N = runner.n_eval_rollout_threads
        self._alloc(runner, dict(dtype=torch.float32, device=dev))
        self.totals = torch.zeros(self.N, self.A, 1, dtype=torch.float32, device=dev)
        self._obs0 = None       # what the last in-place reset returned

    def _alloc(self, runner, f32):
        N, A = self.N, self.A
        self.recurrent = runner.trainer.policy.actor._recurrent
        self.cur_obs = torch.empty(N, A, self.envs.observation_space[0].shape[0], **f32)
        self.cur_masks = torch.empty(N, A, 1, **f32)
        # (feed-forward policies hand the states back as they got them: these stay zero)
        self.cur_rnn_a = torch.zeros(N, A, runner.recurrent_N, runner.hidden_size, **f32)

    # -- the step itself: the runner's eager step on the static tensors, captured once
    @torch.no_grad()
    def _body(self):
        obs, rnn_a, masks, rewards = self.r._device_eval_step(self.cur_obs, self.cur_rnn_a, self.cur_masks)
        self._carry(obs, rnn_a, masks)
        self.totals.add_(rewards)
        return None, None

    def _carry(self, obs, rnn_a, masks):
        self.cur_obs.copy_(obs)
        self.cur_masks.copy_(masks)
        if self.recurrent:
            self.cur_rnn_a.copy_(rnn_a)

    def _carried(self):
        return [self.cur_obs, self.cur_masks, self.totals] + ([self.cur_rnn_a] if self.recurrent else [])

    def _start(self, obs):
        self.cur_obs.copy_(obs)
        self.cur_masks.fill_(1.0)
        self.cur_rnn_a.zero_()

    def begin_episode(self):
        """The state an evaluation starts from, given the observations of the reset just made."""
        self._start(self._obs0)
        self.totals.zero_()

    def begin(self):
        """A new evaluation: the worlds restart where they are, the carried state goes back to its beginning."""
        self._obs0 = self.envs.reset_in_place()
        self.begin_episode()

    def capture(self):
        """``RolloutGraph.capture`` on freshly reset worlds; the reset's draws are handed back, so that the first
        evaluation starts from the worlds it would have started from without a graph."""
        rng = self.envs.rng.get_state()
        self._obs0 = self.envs.reset_in_place()
        try:
            return super().capture()
        finally:
            self.envs.rng.set_state(rng)

    def step(self):
        self.graph.replay()
        self.replays += 1


def enabled():
    return os.environ.get("MAPPO_EVAL_GRAPH", "1") != "0"


def build(runner, make=EvalGraph):
    """-> a captured eval graph for ``runner``, or None when the evaluation has to stay on the eager tensor loop."""
    dev = runner.device
    if not enabled() or not rollout_graph.capturable(runner.eval_envs, dev):
        return None
    return rollout_graph.captured(lambda: make(runner), dev, what="eval")


@torch.no_grad()
def totals(runner, make=EvalGraph):
    """The reward totals [N, A, 1] of one evaluation on ``runner``'s device-resident eval worlds, as a device tensor (kept
    in ``runner.eval_totals``): ``episode_length`` replays of the captured step where ``make`` can be captured -- tried
    once per runner, on the first evaluation, and kept in ``runner.eval_graph`` -- and the eager tensor loop on
    ``runner._device_eval_step`` otherwise.  The policies are in rollout mode already."""
    if not hasattr(runner, "eval_graph"):
        runner.eval_graph = build(runner, make)
    g = runner.eval_graph
    if g is not None:
        g.begin()
        for _ in range(runner.episode_length):
            g.step()
        total = g.totals
    else:
        obs, rnn_states, masks = runner._device_eval_begin(runner.eval_envs.reset_in_place())
        total = torch.zeros(runner.n_eval_rollout_threads, runner.num_agents, 1, dtype=torch.float32,
                            device=runner.eval_envs.device)
        for _ in range(runner.episode_length):
            obs, rnn_states, masks, rewards = runner._device_eval_step(obs, rnn_states, masks)
            total += rewards
    runner.eval_totals = total
    return total
