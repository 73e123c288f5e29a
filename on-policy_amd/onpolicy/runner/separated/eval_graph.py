"""One evaluation step of the separated runner's device-resident eval loop as ONE graph launch: the separated analogue
of runner/shared/eval_graph.py, which it inherits everything from but the shape of the carried state.

With one policy per agent (``--share_policy``: simple_speaker_listener, simple_push) an evaluation step (reference
onpolicy/runner/separated/mpe_runner.py:179-235) is every agent's actor forward and deterministic action (K14 mode), the
agents' integer actions side by side into the env step, and masks / RNN states per agent.  The carried state is kept per
agent -- current observation (``eval_envs.agent_obs(obs, i)``), masks, the actor's RNN states -- next to the one totals
tensor [N, A, 1]; the agents' branches are recorded on one stream, in agent order.
"""
import torch

from onpolicy.runner.shared import eval_graph as shared


class SeparatedEvalGraph(shared.EvalGraph):
    def _alloc(self, runner, f32):
        N = self.N
        self.recurrent = any(tr.policy.actor._recurrent for tr in runner.trainer)
        self.cur_obs = [torch.empty(N, space.shape[0], **f32) for space in self.envs.observation_space]
        self.cur_masks = [torch.empty(N, 1, **f32) for _ in range(self.A)]
        self.cur_rnn_a = [torch.zeros(N, runner.recurrent_N, runner.hidden_size, **f32) for _ in range(self.A)]

    def _carry(self, obs, rnn_a, masks):
        for i in range(self.A):
            self.cur_obs[i].copy_(obs[i])
            self.cur_masks[i].copy_(masks[i])
            if self.recurrent:
                self.cur_rnn_a[i].copy_(rnn_a[i])

    def _carried(self):
        return self.cur_obs + self.cur_masks + [self.totals] + (self.cur_rnn_a if self.recurrent else [])

    def _start(self, obs):
        for i in range(self.A):
            self.cur_obs[i].copy_(self.envs.agent_obs(obs, i))
            self.cur_masks[i].fill_(1.0)
            self.cur_rnn_a[i].zero_()

    def _prep_rollout(self):
        for tr in self.r.trainer:
            tr.prep_rollout()
