"""One rollout step of the separated runner's device-resident loop as ONE graph launch: the separated analogue of
runner/shared/rollout_graph.py, whose warm-up, capture, snapshot / restore of worlds and generators, pointer-stability
check and fall-back to the eager loop it inherits.

With one policy and one buffer per agent (``--share_policy``: simple_speaker_listener, whose agents differ in their
observation and action spaces, and simple_push, whose two or more agents differ in their observations and rewards) a rollout step is every agent's actor and critic forward and action sampling (K14), the
agents' integer actions side by side into the env step (K11 family), and the mask / RNN-state bookkeeping per agent
(reference onpolicy/runner/separated/mpe_runner.py:94-177: collect -> envs.step -> insert): twice the launches of the
shared step on half the rows.  The captured step reads and advances a carried state per agent -- current observation,
masks, RNN states of recurrent policies, plus the joint observation of the centralised critics -- and leaves every
agent's results in static tensors; a replay is followed by one ``buffer[i].insert`` (one fused slab write, K2) per agent.
The agents' branches are recorded on one stream, in agent order: the eager loop's kernels in the eager loop's order.

Stays eager (``build`` returns None) where the shared step does, and under a PopArt value head: its ``update`` rebinds
the head's parameters, and the static-head mechanism of the shared graph is not carried over to one head per agent.
"""
import torch

from onpolicy.runner.shared import rollout_graph as shared


class SeparatedRolloutGraph(shared.RolloutGraph):
    def __init__(self, runner):
        bufs = runner.buffer
        dev = bufs[0].device
        self._init_common(runner, dev)      # (popart stays None: build() leaves PopArt heads to the eager loop)
        f32 = dict(dtype=torch.float32, device=dev)
        # carried state of the loop, per agent
        self.cur_obs = [torch.empty(b.obs.shape[1:], **f32) for b in bufs]
        self.cur_masks = [torch.empty(b.masks.shape[1:], **f32) for b in bufs]
        self.recurrent = bufs[0].rnn_states.stride()[0] != 0
        if self.recurrent:
            self.cur_rnn_a = [torch.empty(b.rnn_states.shape[1:], **f32) for b in bufs]
            self.cur_rnn_c = [torch.empty(b.rnn_states_critic.shape[1:], **f32) for b in bufs]
        else:       # feed-forward policies: the buffers' zero views serve every step
            self.cur_rnn_a = [b.rnn_states[0] for b in bufs]
            self.cur_rnn_c = [b.rnn_states_critic[0] for b in bufs]
        # the centralised critics all read the joint observation: carried once
        self.cur_joint = torch.empty(bufs[0].share_obs.shape[1:], **f32) if runner.use_centralized_V else None

    @torch.no_grad()
    def _body(self):
        r, N = self.r, self.N
        agents = range(self.A)
        values, actions, logp, rnn_a, rnn_c = [], [], [], [], []
        for i, tr in zip(agents, r.trainer):
            share = self.cur_joint if r.use_centralized_V else self.cur_obs[i]
            v, a, lp, ha, hc = tr.policy.get_actions(share, self.cur_obs[i], self.cur_rnn_a[i], self.cur_rnn_c[i],
                                                     self.cur_masks[i])
            values.append(v), actions.append(a), logp.append(lp), rnn_a.append(ha), rnn_c.append(hc)
        obs, rewards, dones, infos = self.envs.step(torch.cat(actions, -1))
        masks = torch.where(dones, 0.0, 1.0)                        # [N, A]: 0 where the episode ended (one launch)
        # the carried state of the next step; the slab writes take the static tensors as they are
        if r.use_centralized_V:
            self.cur_joint.copy_(obs)
        out = []
        for i in agents:
            self.cur_obs[i].copy_(self.envs.agent_obs(obs, i))
            self.cur_masks[i].copy_(masks[:, i:i + 1])
            if self.recurrent:
                # finished agents restart from a zero RNN state (reference mpe_runner.py:151-154)
                self.cur_rnn_a[i].copy_(rnn_a[i] * self.cur_masks[i].view(N, 1, 1))
                self.cur_rnn_c[i].copy_(rnn_c[i] * self.cur_masks[i].view(N, 1, 1))
            share_next = self.cur_joint if r.use_centralized_V else self.cur_obs[i]
            out.append((share_next, self.cur_obs[i], self.cur_rnn_a[i], self.cur_rnn_c[i], actions[i], logp[i],
                        values[i], rewards[:, i].contiguous(), self.cur_masks[i]))
        return out, infos

    def _carried(self):
        joint = [self.cur_joint] if self.cur_joint is not None else []
        rnn = self.cur_rnn_a + self.cur_rnn_c if self.recurrent else []
        return joint + self.cur_obs + self.cur_masks + rnn

    def _prep_rollout(self):
        for tr in self.r.trainer:
            tr.prep_rollout()

    def begin_episode(self):
        """Row 0 of every agent's buffer is the state the rollout starts from (warmup() / after_update() put it there)."""
        bufs = self.r.buffer
        if self.cur_joint is not None:
            self.cur_joint.copy_(bufs[0].share_obs[0])
        for i, b in enumerate(bufs):
            self.cur_obs[i].copy_(b.obs[0])
            self.cur_masks[i].copy_(b.masks[0])
            if self.recurrent:
                self.cur_rnn_a[i].copy_(b.rnn_states[0])
                self.cur_rnn_c[i].copy_(b.rnn_states_critic[0])

    def step(self):
        """One rollout step: graph launch + one fused slab write per agent into its buffer's current row."""
        self.graph.replay()
        self.replays += 1
        for b, out in zip(self.r.buffer, self.out):
            b.insert(*out)
        return self.infos.fresh()


def build(runner):
    """-> a captured SeparatedRolloutGraph for ``runner``, or None when the step has to stay eager."""
    dev = runner.buffer[0].device
    if not shared.capturable(runner.envs, dev):
        return None
    if any(type(getattr(tr.policy.critic, "v_out", None)).__name__ == "PopArt" for tr in runner.trainer):
        return None
    return shared.captured(lambda: SeparatedRolloutGraph(runner), dev)
