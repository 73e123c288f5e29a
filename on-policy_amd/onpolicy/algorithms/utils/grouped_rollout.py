"""Grouped forward-and-sample (K19, ``mappo_grouped_prepare`` / ``mappo_grouped_forward``): every actor and critic of a
separated-runner rollout step -- one ``R_MAPPOPolicy`` per agent, the same architecture, different weights -- in ONE
launch, each network on its own column slice of the env's joint observation row (actors: ``envs.agent_obs``'s columns;
critics: the whole row under ``use_centralized_V``, else their agent's columns).  The launch leaves values, sampled
actions and their log-probabilities in static tensors; with the one ``exponential_()`` draw of all actors' noise in front
of it that is the policies' whole side of a step (reference runner/separated/mpe_runner.py:94-120 loops over the agents).

Opt-in: ``MAPPO_GROUPED_ROLLOUT=1``, read where the rollout graph / the runner's eager device loop is built.  The noise is
one tensor for all agents instead of one draw per agent, so the route samples other trajectories than the per-agent
route from the first step on (same distribution).  ``refusal`` names what the kernel does not take; the per-agent body
runs then.
"""
import os

import torch

from onpolicy import _native
from . import fused_mlp


def enabled():
    return os.environ.get("MAPPO_GROUPED_ROLLOUT", "0") == "1"


def _blocks(base):
    return [base.mlp.fc1] + list(base.mlp.fc2)


def refusal(policies, available_actions=False):
    """Why these policies stay on the per-agent route (None: K19 takes them)."""
    from . import distributions
    if distributions.SAMPLING_RNG != "device":
        return "the host sampling mode draws on the CPU generator"
    if available_actions:
        return "available_actions are not masked in the kernel"
    if not 1 <= 2 * len(policies) <= _native.GROUPED_MAX_NETS:
        return "%d agents: more networks than one launch takes" % len(policies)
    for po in policies:
        actor, critic = po.actor, po.critic
        if actor._recurrent or critic._recurrent:
            return "recurrent policies"
        if actor.act.action_type != "Discrete":
            return "a %s action space" % actor.act.action_type
        if type(critic.v_out).__name__ == "PopArt":
            return "a PopArt head rebinds its parameters"
        heads = ((actor.base, actor.act.action_out.linear), (critic.base, critic.v_out))
        for base, head in heads:
            if not hasattr(base, "mlp") or base.hidden_size != fused_mlp.HIDDEN:
                return "a trunk that is not an MLPBase of hidden size 64"
            blocks = _blocks(base)
            if len(blocks) not in (2, 3):
                return "layer_N = %d" % (len(blocks) - 1)
            eps = {float(b[2].eps) for b in blocks} | ({float(base.feature_norm.eps)} if base._use_feature_normalization else set())
            if len(eps) != 1 or any(fused_mlp._act_kind(b[1]) is None or b[0].bias is None for b in blocks):
                return "a trunk the fused kernels do not evaluate"
            if head.bias is None or head.weight.shape[0] > _native.GROUPED_MAX_OUT \
                    or blocks[0][0].weight.shape[1] > _native.GROUPED_MAX_DIN:
                return "a head of more than %d outputs or an input wider than %d" % (_native.GROUPED_MAX_OUT,
                                                                                      _native.GROUPED_MAX_DIN)
    p = policies[0].actor.base.mlp.fc1[0].weight
    if not p.is_cuda or p.dtype != torch.float32:
        return "parameters that are not float32 on a HIP device"
    return None


def _describe(d, base, head, joint, col):
    """Fill descriptor ``d`` for head(base(joint[:, col:col + din])) -> the parameter tensors it points into."""
    blocks = _blocks(base)
    params = []

    def at(t):
        params.append(t)
        return t.data_ptr()
    d.src, d.ld, d.col, d.din = joint.data_ptr(), joint.stride(0), col, blocks[0][0].weight.shape[1]
    d.n_layers, d.act, d.hidden, d.ln_eps = len(blocks), fused_mlp._act_kind(blocks[0][1]), base.hidden_size, blocks[0][2].eps
    if base._use_feature_normalization:
        d.in_g, d.in_b = at(base.feature_norm.weight), at(base.feature_norm.bias)
    d.w1 = at(blocks[0][0].weight)
    for l, blk in enumerate(blocks):
        d.bias[l], d.ln_g[l], d.ln_b[l] = at(blk[0].bias), at(blk[2].weight), at(blk[2].bias)
        if l:
            d.w2[l - 1] = at(blk[0].weight)
    d.wh, d.bh, d.out = at(head.weight), at(head.bias), head.weight.shape[0]
    return params


class GroupedRollout(object):
    """The prepared launch for ``policies`` (``refusal`` returned None) reading ``joint`` [N, sum(obs_dims)], a static
    contiguous float32 device tensor the caller refreshes before every ``forward``.  ``keep_logits``: the actors' head
    outputs are written too (``logits``, per agent [N, n]); the rollout itself needs only actions and log-probabilities."""

    def __init__(self, policies, obs_dims, joint, centralized, keep_logits=False):
        N, dev = int(joint.shape[0]), joint.device
        assert joint.dim() == 2 and joint.stride(1) == 1 and joint.shape[1] == sum(obs_dims) and len(obs_dims) == len(policies)
        self.rows, self.G = N, 2 * len(policies)
        sizes = [int(po.actor.act.action_out.linear.weight.shape[0]) for po in policies]
        self.noise = torch.empty(N * sum(sizes), dtype=torch.float32, device=dev)       # every actor's [N, n_i], one draw
        self.values = [torch.empty((N, 1), dtype=torch.float32, device=dev) for _ in policies]
        self.actions = [torch.empty((N, 1), dtype=torch.int64, device=dev) for _ in policies]
        self.logp = [torch.empty((N, 1), dtype=torch.float32, device=dev) for _ in policies]
        self.logits = [torch.empty((N, n), dtype=torch.float32, device=dev) for n in sizes] if keep_logits else None
        nets = (_native.GroupedNet * self.G)()
        self._params = []
        lo = at = 0
        for i, (po, width, n) in enumerate(zip(policies, obs_dims, sizes)):
            # the critics, whose rows are the long ones, first: their workgroups start first
            c, a = nets[i], nets[len(policies) + i]
            self._params += _describe(c, po.critic.base, po.critic.v_out, joint, 0 if centralized else lo)
            c.y = self.values[i].data_ptr()
            self._params += _describe(a, po.actor.base, po.actor.act.action_out.linear, joint, lo)
            assert a.din == width and c.din == (joint.shape[1] if centralized else width), "obs_dims do not match the networks"
            a.noise = self.noise[at:at + N * n].data_ptr()
            a.actions, a.logp = self.actions[i].data_ptr(), self.logp[i].data_ptr()
            a.y = self.logits[i].data_ptr() if keep_logits else None
            lo, at = lo + width, at + N * n
        self._where = [t.data_ptr() for t in self._params]
        lib = _native.lib()
        self.table = torch.empty(int(lib.mappo_grouped_table_bytes(self.G)), dtype=torch.uint8, device=dev)
        _native.check(lib.mappo_grouped_prepare(nets, self.G, self.table.data_ptr()), "mappo_grouped_prepare")

    def check_parameters(self):
        """The table holds the parameters' addresses: an optimiser step in place keeps them, a rebound tensor does not."""
        if self._where != [t.data_ptr() for t in self._params]:
            raise RuntimeError("a parameter of the grouped rollout's networks moved: the prepared table is stale")

    @torch.no_grad()
    def forward(self):
        """-> (values, actions, log-probs): per-agent lists of the static [N, 1] tensors, valid until the next call."""
        self.noise.exponential_(1.0)
        _native.check(_native.lib().mappo_grouped_forward(self.table.data_ptr(), self.G, self.rows,
                                                          _native.stream_of(self.table.device)), "mappo_grouped_forward")
        return self.values, self.actions, self.logp


def build(policies, envs, joint, centralized, available_actions=False):
    """-> the GroupedRollout of a runner's policies on ``joint``, or None (with the reason printed once) where K19 does not
    take them."""
    why = refusal(policies, available_actions) if hasattr(envs, "obs_dims") else "worlds without obs_dims"
    if why is not None:
        print("grouped rollout: %s; the per-agent step runs" % why)
        return None
    return GroupedRollout(policies, envs.obs_dims, joint, centralized)
