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

``MAPPO_GROUPED_ROLLOUT_RNN=1`` on top of it (read at the same places) lets the route take recurrent policies too: the recurrent
K19 kernel (``mappo_grouped_rnn_prepare`` / ``mappo_grouped_rnn_forward``) carries every network through trunk, GRU cell, the
LayerNorm behind it, head and sampling, and reads and writes the RNN states.  Without it recurrent policies are refused.
"""
import os

import torch

from onpolicy import _native
from . import fused_mlp


def enabled():
    return os.environ.get("MAPPO_GROUPED_ROLLOUT", "0") == "1"


def rnn_enabled():
    return enabled() and os.environ.get("MAPPO_GROUPED_ROLLOUT_RNN", "0") == "1"


def _blocks(base):
    return [base.mlp.fc1] + list(base.mlp.fc2)


def _rnn_refusal(net, eps):
    """Why the recurrent K19 kernel does not take this actor's or critic's RNNLayer (None: it does)."""
    if net._recurrent_N != 1:
        return "recurrent_N = %d" % net._recurrent_N
    gru, norm = net.rnn.rnn, net.rnn.norm
    if (gru.input_size, gru.hidden_size) != (fused_mlp.HIDDEN, fused_mlp.HIDDEN) or not gru.bias or gru.bidirectional:
        return "a GRU that is not 64 -> 64 with biases"
    if not norm.elementwise_affine or norm.bias is None or float(norm.eps) != eps:
        return "an RNN LayerNorm without affine parameters or with another eps than the trunk's"
    return None


def refusal(policies, available_actions=False, recurrent=False):
    """Why these policies stay on the per-agent route (None: K19 takes them).  ``recurrent``: the recurrent kernel may be
    used -- policies whose actors and critics are ALL recurrent (one GRU layer 64 -> 64) are taken then."""
    from . import distributions
    if distributions.SAMPLING_RNG != "device":
        return "the host sampling mode draws on the CPU generator"
    if available_actions:
        return "available_actions are not masked in the kernel"
    if not 1 <= 2 * len(policies) <= _native.GROUPED_MAX_NETS:
        return "%d agents: more networks than one launch takes" % len(policies)
    for po in policies:
        actor, critic = po.actor, po.critic
        if (actor._recurrent or critic._recurrent) and not recurrent:
            return "recurrent policies"
        if not (actor._recurrent == critic._recurrent == policies[0].actor._recurrent):
            return "a mixed set of recurrent and feed-forward networks"
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
        for net in (actor, critic) if actor._recurrent else ():
            why = _rnn_refusal(net, float(_blocks(net.base)[0][2].eps))
            if why is not None:
                return why
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


def _describe_rnn(e, net, h_in, mask, h_out):
    """Fill the recurrent part of descriptor ``e`` for ``net`` (an actor or critic) -> its parameter tensors."""
    gru, norm = net.rnn.rnn, net.rnn.norm
    params = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, norm.weight, norm.bias]
    e.w_ih, e.w_hh, e.b_ih, e.b_hh, e.rnn_g, e.rnn_b = (t.data_ptr() for t in params)
    e.h_in, e.mask, e.h_out = h_in.data_ptr(), mask.data_ptr(), h_out.data_ptr()
    return params


class GroupedRollout(object):
    """The prepared launch for ``policies`` (``refusal`` returned None) reading ``joint`` [N, sum(obs_dims)], a static
    contiguous float32 device tensor the caller refreshes before every ``forward``.  ``keep_logits``: the actors' head
    outputs are written too (``logits``, per agent [N, n]); the rollout itself needs only actions and log-probabilities.

    Recurrent policies (``refusal(..., recurrent=True)`` returned None): ``states`` = per-agent lists (h_a, h_c, masks) of
    static contiguous float32 tensors [N, 1, 64], [N, 1, 64], [N, 1] the launch reads -- the caller's own (the captured
    step's carried state) or, by default, tensors of this object the caller refreshes like ``joint``; ``new_h_a`` /
    ``new_h_c`` receive the new states, and ``forward`` returns them too."""

    def __init__(self, policies, obs_dims, joint, centralized, keep_logits=False, states=None):
        N, dev = int(joint.shape[0]), joint.device
        assert joint.dim() == 2 and joint.stride(1) == 1 and joint.shape[1] == sum(obs_dims) and len(obs_dims) == len(policies)
        self.rows, self.G = N, 2 * len(policies)
        sizes = [int(po.actor.act.action_out.linear.weight.shape[0]) for po in policies]
        self.noise = torch.empty(N * sum(sizes), dtype=torch.float32, device=dev)       # every actor's [N, n_i], one draw
        self.values = [torch.empty((N, 1), dtype=torch.float32, device=dev) for _ in policies]
        self.actions = [torch.empty((N, 1), dtype=torch.int64, device=dev) for _ in policies]
        self.logp = [torch.empty((N, 1), dtype=torch.float32, device=dev) for _ in policies]
        self.logits = [torch.empty((N, n), dtype=torch.float32, device=dev) for n in sizes] if keep_logits else None
        self.recurrent = bool(policies[0].actor._recurrent)
        nets = ((_native.GroupedRnnNet if self.recurrent else _native.GroupedNet) * self.G)()
        if self.recurrent:
            state = lambda *shape: [torch.zeros((N,) + shape, dtype=torch.float32, device=dev) for _ in policies]
            self.h_a, self.h_c, self.masks = states if states is not None else (state(1, 64), state(1, 64), state(1))
            self.new_h_a, self.new_h_c = state(1, 64), state(1, 64)
            for t, shape in [(t, (N, 1, 64)) for t in self.h_a + self.h_c] + [(t, (N, 1)) for t in self.masks]:
                assert t.shape == shape and t.is_contiguous() and t.dtype == torch.float32 and t.device == dev
        net_of = (lambda e: e.net) if self.recurrent else (lambda e: e)
        self._params = []
        lo = at = 0
        for i, (po, width, n) in enumerate(zip(policies, obs_dims, sizes)):
            # the critics, whose rows are the long ones, first: their workgroups start first
            c, a = net_of(nets[i]), net_of(nets[len(policies) + i])
            self._params += _describe(c, po.critic.base, po.critic.v_out, joint, 0 if centralized else lo)
            c.y = self.values[i].data_ptr()
            self._params += _describe(a, po.actor.base, po.actor.act.action_out.linear, joint, lo)
            assert a.din == width and c.din == (joint.shape[1] if centralized else width), "obs_dims do not match the networks"
            a.noise = self.noise[at:at + N * n].data_ptr()
            a.actions, a.logp = self.actions[i].data_ptr(), self.logp[i].data_ptr()
            a.y = self.logits[i].data_ptr() if keep_logits else None
            lo, at = lo + width, at + N * n
            if self.recurrent:
                self._params += _describe_rnn(nets[i], po.critic, self.h_c[i], self.masks[i], self.new_h_c[i])
                self._params += _describe_rnn(nets[len(policies) + i], po.actor, self.h_a[i], self.masks[i], self.new_h_a[i])
        self._where = [t.data_ptr() for t in self._params]
        lib = _native.lib()
        size, prepare = (lib.mappo_grouped_rnn_table_bytes, lib.mappo_grouped_rnn_prepare) if self.recurrent else \
            (lib.mappo_grouped_table_bytes, lib.mappo_grouped_prepare)
        self.table = torch.empty(int(size(self.G)), dtype=torch.uint8, device=dev)
        _native.check(prepare(nets, self.G, self.table.data_ptr()), prepare.__name__)

    def check_parameters(self):
        """The table holds the parameters' addresses: an optimiser step in place keeps them, a rebound tensor does not."""
        if self._where != [t.data_ptr() for t in self._params]:
            raise RuntimeError("a parameter of the grouped rollout's networks moved: the prepared table is stale")

    @torch.no_grad()
    def forward(self):
        """-> (values, actions, log-probs): per-agent lists of the static [N, 1] tensors, valid until the next call;
        recurrent policies: -> (values, actions, log-probs, new_h_a, new_h_c)."""
        self.noise.exponential_(1.0)
        if self.recurrent:
            _native.check(_native.lib().mappo_grouped_rnn_forward(self.table.data_ptr(), self.G, self.rows,
                                                                  _native.stream_of(self.table.device)),
                          "mappo_grouped_rnn_forward")
            return self.values, self.actions, self.logp, self.new_h_a, self.new_h_c
        _native.check(_native.lib().mappo_grouped_forward(self.table.data_ptr(), self.G, self.rows,
                                                          _native.stream_of(self.table.device)), "mappo_grouped_forward")
        return self.values, self.actions, self.logp


def build(policies, envs, joint, centralized, available_actions=False, states=None):
    """-> the GroupedRollout of a runner's policies on ``joint`` (recurrent ones: on ``states``, see there), or None (with
    the reason printed once) where K19 does not take them."""
    why = refusal(policies, available_actions, rnn_enabled()) if hasattr(envs, "obs_dims") else "worlds without obs_dims"
    if why is not None:
        print("grouped rollout: %s; the per-agent step runs" % why)
        return None
    return GroupedRollout(policies, envs.obs_dims, joint, centralized, states=states)
