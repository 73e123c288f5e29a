"""The PPO loss of R_MAPPO.ppo_update for a MultiDiscrete action head written with torch ops (act.py, multi-discrete branch
of evaluate_actions: one Categorical per sub-head, no availability mask; r_mappo.py:119-153), shared by the CPU and the
device tests of ``mappo_ppo_loss_multi_f32``.  The value half, the judge and the caps are those of tests/loss_reference.py:

* ``torch_loss``: the expression itself, dtype-generic -- float32 and float64 tensors go through the same ops and autograd;
* ``make_inputs``: seeded inputs, one action per sub-head drawn from that head's softmax;
* ``near_boundary``: per (row, head) PAIR the ratios that sit within ``MARGIN`` of 1 +- clip -- a head's logit gradient
  depends on that head's clip branch only, so only that head's columns are left out of a gradient comparison -- and the
  value rows of ``loss_reference.near_boundary``.
"""
import torch

import loss_reference as lr
from loss_reference import Judge, SKIP_CAP, MARGIN      # noqa: F401  (the device tests take them from here)

INPUT_NAMES = ("logits", "actions", "old_logp", "adv", "active", "values", "value_preds", "returns")


def _value_half(values, value_preds, returns, active, norm, terms, **kw):
    """K7's value loss through ``loss_reference.torch_loss`` (one dummy action of probability 1 as the actor half)."""
    rows = values.shape[0]
    zero = values.new_zeros(rows, 1)
    t = {} if terms is not None else None
    _, _, value_loss, _ = lr.torch_loss(zero, None, zero, zero, zero, active, None, values, value_preds, returns, norm,
                                        terms=t, **kw)
    if terms is not None:
        terms["value"] = t["value"]
    return value_loss


def torch_loss(logits, head_sizes, actions, old_logp, adv, active, values, value_preds, returns, norm, *, clip,
               huber_delta, entropy_coef, value_loss_coef, use_huber, use_clipped, p_active, v_active, terms=None):
    """-> (policy_loss, entropy, value_loss, ratio [rows, heads]) in the dtype of the tensors given.
    ``terms``: a dict that receives the per-row terms of the four sums the kernel accumulates (detached)."""
    logps, ents = [], []
    for x, act in zip(logits.split(list(head_sizes), -1), actions.t()):
        dist = torch.distributions.Categorical(logits=x)
        logps.append(dist.log_prob(act.long()).unsqueeze(-1))
        ents.append(dist.entropy())
    ratio = torch.exp(torch.cat(logps, -1) - old_logp)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)
    per = -surr.sum(-1, keepdim=True)
    if p_active:
        policy_loss = (per * active).sum() / active.sum()
        entropy = sum((e * active.squeeze(-1)).sum() / active.sum() for e in ents) / len(ents)
    else:
        policy_loss = per.mean()
        entropy = sum(e.mean() for e in ents) / len(ents)
    value_loss = _value_half(values, value_preds, returns, active, norm, terms, clip=clip, huber_delta=huber_delta,
                             entropy_coef=entropy_coef, value_loss_coef=value_loss_coef, use_huber=use_huber,
                             use_clipped=use_clipped, p_active=p_active, v_active=v_active)
    if terms is not None:
        wp = active if p_active else torch.ones_like(active)
        ent_row = torch.stack(ents, -1).mean(-1, keepdim=True)
        terms.update(policy=(per * wp).detach(), entropy=(ent_row * wp).detach(),
                     ratio=ratio.detach().mean(-1, keepdim=True))
    return policy_loss, entropy, value_loss, ratio


def make_inputs(rows, head_sizes, mode="plain", seed=0):
    """Seeded float32 CPU inputs of one minibatch span -> dict over INPUT_NAMES.  Per sub-head the action is drawn from the
    head's softmax and the old log-prob is the current one plus noise.
    ``mode="wide"``: logits x 30, old log-probs off by N(0, 5), advantages x 1e3 -- ratios from e-20 to e+20, all finite."""
    assert mode in ("plain", "wide")
    wide = mode == "wide"
    width, k = sum(head_sizes), len(head_sizes)
    g = torch.Generator(device="cpu").manual_seed(1000003 * seed + 8191 * k + 131 * width + rows + (7 if wide else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)                   # noqa: E731
    logits = rnd(rows, width) * (30.0 if wide else 2.0)
    actions, old_logp = [], []
    for x in logits.split(list(head_sizes), -1):
        logp = torch.log_softmax(x.double(), -1)
        a = torch.multinomial(logp.exp(), 1, generator=g)
        actions.append(a)
        old_logp.append((logp.gather(1, a) + rnd(rows, 1).double() * (5.0 if wide else 0.2)).float())
    adv = rnd(rows, 1) * (1e3 if wide else 1.0)
    active = (torch.rand(rows, 1, generator=g) < 0.8).float()
    active[0] = 1.0
    values = rnd(rows, 1)
    value_preds = values + rnd(rows, 1) * 0.3
    returns = rnd(rows, 1) * 3 + 1
    out = dict(logits=logits, actions=torch.cat(actions, -1).float(), old_logp=torch.cat(old_logp, -1), adv=adv,
               active=active, values=values, value_preds=value_preds, returns=returns)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    return out


def near_boundary(inputs, head_sizes, norm, *, clip, huber_delta, margin=MARGIN):
    """-> (pairs, value_rows): bool [rows, heads] of the (row, head) pairs whose ratio, in float64, lies within ``margin``
    of 1 - clip or 1 + clip, and bool [rows] of the rows near one of K7's value-side branch points."""
    d = lr.to(inputs, dtype=torch.float64)
    logp = torch.cat([torch.log_softmax(x, -1).gather(1, a.long().unsqueeze(-1))
                      for x, a in zip(d["logits"].split(list(head_sizes), -1), d["actions"].t())], -1)
    ratio = torch.exp(logp - d["old_logp"])
    pairs = ((ratio - (1 - clip)).abs() < margin) | ((ratio - (1 + clip)).abs() < margin)
    rows = d["values"].shape[0]
    zero = torch.zeros(rows, 1)
    k7 = dict(logits=zero, avail=None, actions=zero, old_logp=zero, values=inputs["values"],
              value_preds=inputs["value_preds"], returns=inputs["returns"])
    _, value_rows = lr.near_boundary(k7, norm, clip=clip, huber_delta=huber_delta, margin=margin)
    return pairs, value_rows


def columns_of(pairs, head_sizes):
    """A [rows, heads] mask spread over the heads' logit columns -> [rows, sum head_sizes]."""
    return torch.repeat_interleave(pairs, torch.tensor(list(head_sizes), device=pairs.device), dim=1)


def clear_rows(inputs, rows, head_sizes, norm, *, clip, huber_delta):
    """The first ``rows`` rows of ``inputs`` with no pair and no value branch near a boundary (spans of a few hundred rows
    are compared on every row)."""
    pairs, value_rows = near_boundary(inputs, head_sizes, norm, clip=clip, huber_delta=huber_delta)
    idx = torch.nonzero(~(pairs.any(-1) | value_rows)).reshape(-1)[:rows]
    assert idx.numel() == rows
    return {k: v[idx].contiguous() for k, v in inputs.items()}
