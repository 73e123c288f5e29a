"""The PPO loss of R_MAPPO.ppo_update written with torch ops (r_mappo.py:52-89 cal_value_loss, :119-153 policy loss and
entropy; FixedCategorical on masked logits), shared by the CPU and the device tests of K7 (``mappo_ppo_loss_f32``):

* ``torch_loss``: the expression itself, dtype-generic -- float32 and float64 tensors go through the same ops and autograd;
* ``make_inputs``: seeded inputs whose availability masks guarantee one available action at a RANDOM index;
* ``near_boundary``: the rows whose branch (surrogate clip, value clip, huber knee, larger value loss) could flip under
  float32 rounding, which a gradient comparison against float64 has to leave out;
* ``tie_table``: value-loss rows from dyadic numbers that sit EXACTLY on those branch points, with the gradient that
  torch's sub-gradient conventions give there;
* ``Judge``: "my float32 error against float64 is within 4 x torch's float32 error + a floor", with the measured figures
  collected for profiles/small_kernel_margins.json.
"""
import json
import os

import torch

MASKED = -1e10                      # distributions.py: the logit of an unavailable action
SKIP_CAP = 0.005                    # at most this share of rows may be left out of a gradient comparison, per half
MARGIN = 1e-4                       # distance to a branch point below which float32 rounding may pick the other branch
FLAGS = dict(use_huber=1, use_clipped=2, p_active=4, v_active=8)      # MAPPO_LOSS_* bits


def flag_kwargs(flags):
    return {k: bool(flags & bit) for k, bit in FLAGS.items()}


def masked_logits(logits, avail):
    return logits if avail is None else torch.where(avail == 0, torch.full_like(logits, MASKED), logits)


def torch_loss(logits, avail, actions, old_logp, adv, active, factor, values, value_preds, returns, norm, *,
               clip, huber_delta, entropy_coef, value_loss_coef, use_huber, use_clipped, p_active, v_active,
               terms=None):
    """The reference's formulas (FixedCategorical on masked logits; clipped surrogate; clipped huber / mse value
    loss) with torch ops, in the dtype of the tensors given -> (policy_loss, entropy, value_loss, ratio).
    ``terms``: a dict that receives the per-row terms of the four sums K7 accumulates (detached)."""
    x = masked_logits(logits, avail)
    dist = torch.distributions.Categorical(logits=x)
    logp = dist.log_prob(actions.squeeze(-1).long()).unsqueeze(-1)
    ent = dist.entropy()
    ratio = torch.exp(logp - old_logp)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)
    if factor is not None:
        surr = factor * surr
    per = -surr.sum(-1, keepdim=True)
    if p_active:
        policy_loss = (per * active).sum() / active.sum()
        entropy = (ent * active.squeeze(-1)).sum() / active.sum()
    else:
        policy_loss, entropy = per.mean(), ent.mean()
    target = returns if norm is None else (returns - norm[1]) / norm[0]
    vpc = value_preds + (values - value_preds).clamp(-clip, clip)
    e_c, e_o = target - vpc, target - values

    def loss(e):
        if not use_huber:
            return e ** 2 / 2
        a = (e.abs() <= huber_delta).to(e.dtype)
        return a * e ** 2 / 2 + (1 - a) * huber_delta * (e.abs() - huber_delta / 2)
    vl = torch.max(loss(e_o), loss(e_c)) if use_clipped else loss(e_o)
    value_loss = (vl * active).sum() / active.sum() if v_active else vl.mean()
    if terms is not None:
        wp = active if p_active else torch.ones_like(active)
        wv = active if v_active else torch.ones_like(active)
        terms.update(policy=(per * wp).detach(), entropy=(ent.unsqueeze(-1) * wp).detach(), value=(vl * wv).detach(),
                     ratio=ratio.detach())
    return policy_loss, entropy, value_loss, ratio


INPUT_NAMES = ("logits", "avail", "actions", "old_logp", "adv", "active", "factor", "values", "value_preds", "returns")


def make_inputs(rows, na, *, with_avail, mode="plain", seed=0, with_factor=False, single_share=0.03):
    """Seeded float32 CPU inputs of one minibatch span -> dict over INPUT_NAMES (``avail`` / ``factor`` may be None).

    Masks: every action available with probability 0.6, then one action at a uniformly random index made available (so
    action 0 is unavailable in ~0.4 (1 - 1/na) of the rows), and ``single_share`` of the rows keep ONLY that action.
    Actions are drawn from the masked softmax, old log-probs are the current ones plus noise.
    ``mode="wide"``: logits x 30, old log-probs off by N(0, 5), advantages x 1e3 -- ratios from e-20 to e+20, all finite."""
    assert mode in ("plain", "wide")
    wide = mode == "wide"
    g = torch.Generator(device="cpu").manual_seed(1000003 * seed + 131 * na + rows + (7 if wide else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    logits = rnd(rows, na) * (30.0 if wide else 2.0)
    avail = None
    if with_avail:
        avail = (torch.rand(rows, na, generator=g) < 0.6).float()
        keep = torch.randint(0, na, (rows, 1), generator=g)
        single = torch.rand(rows, 1, generator=g) < single_share
        avail = torch.where(single, torch.zeros_like(avail), avail)
        avail.scatter_(1, keep, 1.0)
    logp = torch.log_softmax(masked_logits(logits, avail).double(), -1)
    actions = torch.multinomial(logp.exp(), 1, generator=g)
    old_logp = (logp.gather(1, actions) + rnd(rows, 1).double() * (5.0 if wide else 0.2)).float()
    adv = rnd(rows, 1) * (1e3 if wide else 1.0)
    active = (torch.rand(rows, 1, generator=g) < 0.8).float()
    active[0] = 1.0
    factor = (torch.rand(rows, 1, generator=g) + 0.5) if with_factor else None
    values = rnd(rows, 1)
    value_preds = values + rnd(rows, 1) * 0.3
    returns = rnd(rows, 1) * 3 + 1
    out = dict(logits=logits, avail=avail, actions=actions.float(), old_logp=old_logp, adv=adv, active=active,
               factor=factor, values=values, value_preds=value_preds, returns=returns)
    for v in out.values():
        assert v is None or bool(torch.isfinite(v).all())
    return out


def to(inputs, device=None, dtype=None):
    """The inputs on ``device`` / in ``dtype`` (None entries stay None)."""
    return {k: (None if v is None else v.to(device=device, dtype=dtype)) for k, v in inputs.items()}


def near_boundary(inputs, norm, *, clip, huber_delta, margin=MARGIN):
    """-> (policy_rows, value_rows): bool [rows] masks, computed in float64, of the rows whose branch could flip under
    float32 rounding -- |ratio - (1 +- clip)|, ||v - vp| - clip|, ||e| - delta| for both errors and, where |v - vp| > clip,
    |l_c - l_o| (either loss form), each below ``margin``.  Independent of the flags, so that one mask serves them all."""
    d = to(inputs, dtype=torch.float64)
    logp = torch.log_softmax(masked_logits(d["logits"], d["avail"]), -1).gather(1, d["actions"].long())
    ratio = torch.exp(logp - d["old_logp"])
    policy = ((ratio - (1 - clip)).abs() < margin) | ((ratio - (1 + clip)).abs() < margin)
    v, vp = d["values"], d["value_preds"]
    target = d["returns"] if norm is None else (d["returns"] - float(norm[1])) / float(norm[0])
    dv = v - vp
    e_c, e_o = target - (vp + dv.clamp(-clip, clip)), target - v
    value = ((dv.abs() - clip).abs() < margin) | ((e_c.abs() - huber_delta).abs() < margin) | \
        ((e_o.abs() - huber_delta).abs() < margin)
    for huber in (False, True):
        def loss(e):
            if not huber:
                return e ** 2 / 2
            return torch.where(e.abs() <= huber_delta, e ** 2 / 2, huber_delta * (e.abs() - huber_delta / 2))
        value |= (dv.abs() > clip) & ((loss(e_c) - loss(e_o)).abs() < margin)
    return policy.reshape(-1), value.reshape(-1)


def clear_rows(inputs, rows, norm, *, clip, huber_delta):
    """The first ``rows`` rows of ``inputs`` that are NOT near a branch point.  For spans of a few hundred rows the 0.5 % cap
    allows one skipped row or none, so those tests run on rows chosen clear of the boundaries and compare every row."""
    p_rows, v_rows = near_boundary(inputs, norm, clip=clip, huber_delta=huber_delta)
    idx = torch.nonzero(~(p_rows | v_rows)).reshape(-1)[:rows]
    assert idx.numel() == rows
    return {k: (None if v is None else v[idx].contiguous()) for k, v in inputs.items()}


# ---------------------------------------------------------------------------------------------------- exact ties
TIE_CLIP, TIE_DELTA = 0.25, 0.5

# (v, vp, target, dL/dv with mse, dL/dv with huber) per row, before the 1 / rows of the mean.  Every number is a small dyadic
# rational, so float32 evaluates each expression exactly and the rows sit ON the branch points.  The gradients follow
# torch's conventions: clamp passes the gradient on its closed interval, (|e| <= delta) is closed, and torch.max gives each
# argument half the gradient on a tie -- with v - vp outside the clip the clipped branch has no gradient, so a tie of the two
# losses there leaves HALF of the plain branch's.
_TIES = [
    (1.25, 1.0, 1.5, -0.25, -0.25),             # v - vp = +clip: still inside the clamp, e_c = e_o
    (0.75, 1.0, 2.0, -1.25, -0.5),              # v - vp = -clip
    (1.0, 1.125, 1.5, -0.5, -0.5),              # |e_o| = |e_c| = delta, inside the clip: the quadratic branch
    (1.0, 0.875, 0.5, 0.5, 0.5),                # e_o = -delta
    (2.0, 1.0, 1.75, 0.0, 0.0),                 # |e_c| = delta with v - vp outside: l_c > l_o, the clipped branch, no gradient
    (1.25, 1.0, 1.75, -0.5, -0.5),              # v - vp = +clip and |e| = delta at once
    (1.0625, 1.0, 3.0, -1.9375, -0.5),          # l_c = l_o with v - vp inside the clip
    (1.0, 0.0, 0.625, 0.1875, 0.1875),          # l_c = l_o with v - vp outside (e_c = -e_o = 0.375): half of g_o
    (4.0, 0.0, 2.125, 0.9375, 0.25),            # the same beyond the huber knee (e_c = -e_o = 1.875)
    (0.0, 1.0, 0.375, -0.1875, -0.1875),        # ... and from below (v - vp = -1, e_o = -e_c = 0.375)
    (1.5, 1.0, 1.0, 0.5, 0.5),                  # outside the clip, l_o > l_c, e_o = -delta
    (1.0, 1.0, 1.0, 0.0, 0.0),                  # everything zero
]


def tie_table(rows=64):
    """-> (values, value_preds, returns, expected dvalues for mse, for huber), float32 [rows, 1] each; ``rows`` a power of
    two so that the mean's 1 / rows is exact.  Losses: clipped value loss, clip 0.25, delta 0.5, no normaliser,
    coefficient 1."""
    assert rows & (rows - 1) == 0 and rows >= 16
    t = torch.tensor(_TIES, dtype=torch.float64)
    t = t.repeat((rows + len(_TIES) - 1) // len(_TIES), 1)[:rows]
    col = lambda i: t[:, i:i + 1].float().contiguous()
    return col(0), col(1), col(2), (t[:, 3:4] / rows).float(), (t[:, 4:5] / rows).float()


def tie_autograd(use_huber, rows=64, dtype=torch.float32):
    """dL/dvalues of the tie table by autograd through ``torch_loss``'s value half."""
    v, vp, ret, _, _ = tie_table(rows)
    v = v.to(dtype).requires_grad_(True)
    one = torch.ones(rows, 1, dtype=dtype)
    lg = torch.zeros(rows, 1, dtype=dtype)
    _, _, vl, _ = torch_loss(lg, None, torch.zeros(rows, 1), torch.zeros(rows, 1, dtype=dtype), one, one, None, v,
                             vp.to(dtype), ret.to(dtype), None, clip=TIE_CLIP, huber_delta=TIE_DELTA, entropy_coef=0.0,
                             value_loss_coef=1.0, use_huber=use_huber, use_clipped=True, p_active=False, v_active=False)
    vl.backward()
    return v.grad


# ---------------------------------------------------------------------------------------------------- the judge
class Judge(object):
    """``check(name, mine, theirs, exact, floor)``: both float32 results against the float64 one, each on the tensor's
    max-abs scale (or the ``scale`` given); asserts e_mine <= 4 e_theirs + floor -- the margin the LayerNorm kernels are
    held to -- and keeps the worst figures per name.  With MAPPO_MARGINS_JSON set the figures are merged into that file
    when ``dump()`` is called (the record committed as profiles/small_kernel_margins.json)."""

    def __init__(self):
        self.seen = {}

    @staticmethod
    def errors(mine, theirs, exact, scale=None):
        exact = exact.double()
        scale = float(exact.abs().max()) + 1e-300 if scale is None else float(scale) + 1e-300
        e_mine = float((mine.double() - exact).abs().max()) / scale
        e_theirs = float((theirs.double() - exact).abs().max()) / scale
        return e_mine, e_theirs

    def check(self, name, mine, theirs, exact, floor, scale=None, what=""):
        e_mine, e_theirs = self.errors(mine, theirs, exact, scale)
        rec = self.seen.setdefault(name, {"kernel": 0.0, "torch32": 0.0, "floor": floor, "cases": 0,
                                          "worst_kernel_over_bound": 0.0, "by_case": {}})
        rec["kernel"], rec["torch32"] = max(rec["kernel"], e_mine), max(rec["torch32"], e_theirs)
        rec["cases"] += 1
        rec["worst_kernel_over_bound"] = max(rec["worst_kernel_over_bound"], e_mine / (4 * e_theirs + floor))
        case = rec["by_case"].setdefault(what.split(" flags=")[0], {"kernel": 0.0, "torch32": 0.0})     # (over its flag sets)
        case["kernel"], case["torch32"] = max(case["kernel"], e_mine), max(case["torch32"], e_theirs)
        print("judge %-28s %-40s kernel %.3e torch32 %.3e floor %.1e" % (name, what, e_mine, e_theirs, floor))
        assert e_mine == e_mine and e_mine <= 4 * e_theirs + floor, (name, what, e_mine, e_theirs, floor)

    def dump(self):
        path = os.environ.get("MAPPO_MARGINS_JSON")
        if not path or not self.seen:
            return
        doc = {}
        if os.path.exists(path):
            with open(path) as f:
                doc = json.load(f)
        doc["what"] = ("Small kernels (K6 row normalisation, K7 loss, K13 clip + Adam) against float64 on the MI355X: per comparison the largest error of "
                       "the kernel and of the same float32 torch expression (overall and per case), each relative to the tensor's scale (sums: to sum "
                       "|per-row term|), the floor of the assert e_kernel <= 4 e_torch32 + floor (about 3 x the largest kernel "
                       "error; never above the 1e-5 it began at) and the worst e_kernel / bound.  Written by "
                       "tests/test_gpu_fused_loss.py, tests/test_gpu_optim.py and tests/test_gpu_row_norm.py under MAPPO_MARGINS_JSON=<path>.  "
                       "k6.*: the LayerNorm kernels (y, mean, rstd, dx, dw, db, dpre), the standardising gather and the two standardisers of the "
                       "resident copies (slab, rows_ld), per kernel shape v<VEC>.l<LPR>.e<EPL> or width; k6.narrow.*: rows of at most 16 floats, "
                       "whose statistics are ill-conditioned in float32 whoever computes them; k6.*far.*: x = 100 + randn; k6.module: FusedLayerNorm "
                       "on a contiguous view off a 16-byte boundary.")
        for name, rec in self.seen.items():
            old = doc.get(name)
            if old is not None and old.get("floor") == rec["floor"]:
                cases = dict(old["by_case"])
                for k, c in rec["by_case"].items():
                    o = cases.get(k, c)
                    cases[k] = {"kernel": max(o["kernel"], c["kernel"]), "torch32": max(o["torch32"], c["torch32"])}
                rec = {"kernel": max(old["kernel"], rec["kernel"]), "torch32": max(old["torch32"], rec["torch32"]),
                       "floor": rec["floor"], "cases": old["cases"] + rec["cases"], "by_case": cases,
                       "worst_kernel_over_bound": max(old["worst_kernel_over_bound"], rec["worst_kernel_over_bound"])}
            doc[name] = rec
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
        self.seen = {}
