"""The MultiDiscrete form of the fused PPO loss (``mappo_ppo_loss_multi_f32``) without a device: the float64 reference of
its device tests (tests/loss_reference_multi.py) against the framework path it replaces -- ``ACTLayer.evaluate_actions``
and the formulas of ``R_MAPPO._framework_span`` / ``_value_loss``, which the fixtures of test_action_spaces_cpu.py tie to
the reference's own code -- the entry point's argument checks, and the route staying off on the CPU."""
import ctypes

import pytest
import torch

import loss_reference as lr
import loss_reference_multi as lrm
from helpers import Box, make_args
from test_misc_cpu import _MultiDiscrete

# (a dyadic huber knee: utils/util.py huber_loss multiplies a float32 indicator by delta first, as the reference does, so in a
# float64 evaluation a delta like 0.8 enters rounded to float32 -- 1.5e-8 off the helper's, which is not what is compared here)
HP = dict(clip=0.2, huber_delta=0.75, entropy_coef=0.01, value_loss_coef=1.3)


def _trainer(head_sizes, fused_multi_loss=None):
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from onpolicy.algorithms.r_mappo.r_mappo import R_MAPPO
    args = make_args(hidden_size=16, use_valuenorm=False, use_popart=False, clip_param=HP["clip"],
                     huber_delta=HP["huber_delta"], entropy_coef=HP["entropy_coef"],
                     value_loss_coef=HP["value_loss_coef"])
    if fused_multi_loss is not None:        # train_mpe.py's own flag, not one of config.py's
        args.fused_multi_loss = fused_multi_loss
    torch.manual_seed(3)
    policy = R_MAPPOPolicy(args, Box((7,)), Box((9,)), _MultiDiscrete(list(head_sizes)))
    return R_MAPPO(args, policy), policy


@pytest.mark.parametrize("head_sizes", [(3, 4), (5, 10)])
@pytest.mark.parametrize("flags", [0, 5, 10, 15])
def test_float64_reference_is_the_framework_path(head_sizes, flags):
    """The four logged means and the gradients -- at the action head's input and parameters and at the values -- of the
    helper's expression and of the framework path agree to 1e-12 relative in float64."""
    rows = 257
    trainer, policy = _trainer(head_sizes)
    kw = lr.flag_kwargs(flags)
    trainer._use_huber_loss, trainer._use_clipped_value_loss = kw["use_huber"], kw["use_clipped"]
    trainer._use_policy_active_masks, trainer._use_value_active_masks = kw["p_active"], kw["v_active"]
    act = policy.actor.act.double()
    d = lr.to(lrm.make_inputs(rows, head_sizes, seed=4), dtype=torch.float64)
    feats = torch.randn(rows, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    # the head's own logits instead of the generated ones: actions and old log-probs stay as drawn (any ratio will do)
    results = []
    for which in ("helper", "framework"):
        act.zero_grad()
        x = feats.clone().requires_grad_(True)
        values = d["values"].clone().requires_grad_(True)
        if which == "helper":
            pl, ent, vl, ratio = lrm.torch_loss(act.multi_logits(x), head_sizes, d["actions"], d["old_logp"], d["adv"],
                                                d["active"], values, d["value_preds"], d["returns"], None, **kw, **HP)
        else:
            logp, ent = act.evaluate_actions(x, d["actions"], None, d["active"] if kw["p_active"] else None)
            ratio = trainer._ratio(logp, d["old_logp"])
            surr = torch.min(ratio * d["adv"], torch.clamp(ratio, 1.0 - HP["clip"], 1.0 + HP["clip"]) * d["adv"])
            per = -torch.sum(surr, dim=-1, keepdim=True)
            pl = (per * d["active"]).sum() / d["active"].sum() if kw["p_active"] else per.mean()
            vl = trainer._value_loss(values, d["value_preds"], d["returns"], d["active"], update_normalizer=False)
        (pl - ent * HP["entropy_coef"]).backward()
        (vl * HP["value_loss_coef"]).backward()
        results.append([pl.detach(), ent.detach(), vl.detach(), ratio.detach().mean(), x.grad, values.grad] +
                       [p.grad.clone() for p in act.parameters()])
    assert len(results[0]) == 6 + 2 * len(head_sizes)
    for a, b in zip(*results):
        assert a.dtype == torch.float64 and b.dtype == torch.float64
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))


def _args(**over):
    """A well-formed argument struct (host memory: nothing is launched by a rejected call) -> (struct, what it points to)."""
    from onpolicy import _native
    rows, sizes = 4, over.pop("sizes", [5, 10])
    width, k = sum(sizes), len(sizes)
    keep = {n: torch.zeros(max(1, rows * max(width, k, 1))) for n, _ in _native.PPOLossMulti._fields_[:13]}
    keep["sums"] = torch.zeros(4, dtype=torch.float64)
    padded = (list(sizes) + [0] * _native.LOSS_MULTI_MAX_HEADS)[:_native.LOSS_MULTI_MAX_HEADS]
    a = _native.PPOLossMulti(*[keep[n].data_ptr() for n, _ in _native.PPOLossMulti._fields_[:13]], rows,
                             over.pop("num_heads", k), (ctypes.c_int * _native.LOSS_MULTI_MAX_HEADS)(*padded),
                             0.2, 10.0, 0.01, 1.0, 15)
    for name, value in over.items():
        setattr(a, name, value)
    return a, keep


def test_multi_loss_rejects_bad_arguments():
    from onpolicy import _native
    lib = _native.lib()
    call = lambda **over: lib.mappo_ppo_loss_multi_f32(ctypes.byref(_args(**over)[0]), None)      # noqa: E731
    assert ctypes.sizeof(_native.PPOLossMulti) == 13 * 8 + 8 + 4 + 8 * 4 + 4 * 4 + 4
    assert lib.mappo_ppo_loss_multi_f32(None, None) == -1                                   # NULL struct
    assert lib.mappo_ppo_loss_multi_f32(ctypes.byref(_native.PPOLossMulti()), None) == -1   # every column NULL
    for name in ("logits", "actions", "old_logp", "adv", "values", "value_preds", "returns", "inv_denoms", "dlogits",
                 "dvalues", "sums"):
        assert call(**{name: None}) == -1, name
    assert call(sizes=[], num_heads=0) == -2                    # k = 0
    assert call(sizes=[2] * 8, num_heads=9) == -2               # k = 9
    assert call(sizes=[5, 0]) == -2                             # a size of 0
    assert call(sizes=[5, -1]) == -2
    assert call(sizes=[33, 32]) == -2                           # S = 65
    assert call(sizes=[65]) == -2
    assert call(rows=0) == -2
    assert call(flags=16) == -3                                 # an unknown flag bit
    assert call(flags=1 << 31) == -3


@pytest.mark.parametrize("env", [None, "1"])
def test_multidiscrete_trainer_on_the_cpu_stays_on_the_framework_path(monkeypatch, env):
    from onpolicy.algorithms.utils import fused_loss
    if env is None:
        monkeypatch.delenv("MAPPO_FUSED_LOSS_MULTI", raising=False)
    else:
        monkeypatch.setenv("MAPPO_FUSED_LOSS_MULTI", env)
    assert fused_loss.multi_enabled() == (env == "1")
    trainer, policy = _trainer((5, 10))
    assert policy.actor.act.multi_discrete and trainer._fused_loss is False
    trainer, _ = _trainer((5, 10), fused_multi_loss=True)       # (train_mpe.py's flag: the same on the CPU)
    assert trainer._fused_loss is False
