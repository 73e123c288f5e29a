"""Fused PPO loss (K7, ``mappo_ppo_loss_f32``): value and gradient of the clipped-surrogate loss for a
Discrete action head in one pass over a minibatch span, instead of ~100 elementwise / reduction launches
(reference r_mappo.py:52-89, :119-153).  The trainer feeds the gradients it returns straight into
``torch.autograd.backward`` at the head's logits and the critic's values.

Used when the policy has a single Categorical head and the tensors are on a HIP device; everything else
(continuous / mixed heads, CPU) takes the framework path in ``R_MAPPO.ppo_update``.  A MultiDiscrete head has its own
kernel (``mappo_ppo_loss_multi_f32``, all sub-heads in one launch), which ``R_MAPPO`` itself uses when asked to
(``MAPPO_FUSED_LOSS_MULTI=1`` or train_mpe.py's ``--fused_multi_loss``; the framework path otherwise).
``MAPPO_FUSED_LOSS=0`` disables both.
"""
import ctypes
import os

import torch

from onpolicy import _native

LOSS_MULTI_MAX_HEADS = _native.LOSS_MULTI_MAX_HEADS


def enabled():
    return os.environ.get("MAPPO_FUSED_LOSS", "1") != "0"


def multi_enabled(args=None):
    """The MultiDiscrete form of K7 is opt-in: ``MAPPO_FUSED_LOSS_MULTI=1`` or train_mpe.py's ``--fused_multi_loss``."""
    return os.environ.get("MAPPO_FUSED_LOSS_MULTI", "0") == "1" or bool(getattr(args, "fused_multi_loss", False))


def supported(policy, device, multi=False):
    """The fused loss takes this policy on this device: a Discrete head, or -- with ``multi`` -- a MultiDiscrete head within
    the limits of ``mappo_ppo_loss_multi_f32``."""
    act = getattr(getattr(policy, "actor", None), "act", None)
    if not (enabled() and torch.device(device).type == "cuda" and act is not None and hasattr(policy, "evaluate_logits")):
        return False
    kind = getattr(act, "action_type", None)
    if kind == "MultiDiscrete":
        sizes = act.head_sizes
        return multi and 0 < len(sizes) <= LOSS_MULTI_MAX_HEADS and min(sizes) >= 1 and sum(sizes) <= 64
    return kind == "Discrete"


def _flat(x):
    return None if x is None else x.detach().reshape(-1).contiguous()


def ppo_loss(logits, available_actions, actions, old_logp, adv, active, factor, values, value_preds, returns,
             norm, inv_denoms, sums, *, clip, huber_delta, entropy_coef, value_loss_coef, use_huber,
             use_clipped_value_loss, policy_active_masks, value_active_masks, need_actor=True):
    """-> (dlogits or None, dvalues).  ``sums`` (float64[4], device) accumulates
    {sum w_p * (-surrogate), sum w_p * entropy, sum w_v * value_loss, sum ratio}."""
    rows, na = logits.shape
    lg = logits.detach().contiguous()
    dlogits = torch.empty_like(lg) if need_actor else None
    v = _flat(values)
    dvalues = torch.empty_like(v)
    avail = None if available_actions is None else available_actions.detach().contiguous()
    keep = [lg, avail, _flat(actions), _flat(old_logp), _flat(adv), _flat(active), _flat(factor), v,
            _flat(value_preds), _flat(returns), norm, inv_denoms]
    p = _native.ptr
    a = _native.PPOLoss(*[p(t) for t in keep], p(dlogits), p(dvalues), p(sums), rows, na, float(clip),
                        float(huber_delta), float(entropy_coef), float(value_loss_coef),
                        (_native.LOSS_HUBER if use_huber else 0)
                        | (_native.LOSS_CLIPPED_VALUE if use_clipped_value_loss else 0)
                        | (_native.LOSS_POLICY_ACTIVE_MASKS if policy_active_masks else 0)
                        | (_native.LOSS_VALUE_ACTIVE_MASKS if value_active_masks else 0))
    _native.check(_native.lib().mappo_ppo_loss_f32(a, _native.stream_of(lg.device)), "mappo_ppo_loss_f32")
    return dlogits, dvalues.view_as(values)


def ppo_loss_multi(logits, head_sizes, actions, old_logp, adv, active, values, value_preds, returns, norm, inv_denoms,
                   sums, *, clip, huber_delta, entropy_coef, value_loss_coef, use_huber, use_clipped_value_loss,
                   policy_active_masks, value_active_masks):
    """K7 for a MultiDiscrete head (``mappo_ppo_loss_multi_f32``) -> (dlogits, dvalues).  ``logits`` [rows, sum head_sizes]
    holds the sub-heads' logits side by side, ``actions`` / ``old_logp`` are [rows, len(head_sizes)].  ``sums`` accumulates
    {sum w_p * (-sum_h surrogate_h), sum w_p * mean_h entropy_h, sum w_v * value_loss, sum mean_h ratio_h}."""
    rows, width = logits.shape
    k = len(head_sizes)
    assert width == sum(head_sizes) and tuple(actions.shape) == (rows, k) and tuple(old_logp.shape) == (rows, k)
    lg = logits.detach().contiguous()
    dlogits = torch.empty_like(lg)
    v = _flat(values)
    dvalues = torch.empty_like(v)
    keep = [lg, _flat(actions), _flat(old_logp), _flat(adv), _flat(active), v, _flat(value_preds), _flat(returns), norm,
            inv_denoms]
    p = _native.ptr
    sizes = (ctypes.c_int * LOSS_MULTI_MAX_HEADS)(*[int(n) for n in head_sizes])
    a = _native.PPOLossMulti(*[p(t) for t in keep], p(dlogits), p(dvalues), p(sums), rows, k, sizes, float(clip),
                             float(huber_delta), float(entropy_coef), float(value_loss_coef),
                             (_native.LOSS_HUBER if use_huber else 0)
                             | (_native.LOSS_CLIPPED_VALUE if use_clipped_value_loss else 0)
                             | (_native.LOSS_POLICY_ACTIVE_MASKS if policy_active_masks else 0)
                             | (_native.LOSS_VALUE_ACTIVE_MASKS if value_active_masks else 0))
    _native.check(_native.lib().mappo_ppo_loss_multi_f32(a, _native.stream_of(lg.device)), "mappo_ppo_loss_multi_f32")
    return dlogits, dvalues.view_as(values)


def sample_supported(logits):
    """K14 takes this head's rollout sampling: float32 HIP logits of <= 64 actions, device-sampling mode, no autograd."""
    from . import distributions
    return (os.environ.get("MAPPO_FUSED_SAMPLE", "1") != "0" and torch.is_tensor(logits) and logits.is_cuda
            and logits.dtype == torch.float32 and logits.dim() == 2 and 0 < logits.shape[1] <= 64
            and not torch.is_grad_enabled() and distributions.SAMPLING_RNG == "device")


def sample_categorical(logits, available_actions=None):
    """(actions [rows, 1] int64, log-probs [rows, 1]) of one draw per row from softmax(masked logits)
    (``mappo_categorical_sample``, K14): what ``Categorical.forward`` -> ``FixedCategorical.sample`` / ``log_probs`` give
    (reference distributions.py:14-28, :55-68) as two launches -- the Exponential(1) noise from torch's generator and the
    kernel -- instead of ~15."""
    rows, na = logits.shape
    lg = logits.detach().contiguous()
    avail = None if available_actions is None else available_actions.detach().to(torch.float32).contiguous()
    noise = torch.empty_like(lg).exponential_(1.0)
    actions = torch.empty((rows, 1), dtype=torch.int64, device=lg.device)
    logp = torch.empty((rows, 1), dtype=torch.float32, device=lg.device)
    p = _native.ptr
    _native.check(_native.lib().mappo_categorical_sample(p(lg), p(avail), p(noise), p(actions), p(logp), rows, na,
                                                         _native.stream_of(lg.device)), "mappo_categorical_sample")
    return actions, logp


MULTI_SAMPLE_MAX_HEADS = 8


def multi_sample_supported(x, head_sizes):
    """The MultiDiscrete form of K14 takes this head's rollout sampling: float32 HIP features, at most 8 sub-heads of
    <= 64 actions in all, device-sampling mode, no autograd (``MAPPO_FUSED_SAMPLE=0`` disables it, as for K14)."""
    from . import distributions
    return (os.environ.get("MAPPO_FUSED_SAMPLE", "1") != "0" and torch.is_tensor(x) and x.is_cuda
            and x.dtype == torch.float32 and x.dim() == 2 and 0 < len(head_sizes) <= MULTI_SAMPLE_MAX_HEADS
            and sum(head_sizes) <= 64 and not torch.is_grad_enabled() and distributions.SAMPLING_RNG == "device")


def sample_multi_categorical(logits, head_sizes):
    """(actions [rows, k] int64, log-probs [rows, k]) of one draw per row and sub-head from the sub-heads' logits laid side
    by side in ``logits`` [rows, sum head_sizes] (``mappo_multi_categorical_sample``): what ACTLayer.forward's
    multi-discrete branch gives with one FixedCategorical per sub-head.  The Exponential(1) noise is drawn per sub-head in
    head order, as the framework's per-head torch.multinomial(p, 1) draws it, so both paths consume the same stream."""
    rows = logits.shape[0]
    k = len(head_sizes)
    lg = logits.detach().contiguous()
    noise = [torch.empty((rows, int(n)), dtype=torch.float32, device=lg.device).exponential_(1.0) for n in head_sizes]
    actions = torch.empty((rows, k), dtype=torch.int64, device=lg.device)
    logp = torch.empty((rows, k), dtype=torch.float32, device=lg.device)
    p = _native.ptr
    noise_ptrs = (ctypes.c_void_p * k)(*[p(q) for q in noise])
    sizes = (ctypes.c_int * k)(*[int(n) for n in head_sizes])
    _native.check(_native.lib().mappo_multi_categorical_sample(p(lg), noise_ptrs, sizes, k, p(actions), p(logp), rows,
                                                               _native.stream_of(lg.device)),
                  "mappo_multi_categorical_sample")
    return actions, logp


def mode_supported(logits_or_x, head_sizes=None):
    """The mode form of K14 takes this head's deterministic action: the conditions of ``sample_supported`` (a Discrete
    head's logits) or, with ``head_sizes``, of ``multi_sample_supported`` (a MultiDiscrete head's features), without the
    sampling-generator one -- the mode draws nothing.  ``MAPPO_FUSED_SAMPLE=0`` disables it with the samplers."""
    x = logits_or_x
    if not (os.environ.get("MAPPO_FUSED_SAMPLE", "1") != "0" and torch.is_tensor(x) and x.is_cuda
            and x.dtype == torch.float32 and x.dim() == 2 and not torch.is_grad_enabled()):
        return False
    if head_sizes is None:
        return 0 < x.shape[1] <= 64
    return 0 < len(head_sizes) <= MULTI_SAMPLE_MAX_HEADS and sum(head_sizes) <= 64


def mode_categorical(logits, available_actions=None):
    """(actions [rows, 1] int64, log-probs [rows, 1]) of the most probable action per row of softmax(masked logits)
    (``mappo_categorical_mode``, K14 mode): what ``Categorical.forward`` -> ``FixedCategorical.mode`` / ``log_probs``
    give (reference distributions.py:14-28, :55-68) as one launch; of equal maxima the lowest index."""
    rows, na = logits.shape
    lg = logits.detach().contiguous()
    avail = None if available_actions is None else available_actions.detach().to(torch.float32).contiguous()
    assert avail is None or (avail.shape == lg.shape and avail.device == lg.device)
    actions = torch.empty((rows, 1), dtype=torch.int64, device=lg.device)
    logp = torch.empty((rows, 1), dtype=torch.float32, device=lg.device)
    p = _native.ptr
    _native.check(_native.lib().mappo_categorical_mode(p(lg), p(avail), p(actions), p(logp), rows, na,
                                                       _native.stream_of(lg.device)), "mappo_categorical_mode")
    return actions, logp


def mode_multi_categorical(logits, head_sizes):
    """(actions [rows, k] int64, log-probs [rows, k]) of every sub-head's most probable action from the sub-heads' logits
    laid side by side in ``logits`` [rows, sum head_sizes] (``mappo_multi_categorical_mode``): what ACTLayer.forward's
    multi-discrete branch gives with ``deterministic=True`` (reference act.py:44-60), as one launch."""
    rows = logits.shape[0]
    k = len(head_sizes)
    assert logits.shape[1] == sum(head_sizes)
    lg = logits.detach().contiguous()
    actions = torch.empty((rows, k), dtype=torch.int64, device=lg.device)
    logp = torch.empty((rows, k), dtype=torch.float32, device=lg.device)
    p = _native.ptr
    sizes = (ctypes.c_int * k)(*[int(n) for n in head_sizes])
    _native.check(_native.lib().mappo_multi_categorical_mode(p(lg), sizes, k, p(actions), p(logp), rows,
                                                             _native.stream_of(lg.device)),
                  "mappo_multi_categorical_mode")
    return actions, logp
