"""-m gpu: the mode form of K14 (``mappo_categorical_mode`` / ``mappo_multi_categorical_mode``): the deterministic action
of Categorical heads in one launch.  Actions against ``numpy.argmax`` on the masked float32 logits (exact: first maximum,
no tolerance), log-probs against float64 log-softmax at the chosen action (the sampler tests' bounds), the edges (ties,
one action left, nothing left), MultiDiscrete heads per head, the framework path (``FixedCategorical.mode`` /
``log_probs``), and the route from ``policy.act(deterministic=True)``.

Log-probs and the framework.  The kernel forms log p = -log(sum exp(x - max)); the framework forms x - (max + log(sum)),
whose float32 sum rounds at the size of the maximum.  At logits x 2 the framework is itself within rtol 1e-5 / atol 1e-6 of
float64 on every row (asserted), and the kernel has to agree with it within those bounds.  At logits x 30 that rounding
alone puts the FRAMEWORK up to 3.9e-6 from float64 (|max| ~ 100: a third of the rows at 64 actions are outside the bounds),
so there it is no yardstick at these bounds: the kernel is held to float64 within the bounds on every row
(``test_mode_kernel_is_exact_argmax`` as well), and to the framework within the bounds plus the framework's own measured
distance from float64 on that row.  Measured on the MI355X at x 30: framework up to 3.9e-6 from float64, kernel up to
2.4e-7 (5.9e-7 over all cases: profiles/small_kernel_margins.json, ``k14mode.*``).
"""
import json
import os

import numpy as np
import pytest
import torch

from helpers import Box, Discrete, make_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RTOL, ATOL = 1e-5, 1e-6             # the sampler test's bounds (test_gpu_fused_loss.py): the arithmetic is the same
NEAR_TIE = 1e-5                     # the project's near-tie bound from the sampler tests
SIZES = (1, 2, 5, 64)
ROWS = (1, 255, 256, 257, 4099)     # around the 256-thread block edge, and several blocks
MARGINS = {}


def _note(name, err, bound, fw_err=None):
    rec = MARGINS.setdefault(name, {"kernel": 0.0, "torch32": 0.0, "bound": "rtol %g atol %g vs float64" % (RTOL, ATOL),
                                    "cases": 0, "worst_kernel_over_bound": 0.0})
    rec["kernel"] = max(rec["kernel"], float(err.max()))
    rec["worst_kernel_over_bound"] = max(rec["worst_kernel_over_bound"], float((err / bound).max()))
    rec["cases"] += 1
    if fw_err is not None:
        rec["torch32"] = max(rec["torch32"], float(fw_err.max()))


@pytest.fixture(autouse=True, scope="module")
def _record_margins():
    yield
    path = os.environ.get("MAPPO_MARGINS_JSON")
    if not path or not MARGINS:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(MARGINS)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


_INPUTS = {}


def inputs(rows, na, masked, scale):
    """(logits, avail or None, masked float32 logits on the host, float64 log-softmax of them): made once per case."""
    key = (rows, na, masked, scale)
    if key not in _INPUTS:
        g = torch.Generator(device=DEV).manual_seed(1000 * na + rows + (7 if masked else 0) + int(scale))
        logits = torch.randn(rows, na, device=DEV, generator=g) * scale
        avail = None
        if masked:
            avail = (torch.rand(rows, na, device=DEV, generator=g) < 0.7).float()
            avail[:, 0] = 1.0
        x = logits if avail is None else torch.where(avail == 0, torch.full_like(logits, -1e10), logits)
        x64 = x.double().cpu()
        _INPUTS[key] = logits, avail, x.cpu().numpy(), x64 - x64.logsumexp(-1, keepdim=True)
    return _INPUTS[key]


def _mode(logits, avail=None):
    from onpolicy.algorithms.utils import fused_loss
    with torch.no_grad():
        assert fused_loss.mode_supported(logits)
        a, l = fused_loss.mode_categorical(logits, avail)
    rows = logits.shape[0]
    assert a.shape == (rows, 1) and a.dtype == torch.int64 and l.shape == (rows, 1) and l.dtype == torch.float32
    return a.cpu(), l.cpu()


def _judge_logp(name, logp, l64, actions, fw=None):
    exact = l64.gather(-1, actions)
    err = (logp.double() - exact).abs()
    bound = ATOL + RTOL * exact.abs()
    fw_err = None if fw is None else (fw.double() - exact).abs()
    _note(name, err, bound, fw_err)
    print("%s: max |kernel - float64| %.3e, worst error / bound %.3f" % (name, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all()), (name, float(err.max()), float((err / bound).max()))
    return exact, bound


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("na", SIZES)
def test_mode_kernel_is_exact_argmax(na, rows):
    for masked in (False, True):
        for scale in (2.0, 30.0):
            logits, avail, x, l64 = inputs(rows, na, masked, scale)
            a, l = _mode(logits, avail)
            np.testing.assert_array_equal(a.numpy()[:, 0], np.argmax(x, -1))         # first maximum, float32 compare
            _judge_logp("k14mode.logp", l, l64, a)
            if masked:
                assert bool((avail.cpu().gather(-1, a) == 1).all())                  # never an unavailable action


def test_mode_kernel_edges():
    rows, na = 300, 7
    g = torch.Generator(device=DEV).manual_seed(5)
    logits = torch.randn(rows, na, device=DEV, generator=g) * 2
    # exact ties: the maximum at two positions (3 and 5), and at all positions
    two = logits.clone()
    top = two.max(-1).values + 1.0
    two[:, 3] = top
    two[:, 5] = top
    a, l = _mode(two)
    assert bool((a == 3).all())
    a, l = _mode(torch.full((rows, na), 0.75, device=DEV))
    assert bool((a == 0).all())
    torch.testing.assert_close(l, torch.full((rows, 1), -float(np.log(na))), rtol=RTOL, atol=ATOL)
    # only the last action left: that action, log-prob exactly 0
    avail = torch.zeros(rows, na, device=DEV)
    avail[:, -1] = 1.0
    a, l = _mode(logits, avail)
    assert bool((a == na - 1).all()) and bool((l == 0.0).all())
    # action 0 unavailable (its logit the largest by far): never chosen
    big = logits.clone()
    big[:, 0] = 50.0
    avail = (torch.rand(rows, na, device=DEV, generator=g) < 0.7).float()
    avail[:, 0] = 0.0
    avail[:, 2] = 1.0
    a, l = _mode(big, avail)
    assert bool((a != 0).all()) and bool((avail.cpu().gather(-1, a) == 1).all())
    x = torch.where(avail == 0, torch.full_like(big, -1e10), big).cpu().numpy()
    np.testing.assert_array_equal(a.numpy()[:, 0], np.argmax(x, -1))
    # nothing available: every masked logit is -1e10, the first wins
    a, l = _mode(logits, torch.zeros(rows, na, device=DEV))
    assert bool((a == 0).all())
    torch.testing.assert_close(l, torch.full((rows, 1), -float(np.log(na))), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("sizes", [(5, 10), (1, 2), (8,) * 8, (64,)], ids=lambda s: "x".join(map(str, s)))
def test_multi_mode_kernel_per_head(sizes):
    from onpolicy.algorithms.utils import fused_loss
    sizes = list(sizes)
    for rows in (257, 4099):
        for scale in (2.0, 30.0):
            g = torch.Generator(device=DEV).manual_seed(sum(sizes) + rows + int(scale))
            logits = torch.randn(rows, sum(sizes), device=DEV, generator=g) * scale
            with torch.no_grad():
                assert fused_loss.mode_supported(logits, sizes)
                a, l = fused_loss.mode_multi_categorical(logits, sizes)
            assert a.shape == (rows, len(sizes)) and a.dtype == torch.int64 and l.shape == (rows, len(sizes))
            a, l = a.cpu(), l.cpu()
            for k, part in enumerate(logits.cpu().split(sizes, -1)):
                np.testing.assert_array_equal(a[:, k].numpy(), np.argmax(part.numpy(), -1))
                x64 = part.double()
                _judge_logp("k14mode.multi.logp", l[:, k:k + 1], x64 - x64.logsumexp(-1, keepdim=True), a[:, k:k + 1])
            if sizes == [64]:           # one head of 64: the single-head entry point, bit for bit
                a1, l1 = _mode(logits)
                assert torch.equal(a, a1) and torch.equal(l, l1)


@pytest.mark.parametrize("na", SIZES)
def test_mode_kernel_against_the_framework_path(na):
    from onpolicy.algorithms.utils.distributions import FixedCategorical
    rows = 4099
    for masked in (False, True):
        for scale in (2.0, 30.0):
            logits, avail, x, l64 = inputs(rows, na, masked, scale)
            a, l = _mode(logits, avail)
            with torch.no_grad():
                xm = logits if avail is None else torch.where(avail == 0, torch.full_like(logits, -1e10), logits)
                dist = FixedCategorical(logits=xm)
                fa = dist.mode()
                fl = dist.log_probs(fa).cpu()
                fa = fa.cpu()
            assert fa.shape == a.shape and fa.dtype == a.dtype and fl.shape == l.shape
            # the framework path itself against the exact argmax on these seeds
            assert int((fa.numpy()[:, 0] != np.argmax(x, -1)).sum()) <= 2
            differ = (a != fa)[:, 0]
            x64 = torch.from_numpy(x).double()
            gap = (x64.gather(-1, a) - x64.gather(-1, fa)).abs()[:, 0]
            assert bool((gap[differ] <= NEAR_TIE).all()) and int(differ.sum()) <= 2, (int(differ.sum()), gap[differ])
            # log-probs, where both chose the same action (module docstring)
            same = ~differ
            exact = l64.gather(-1, a)[same]
            bound = ATOL + RTOL * exact.abs()
            fw_err = (fl[same].double() - exact).abs()
            valid = fw_err <= bound                      # the framework's value is itself within the bounds of float64
            k_fw = (l[same].double() - fl[same].double()).abs()
            k_64 = (l[same].double() - exact).abs()
            print("na %d masked %d x%g: framework within the bounds of float64 on %d of %d rows (its max error %.3e); "
                  "kernel vs framework max %.3e, kernel vs float64 max %.3e"
                  % (na, masked, scale, int(valid.sum()), int(same.sum()), float(fw_err.max()), float(k_fw.max()),
                     float(k_64.max())))
            assert bool((k_64 <= bound).all())           # the kernel against float64: every row, both scales
            if scale == 2.0:
                assert bool(valid.all())                 # at ordinary logits the framework is a yardstick on every row
                assert bool((k_fw <= bound).all())
            else:                                        # (module docstring) the framework's own error on the row is added
                assert bool((k_fw <= bound + fw_err).all())
            _note("k14mode.logp", k_64, bound, fw_err)


def _multi_discrete():
    from onpolicy.utils.multi_discrete import MultiDiscrete
    return MultiDiscrete([[0, 4], [0, 9]])


@pytest.mark.parametrize("kind,recurrent", [("discrete", False), ("discrete", True), ("multidiscrete", False)])
def test_policy_act_routes_the_deterministic_action_to_the_kernel(kind, recurrent):
    """``R_MAPPOPolicy`` built with ``use_device_eval`` runs the mode entry point in ``act(deterministic=True)`` -- a
    Discrete head behind the fused trunk + head launch (K9) or behind the GRU, a MultiDiscrete (5, 10) head -- and one
    built without it does not; both choose the same actions."""
    from onpolicy import _native
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from onpolicy.algorithms.utils import distributions
    distributions.set_sampling_rng("device")
    space = Discrete(5) if kind == "discrete" else _multi_discrete()
    symbol = "mappo_categorical_mode" if kind == "discrete" else "mappo_multi_categorical_mode"
    rows = 513
    g = torch.Generator(device=DEV).manual_seed(2)
    obs = torch.randn(rows, 18, device=DEV, generator=g)
    rnn = torch.zeros(rows, 1, 64, device=DEV)
    masks = torch.ones(rows, 1, device=DEV)
    out = {}
    for flag in (True, False):
        args = make_args(hidden_size=64, use_recurrent_policy=recurrent)
        if flag:
            args.use_device_eval = True
        torch.manual_seed(1)
        policy = R_MAPPOPolicy(args, Box((18,)), Box((54,)), space, device=DEV)
        policy.actor.eval()
        assert policy.actor.act.fused_mode is flag
        _native.count_calls(True)
        try:
            with torch.no_grad():
                before = torch.cuda.get_rng_state(DEV)
                a, h = policy.act(obs, rnn, masks, deterministic=True)
                assert torch.equal(before, torch.cuda.get_rng_state(DEV))       # the mode draws nothing
                sampled, _ = policy.act(obs, rnn, masks)                        # sampling keeps its own kernels
            calls = _native.calls()
        finally:
            _native.count_calls(False)
        assert calls.get(symbol, 0) == (1 if flag else 0), calls
        assert calls.get("mappo_categorical_mode", 0) + calls.get("mappo_multi_categorical_mode", 0) == (1 if flag else 0)
        if kind == "discrete" and not recurrent and flag:
            assert calls.get("mappo_mlp_forward", 0) > 0, calls                 # the K9 trunk + head route
        assert a.dtype == torch.int64 and a.shape == (rows, 1 if kind == "discrete" else 2)
        out[flag] = a.cpu()
    assert (out[True] == out[False]).float().mean() >= 0.999
