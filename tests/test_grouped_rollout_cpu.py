"""No GPU: K19's entry points refuse bad descriptors by return code, the ctypes descriptor is the header's struct, the
grouped route is off unless asked for and names what it leaves to the per-agent body."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT
from helpers import Box, Discrete, make_args
from onpolicy import _native
from onpolicy.algorithms.utils import grouped_rollout


def _net(**over):
    """A descriptor the checks accept (host memory stands in: validation returns before anything touches the device)."""
    buf = (ctypes.c_float * 64)()
    at = ctypes.addressof(buf)
    d = _native.GroupedNet(src=at, ld=40, col=3, din=17, n_layers=2, act=1, out=5, hidden=64, ln_eps=1e-5, w1=at, wh=at, bh=at,
                           y=at, noise=at, actions=at, logp=at)
    for l in range(2):
        d.bias[l], d.ln_g[l], d.ln_b[l] = at, at, at
    d.w2[0] = at
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d, buf


@pytest.mark.parametrize("over,code", [
    (dict(src=None), -1), (dict(w1=None), -1), (dict(bh=None), -1), (dict(w2=(0, None)), -1), (dict(ln_b=(1, None)), -1),
    (dict(in_g=1024), -1),                                  # an input LayerNorm's weight without its bias
    (dict(logp=None), -1),                                  # an actor without somewhere to put its log-probabilities
    (dict(noise=None, actions=None, logp=None, y=None), -1),    # a critic without y
    (dict(out=0), -2), (dict(out=33), -2), (dict(n_layers=1), -2), (dict(n_layers=4), -2), (dict(hidden=128), -2),
    (dict(din=0), -2), (dict(din=16385, ld=20000), -2), (dict(col=-1), -2), (dict(ld=19), -2), (dict(ln_eps=0.0), -2),
    (dict(act=0), -3), (dict(act=3), -3), (dict(src=1026), -5)])
def test_prepare_refuses_bad_descriptors(over, code):
    table, (good, keep), (bad, keep2) = (ctypes.c_double * 64)(), _net(), _net(**over)
    assert _native.lib().mappo_grouped_prepare((_native.GroupedNet * 2)(good, bad), 2, ctypes.addressof(table)) == code


def test_entry_points_refuse_bad_calls():
    lib, keep = _native.lib(), (ctypes.c_double * 64)()
    nets, table = (_native.GroupedNet * 1)(_net()[0]), ctypes.addressof(keep)
    assert lib.mappo_grouped_prepare(None, 1, table) == -1 and lib.mappo_grouped_prepare(nets, 1, None) == -1
    assert lib.mappo_grouped_prepare(nets, 0, table) == -2 and lib.mappo_grouped_prepare(nets, 129, table) == -2
    assert lib.mappo_grouped_forward(None, 1, 8, None) == -1
    for G, rows in ((0, 8), (129, 8), (1, 0), (1, -3)):
        assert lib.mappo_grouped_forward(table, G, rows, None) == -2
    assert lib.mappo_grouped_table_bytes(128) == 128 * ctypes.sizeof(_native.GroupedNet) and lib.mappo_grouped_table_bytes(0) == 0


def test_descriptor_layout_matches_the_header():
    src = open(ROOT + "/include/mappo_hip.h").read()
    body = src[src.index("typedef struct mappo_grouped_net {"):src.index("} mappo_grouped_net_t;")]
    declared = [n for line in re.findall(r"^\s+(?:const )?\w+\*? ([^;]+);", body, flags=re.M)
                for n in re.sub(r"\[[^\]]*\]", "", line).split(", ")]
    assert declared == [name for name, _ in _native.GroupedNet._fields_]
    assert ctypes.sizeof(_native.GroupedNet) == 208 and _native.GroupedNet.in_g.offset == 48
    limits = {k: int(v) for k, v in re.findall(r"#define MAPPO_GROUPED_MAX_(\w+)\s+(\d+)", src)}
    assert limits == dict(NETS=_native.GROUPED_MAX_NETS, DIN=_native.GROUPED_MAX_DIN, OUT=_native.GROUPED_MAX_OUT)
    assert limits["DIN"] >= 16384


def _policies(action_space=None, n=2, **kw):
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    args = make_args(**kw)
    return [R_MAPPOPolicy(args, Box((6,)), Box((12,)), action_space or Discrete(5)) for _ in range(n)]


@pytest.mark.parametrize("kw,word", [
    (dict(use_recurrent_policy=True), "recurrent"), (dict(action_space="multi"), "MultiDiscrete"),
    (dict(hidden_size=128), "hidden size 64"), (dict(use_popart=True, use_valuenorm=False), "PopArt"),
    (dict(layer_N=3), "layer_N"), (dict(host_rng=True), "host sampling"), (dict(available_actions=True), "available_actions"),
    (dict(), "HIP device")])
def test_route_names_what_it_refuses(kw, word, monkeypatch):
    """Every refusal leaves the per-agent body to run (``build`` returns None); policies the kernel would take are
    refused here only for living on the CPU."""
    from onpolicy.algorithms.utils import distributions
    from onpolicy.utils.multi_discrete import MultiDiscrete
    kw = dict(kw)
    if kw.pop("host_rng", False):
        monkeypatch.setattr(distributions, "SAMPLING_RNG", "host")
    avail = kw.pop("available_actions", False)
    policies = _policies(MultiDiscrete([[0, 2], [0, 4]]) if kw.pop("action_space", None) else None, **kw)
    why = grouped_rollout.refusal(policies, avail)
    assert why is not None and word in why, why

    class Worlds(object):
        obs_dims = (6, 6)
    assert grouped_rollout.build(policies, Worlds(), torch.zeros(4, 12), True, avail) is None


def test_route_is_off_by_default(monkeypatch):
    monkeypatch.delenv("MAPPO_GROUPED_ROLLOUT", raising=False)
    assert not grouped_rollout.enabled()
    monkeypatch.setenv("MAPPO_GROUPED_ROLLOUT", "1")
    assert grouped_rollout.enabled()
