"""No GPU: the recurrent K19 entry points refuse bad descriptors by return code, the ctypes descriptor is the header's struct,
the recurrent grouped route needs both switches and names what it leaves to the per-agent body."""
import ctypes
import re

import pytest

from conftest import ROOT
from helpers import Box, Discrete, make_args
from onpolicy import _native
from onpolicy.algorithms.utils import grouped_rollout

NEW = ("h_in", "mask", "h_out", "w_ih", "w_hh", "b_ih", "b_hh", "rnn_g", "rnn_b")


def _net(**over):
    """A descriptor the checks accept (host memory stands in: validation returns before anything touches the device)."""
    buf = (ctypes.c_float * 64)()
    at = ctypes.addressof(buf)
    e = _native.GroupedRnnNet(**{k: at + 4 * i for i, k in enumerate(NEW)})
    e.net = _native.GroupedNet(src=at, ld=40, col=3, din=17, n_layers=2, act=1, out=5, hidden=64, ln_eps=1e-5, w1=at, wh=at,
                               bh=at, y=at, noise=at, actions=at, logp=at)
    for l in range(2):
        e.net.bias[l], e.net.ln_g[l], e.net.ln_b[l] = at, at, at
    e.net.w2[0] = at
    for k, v in over.items():
        setattr(e.net if k in ("src", "out", "act") else e, k, v)
    return e, buf


@pytest.mark.parametrize("over,code", [(dict([(k, None)]), -1) for k in NEW] + [
    (dict(w_hh=1026), -5),
    (dict(src=None), -1), (dict(out=33), -2), (dict(act=3), -3)])          # a bad embedded net
def test_prepare_refuses_bad_descriptors(over, code):
    table, (good, keep), (bad, keep2) = (ctypes.c_double * 128)(), _net(), _net(**over)
    lib = _native.lib()
    assert lib.mappo_grouped_rnn_prepare((_native.GroupedRnnNet * 2)(good, bad), 2, ctypes.addressof(table)) == code


def test_state_must_not_be_updated_in_place_and_entry_points_refuse_bad_calls():
    lib, keep = _native.lib(), (ctypes.c_double * 128)()
    same, buf = _net()
    same.h_out = same.h_in
    nets, table = (_native.GroupedRnnNet * 1)(_net()[0]), ctypes.addressof(keep)
    assert lib.mappo_grouped_rnn_prepare((_native.GroupedRnnNet * 1)(same), 1, table) == -2
    assert lib.mappo_grouped_rnn_prepare(None, 1, table) == -1 and lib.mappo_grouped_rnn_prepare(nets, 1, None) == -1
    assert lib.mappo_grouped_rnn_prepare(nets, 0, table) == -2 and lib.mappo_grouped_rnn_prepare(nets, 129, table) == -2
    assert lib.mappo_grouped_rnn_forward(None, 1, 8, None) == -1
    for G, rows in ((0, 8), (129, 8), (1, 0), (1, -3)):
        assert lib.mappo_grouped_rnn_forward(table, G, rows, None) == -2
    assert lib.mappo_grouped_rnn_table_bytes(128) == 128 * ctypes.sizeof(_native.GroupedRnnNet)
    assert lib.mappo_grouped_rnn_table_bytes(0) == 0


def test_descriptor_layout_matches_the_header():
    src = open(ROOT + "/include/mappo_hip.h").read()
    body = src[src.index("typedef struct mappo_grouped_rnn_net {"):src.index("} mappo_grouped_rnn_net_t;")]
    declared = re.findall(r"^\s+(?:const )?\w+\*? (\w+);", body, flags=re.M)
    assert declared == [name for name, _ in _native.GroupedRnnNet._fields_] == ["net"] + list(NEW)
    assert _native.GroupedRnnNet.net.offset == 0 and _native.GroupedRnnNet.h_in.offset == ctypes.sizeof(_native.GroupedNet)
    assert ctypes.sizeof(_native.GroupedRnnNet) == 208 + 9 * 8


def test_route_needs_both_switches(monkeypatch):
    monkeypatch.delenv("MAPPO_GROUPED_ROLLOUT", raising=False)
    monkeypatch.setenv("MAPPO_GROUPED_ROLLOUT_RNN", "1")
    assert not grouped_rollout.rnn_enabled()
    monkeypatch.setenv("MAPPO_GROUPED_ROLLOUT", "1")
    assert grouped_rollout.rnn_enabled()
    monkeypatch.delenv("MAPPO_GROUPED_ROLLOUT_RNN")
    assert grouped_rollout.enabled() and not grouped_rollout.rnn_enabled()


def _policies(*kws):
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    return [R_MAPPOPolicy(make_args(**kw), Box((6,)), Box((12,)), Discrete(5)) for kw in kws]


@pytest.mark.parametrize("kws,word", [
    ([dict(use_recurrent_policy=True, recurrent_N=2)] * 2, "recurrent_N = 2"),
    ([dict(use_recurrent_policy=True), dict()], "mixed"),
    ([dict(use_recurrent_policy=True)] * 2, "HIP device")])
def test_recurrent_route_names_what_it_refuses(kws, word):
    policies = _policies(*kws)
    why = grouped_rollout.refusal(policies, recurrent=True)
    assert why is not None and word in why, why
    if kws[0] == kws[1]:
        assert "recurrent policies" in grouped_rollout.refusal(policies)
