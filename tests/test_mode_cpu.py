"""CPU-side checks of the mode form of K14 (``mappo_categorical_mode`` / ``mappo_multi_categorical_mode``): argument
validation returns before anything is enqueued, ``fused_loss.mode_supported`` refuses what the kernel cannot take, and an
``ACTLayer`` routes to it only when asked (``use_device_eval``) -- on the CPU it falls through to the framework's ops
either way."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from onpolicy import _native
from onpolicy.algorithms.utils import fused_loss
from onpolicy.algorithms.utils.act import ACTLayer
from onpolicy.envs.spaces import Discrete


def _host(n=64, ctype=ctypes.c_float):
    buf = (ctype * n)()
    return buf, ctypes.addressof(buf)


def test_categorical_mode_rejects_bad_shapes():
    lib = _native.lib()
    bufs = [_host(65 * 4), _host(65 * 4), _host(4, ctypes.c_int64), _host(4)]
    lg, av, ac, lp = [b[1] for b in bufs]
    assert lib.mappo_categorical_mode(lg, av, ac, lp, 4, 65, None) == -2           # 65 actions
    assert lib.mappo_categorical_mode(lg, av, ac, lp, 4, 0, None) == -2
    assert lib.mappo_categorical_mode(lg, av, ac, lp, 0, 5, None) == -2            # no rows
    assert lib.mappo_categorical_mode(lg, av, ac, lp, -1, 5, None) == -2
    assert lib.mappo_categorical_mode(None, av, ac, lp, 4, 5, None) == -1
    assert lib.mappo_categorical_mode(lg, av, None, lp, 4, 5, None) == -1
    assert lib.mappo_categorical_mode(lg, None, ac, None, 4, 5, None) == -1
    assert lib.mappo_categorical_mode(None, None, None, None, 0, 65, None) == -1   # NULL is reported first, as by K14


def test_multi_categorical_mode_rejects_bad_heads():
    lib = _native.lib()
    lg = _host(65 * 4)
    ac, lp = _host(64, ctypes.c_int64), _host(64)

    def call(sizes, rows=4):
        k = len(sizes)
        return lib.mappo_multi_categorical_mode(lg[1], (ctypes.c_int * max(k, 1))(*sizes), k, ac[1], lp[1], rows, None)
    assert call([]) == -2                               # 0 heads
    assert call([7] * 9) == -2                          # 9 heads
    assert call([58, 7]) == -2                          # total width 65
    assert call([65]) == -2
    assert call([1] * 7 + [58]) == -2
    assert call([5, 0, 3]) == -2                        # a head of size 0
    assert call([5, -1]) == -2
    assert call([5, 10], rows=0) == -2
    assert call([5, 10], rows=-3) == -2
    sizes = (ctypes.c_int * 2)(5, 10)
    assert lib.mappo_multi_categorical_mode(None, sizes, 2, ac[1], lp[1], 4, None) == -1
    assert lib.mappo_multi_categorical_mode(lg[1], None, 2, ac[1], lp[1], 4, None) == -1
    assert lib.mappo_multi_categorical_mode(lg[1], sizes, 2, None, lp[1], 4, None) == -1
    assert lib.mappo_multi_categorical_mode(lg[1], sizes, 2, ac[1], None, 4, None) == -1
    assert {"mappo_categorical_mode", "mappo_multi_categorical_mode"} <= set(_native.SIGNATURES)


class _FakeDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: ``mode_supported`` only looks."""
    is_cuda = True


def test_mode_supported_conditions(monkeypatch):
    monkeypatch.delenv("MAPPO_FUSED_SAMPLE", raising=False)
    with torch.no_grad():
        ok = torch.zeros(4, 5).as_subclass(_FakeDevice)
        assert fused_loss.mode_supported(ok) and fused_loss.mode_supported(ok, [2, 3])     # the conditions that remain
        assert not fused_loss.mode_supported(torch.zeros(4, 5))                             # CPU
        assert not fused_loss.mode_supported(torch.zeros(4, 5), [2, 3])
        assert not fused_loss.mode_supported(torch.zeros(4, 5, dtype=torch.float64).as_subclass(_FakeDevice))
        assert not fused_loss.mode_supported(torch.zeros(4, 65).as_subclass(_FakeDevice))   # 65 actions
        assert not fused_loss.mode_supported(torch.zeros(4, 0).as_subclass(_FakeDevice))
        assert not fused_loss.mode_supported(torch.zeros(5).as_subclass(_FakeDevice))
        assert not fused_loss.mode_supported(ok, [7] * 9) and not fused_loss.mode_supported(ok, [58, 7])
        assert not fused_loss.mode_supported(ok, [])
        assert not fused_loss.mode_supported(np.zeros((4, 5), np.float32))
        monkeypatch.setenv("MAPPO_FUSED_SAMPLE", "0")
        assert not fused_loss.mode_supported(ok) and not fused_loss.mode_supported(ok, [2, 3])
        monkeypatch.delenv("MAPPO_FUSED_SAMPLE")
        # the mode draws nothing: the sampling generator's mode is not asked
        from onpolicy.algorithms.utils import distributions
        monkeypatch.setattr(distributions, "SAMPLING_RNG", "host")
        assert fused_loss.mode_supported(ok) and not fused_loss.sample_supported(ok)
    with torch.enable_grad():
        assert not fused_loss.mode_supported(ok) and not fused_loss.mode_supported(ok, [2, 3])


class _MultiDiscrete(object):
    def __init__(self, sizes):
        self.low = np.zeros(len(sizes), dtype=np.int64)
        self.high = np.asarray(sizes, dtype=np.int64) - 1
        self.shape = len(sizes)


_MultiDiscrete.__name__ = "MultiDiscrete"


def _layer(space, **flags):
    torch.manual_seed(3)
    return ACTLayer(space, 16, True, 0.01, SimpleNamespace(**flags))


def test_fused_mode_is_off_unless_asked():
    assert _layer(Discrete(5)).fused_mode is False
    assert ACTLayer(Discrete(5), 16, True, 0.01).fused_mode is False              # args=None
    assert _layer(Discrete(5), use_device_eval=False).fused_mode is False
    assert _layer(Discrete(5), use_device_eval=True).fused_mode is True


@pytest.mark.parametrize("space", [Discrete(5), _MultiDiscrete([5, 10])], ids=["discrete", "multidiscrete"])
def test_fused_mode_falls_through_on_cpu(space):
    off, on = _layer(space), _layer(space, use_device_eval=True)
    on.load_state_dict(off.state_dict())
    x = torch.randn(33, 16, generator=torch.Generator().manual_seed(0))
    avail = None
    if space.__class__.__name__ == "Discrete":
        avail = (torch.rand(33, 5, generator=torch.Generator().manual_seed(1)) < 0.7).float()
        avail[:, 0] = 1.0
    with torch.no_grad():
        a0, l0 = off(x, avail, deterministic=True)
        a1, l1 = on(x, avail, deterministic=True)
        assert a0.dtype == a1.dtype and torch.equal(a0, a1) and torch.equal(l0, l1)
        if avail is not None:
            f0 = off.from_logits(off.action_out.linear(x), avail, deterministic=True)
            f1 = on.from_logits(on.action_out.linear(x), avail, deterministic=True)
            assert torch.equal(f0[0], f1[0]) and torch.equal(f0[1], f1[1]) and torch.equal(f1[0], a1)
