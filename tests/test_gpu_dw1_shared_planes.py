"""-m gpu: the six-term direct first-layer weight-gradient kernel with the dz1 tile's bf16 planes split once per workgroup
and shared through LDS (the default) against the same kernel with every wave splitting the whole tile itself (option
bit 16384).  Same split function, same term order, same order of tiles on every accumulator: every parameter gradient
must be bit for bit the same (tests/test_dw1_shared_planes_emulated.py is the same comparison on the host emulator)."""
import pytest
import torch
import torch.nn as nn

from helpers import make_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PER_WAVE = 16384


def _gradients(din, rows, flags, cap):
    from onpolicy import _native
    from onpolicy.algorithms.utils import fused_mlp
    from onpolicy.algorithms.utils.mlp import MLPBase
    torch.manual_seed(din)
    base = MLPBase(make_args(hidden_size=64, layer_N=1, use_ReLU=False), (din,)).to(DEV)
    head = nn.Linear(64, 1).to(DEV)
    g = torch.Generator().manual_seed(din + rows)
    src_rows = rows + 500
    src = (torch.randn(src_rows, din, generator=g) * 1.5 + 0.7).to(DEV)
    idx = torch.randperm(src_rows, generator=g)[:rows].to(DEV)
    dy = torch.randn(rows, 1, generator=g).to(DEV)
    lib = _native.lib()
    old = lib.mappo_mlp_set_flags(flags)
    assert old >= 0
    lib.mappo_mlp_set_grid_cap(cap)
    try:
        rs = fused_mlp.RowSource(fused_mlp.standardize_rows(src), idx, standardized=True, width=din)
        y = fused_mlp.trunk_forward(base, rs, head)
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        lib.mappo_mlp_set_grid_cap(0)
        lib.mappo_mlp_set_flags(old)
    return {name: p.grad.detach().cpu() for name, p in list(base.named_parameters()) + list(head.named_parameters())}


@pytest.fixture(autouse=True)
def _six_term(monkeypatch):
    monkeypatch.setenv("MAPPO_MATRIX_ARITHMETIC", "six_term")


@pytest.mark.parametrize("cap", [0, 3], ids=["default_grid", "cap3"])
@pytest.mark.parametrize("din,rows", [(384, 16 * 300 + 5), (200, 16 * 64 + 1)])
def test_shared_planes_give_the_bits_of_the_per_wave_split(din, rows, cap):
    shared = _gradients(din, rows, 0, cap)
    per_wave = _gradients(din, rows, PER_WAVE, cap)
    assert shared.keys() == per_wave.keys() and any(tuple(v.shape) == (64, din) for v in shared.values())
    for name, v in shared.items():
        assert torch.isfinite(v).all(), name
        assert torch.equal(v, per_wave[name]), name
