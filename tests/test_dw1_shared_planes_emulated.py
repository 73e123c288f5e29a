"""The six-term direct first-layer weight-gradient kernel (K9, mlp_dw1_direct_kernel<3, 2, true>) splits a tile's dz1 into
bf16 planes once per workgroup -- every wave its own four rows, the planes shared through LDS -- instead of once per wave
(option bit 16384 keeps the per-wave split).  Same split function, same term order, same order of tiles on every
accumulator: the whole gradient vector must be bit for bit the same under both, on the host SIMT emulator (tests/simt),
and the shared form must meet the float64 tolerance of test_mlp_kernels_emulated.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mlp_reference as R

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (host build of the emulator) not found")
PER_WAVE = 16384


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "simt"))
    import build
    return R.bind(ctypes.CDLL(build.build()))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _gradients(emu, seed, din, n_layers, act, out, rows, src_rows):
    """(gradients with the shared planes, gradients with the per-wave split, float64 reference); six-term arithmetic,
    rows gathered through a permuted row table"""
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal((src_rows, din)) * 1.5 + 0.7).astype(np.float32)
    p = R.random_net(rng, din, n_layers, out)
    idx = rng.permutation(src_rows)[:rows].astype(np.int64)
    n_tab = emu.mappo_mlp_row_table_ints(rows)
    tab = np.full(n_tab, -1, np.int32)
    assert emu.mappo_mlp_row_table(_ptr(idx), rows, 0, 0, 0, 0, 0, _ptr(tab), None) == 0
    srows = R.source_rows(idx, rows, chunk_len=0, mb=0, T=0, N=0, A=0)
    assert not np.array_equal(srows, np.arange(rows))
    y = np.full((rows, out if out else 64), np.nan, np.float32)
    z = [np.full((n_tab, 64), np.nan, np.float32) for _ in range(n_layers)]
    st = [np.full((n_tab, 2), np.nan, np.float32) for _ in range(n_layers)]
    m = R.MLP(src=_ptr(src), row_tab=_ptr(tab), rows=rows, din=din, n_layers=n_layers, act=act, out=out, ln_eps=1e-5,
              arith=0, w1=_ptr(p["w1"]), wh=_ptr(p["wh"]) if out else None, bh=_ptr(p["bh"]) if out else None, y=_ptr(y))
    for l in range(n_layers):
        m.bias[l], m.ln_g[l], m.ln_b[l] = _ptr(p["bias%d" % l]), _ptr(p["ln_g%d" % l]), _ptr(p["ln_b%d" % l])
        m.z[l], m.ln_stats[l] = _ptr(z[l]), _ptr(st[l])
        if l > 0:
            m.w2[l - 1] = _ptr(p["w2_%d" % (l - 1)])
    assert emu.mappo_mlp_forward(ctypes.byref(m), None) == 0
    dy = rng.standard_normal(y.shape).astype(np.float32)
    n_g = emu.mappo_mlp_grad_floats(din, n_layers, out)
    got = []
    for flags in (0, PER_WAVE):
        old = emu.mappo_mlp_set_flags(flags)
        assert old >= 0
        try:
            grads = np.full(n_g, np.nan, np.float32)
            ws = np.full(emu.mappo_mlp_workspace_floats(din, n_layers, out), np.nan, np.float32)
            dz1 = np.full((n_tab, 64), np.nan, np.float32)
            m.dy, m.dz1, m.workspace, m.grads = _ptr(dy), _ptr(dz1), _ptr(ws), _ptr(grads)
            assert emu.mappo_mlp_backward(ctypes.byref(m), None) == 0
        finally:
            emu.mappo_mlp_set_flags(old)
        got.append(grads)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    y_ref, _ = R.forward_ref(tp, src, srows, False, n_layers, act, out)
    (y_ref * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    g_ref = R.flat_grads({k: v.grad for k, v in tp.items()}, din, n_layers, out).numpy()
    return got[0], got[1], g_ref


# (din, n_layers, act, out, rows, src_rows, grid cap)
CASES = [
    (384, 2, 1, 1, 16 * 7 + 5, 200, 0),     # the critic's width: every wave owns three k tiles; a last tile of five rows
    (384, 1, 2, 1, 3, 64, 0),               # fewer rows than a tile (single-layer trunk)
    (200, 2, 1, 1, 16 * 5 + 1, 150, 0),     # seven k tiles: waves with two, one and ZERO k tiles; a tile with one live row
    (768, 1, 2, 1, 40, 64, 0),              # two slabs
    (384, 2, 1, 1, 16 * 11 + 9, 300, 2),    # two workgroups: the rings wrap, six tiles against five
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_shared_planes_give_the_bits_of_the_per_wave_split(emu, case):
    din, L, act, out, rows, src_rows, cap = case
    emu.mappo_mlp_set_grid_cap(cap)
    try:
        shared, per_wave, g_ref = _gradients(emu, din * 7 + rows, din, L, act, out, rows, src_rows)
    finally:
        emu.mappo_mlp_set_grid_cap(0)
    assert np.isfinite(shared).all()
    assert np.array_equal(shared, per_wave)
    scale = np.abs(g_ref).max()
    np.testing.assert_allclose(shared, g_ref, rtol=2e-4, atol=2e-5 * scale)


def test_the_option_bit_exists(emu):
    old = emu.mappo_mlp_set_flags(PER_WAVE)
    assert old >= 0
    assert emu.mappo_mlp_set_flags(old) == PER_WAVE
