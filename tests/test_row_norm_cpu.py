"""No GPU: the case table of the row-normalisation tests reaches every kernel shape that mappo_norm.hip builds (asked
of the library itself through ``mappo_layernorm_shape``), the widths the launchers refuse are refused by the query and by
the entry points before anything is enqueued, and the float64 reference the device tests judge against is
``torch.nn.functional.layer_norm`` + autograd."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import row_norm_cases as rn
from onpolicy import _native


def test_ln_for_shapes_is_parsed():
    shapes = rn.built_shapes()
    assert len(shapes) == len(set(shapes)) >= 18
    assert (4, 64, 8) in shapes and (1, 64, 24) in shapes and (1, 4, 1) in shapes
    for vec, lpr, epl in shapes:
        assert vec in (1, 4) and lpr in (4, 8, 16, 32, 64) and epl >= 1


def test_width_table_reaches_every_built_shape():
    """Every entry of LN_FOR_SHAPES is the shape of some width of the table -- a shape added later without a width fails
    here -- and each shape is met at two widths or more, the widest the launchers accept among them."""
    lib = _native.lib()
    built = set(rn.built_shapes())
    reached = {}
    for D, aligned in rn.TABLE:
        s = rn.shape_of(lib, D, aligned)
        assert s is not None and s in built, (D, aligned, s)
        reached.setdefault(s, []).append(D)
    assert set(reached) == built, sorted(built - set(reached))
    for D in rn.ALIGNED:
        assert rn.shape_of(lib, D, 1)[0] == 4
    for D, aligned in rn.TABLE:
        if not aligned or D % 4:
            assert rn.shape_of(lib, D, aligned)[0] == 1
    # every shape at two widths or more, and the widest width of either kind of operand is in the table
    assert all(len(set(ws)) >= 2 for ws in reached.values()), reached
    assert max(D for D in range(1, 4096) if rn.shape_of(lib, D, 1)) == 2048 == max(rn.ALIGNED)
    assert max(D for D in range(1, 4096) if rn.shape_of(lib, D, 0)) == 1536 == max(rn.MISALIGNED)
    assert max(D for D in range(1, 4096) if D % 4 and rn.shape_of(lib, D, 1)) == 1535 == max(rn.SCALAR)
    # the demotion: a multiple of four off a 16-byte boundary takes the scalar shape of the same width
    for D in rn.MISALIGNED:
        assert rn.shape_of(lib, D, 0) == (1, 64, {64: 1, 512: 8, 1024: 16, 1536: 24}[D])


def test_refused_widths():
    lib = _native.lib()
    for D, aligned in rn.REFUSED:
        assert lib.mappo_layernorm_shape(D, aligned) == 0, (D, aligned)
    for D in (0, -4):
        assert lib.mappo_layernorm_shape(D, 1) == 0
    assert lib.mappo_abi_version() == 2                 # the query is additive


def test_row_counts():
    cap = _native.lib().mappo_layernorm_max_blocks()
    assert cap == 2048
    assert rn.row_counts(64, cap) == (1, 5, 8195)
    assert rn.row_counts(4, cap) == (1, 65, 131105)
    for lpr in (4, 8, 16, 32, 64):
        rpb = 256 // lpr
        last = rn.row_counts(lpr, cap)[2]
        assert last > cap * rpb and (last - cap * rpb) % rpb != 0       # a second trip, and a ragged one


def test_launchers_refuse_before_any_launch():
    """Return codes only; validation comes before the first launch, so host memory serves as the pointers."""
    lib = _native.lib()
    keep = [(ctypes.c_float * 4096)() for _ in range(11)]
    dy, x, pre, mean, rstd, w, b, y, dx, dwb, part = [ctypes.addressof(k) for k in keep]
    fwd = lambda D, act=0: lib.mappo_bias_act_layernorm_fwd(x, pre, w, b, y, mean, rstd, 1, D, 1e-5, act, None)
    bwd = lambda D, act=0, dx=dx, dpre=None: lib.mappo_bias_act_layernorm_bwd(dy, x, pre, mean, rstd, w, dx, dwb, dwb, dpre,
                                                                          part, 1, D, act, None)
    assert fwd(1537) == -2 and bwd(1537) == -2
    assert fwd(2052) == -2 and bwd(2052) == -2
    assert fwd(64, act=3) == -3 and bwd(64, act=3) == -3 and fwd(64, act=-1) == -3
    assert bwd(1028, dpre=dwb) == -2
    assert bwd(64, dx=None, dpre=dwb) == -1


def _autograd(x, pre, weight, bias, dy, act):
    z = (x if pre is None else x + pre).double().requires_grad_(True)
    w, b = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    a = torch.tanh(z) if act == 1 else torch.relu(z) if act == 2 else z
    y = F.layer_norm(a, (z.shape[-1],), w, b, rn.EPS)
    (y * dy.double()).sum().backward()
    mean = a.detach().mean(-1)
    rstd = 1.0 / torch.sqrt(a.detach().var(-1, unbiased=False) + rn.EPS)
    return dict(y=y.detach(), mean=mean, rstd=rstd, dx=z.grad, dw=w.grad, db=b.grad, dpre=z.grad.sum(0))


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_pre", [False, True])
def test_reference_is_layer_norm_and_autograd(act, with_pre):
    for rows, D in ((1, 1), (7, 3), (33, 54), (300, 64), (5, 1285)):
        for far in (False, True):
            inp = rn.make_inputs(rows, D, torch.device("cpu"), seed=act, far=far, relu_zeros=(act == 2),
                                 with_pre=with_pre)
            pre = inp["pre"]
            mine = rn.reference(inp["x"], pre, inp["weight"], inp["bias"], inp["dy"], act)
            want = _autograd(inp["x"], pre, inp["weight"], inp["bias"], inp["dy"], act)
            for k, v in want.items():
                assert mine[k].dtype == torch.float64 and mine[k].shape == v.shape, k
                # (far: the formulas divide by a variance whose float64 rounding error is 1e4 times larger relative to it)
                scale = float(v.abs().max()) + 1e-300
                assert float((mine[k] - v).abs().max()) <= 1e-12 * max(scale, 1.0), (k, rows, D, far)
            if act == 2:
                z = inp["x"] + pre if with_pre else inp["x"]
                assert rows * D < 100 or int((z == 0).sum()) > 0        # units exactly on the kink
                assert bool((mine["dx"][z == 0] == 0).all())
            torch.testing.assert_close(rn.standardized(inp["x"]),
                                       F.layer_norm(inp["x"].double(), (D,), None, None, rn.EPS), rtol=0, atol=1e-12)
            assert float(mine["scale_db"]) == float(inp["dy"].double().abs().sum(0).max())
