"""-m gpu: the row-normalisation kernels (K6, on-policy_amd/csrc/mappo_norm.hip) and the two other standardisers
(``mappo_slab_copy_std``, ``mappo_standardize_rows_ld``) against float64, at every kernel shape ``LN_FOR_SHAPES`` builds
and past the caps of their grids.

The kernels are driven through the C ABI with ctypes, so that alignment and NULL arguments are the test's to choose:
every operand is carved out of a larger NaN-filled buffer, on a 16-byte boundary or one float past it, and the NaN
canaries around every output (the ``partials`` workspace included) have to survive bit for bit.  Widths and row counts
come from tests/row_norm_cases.py (tests/test_row_norm_cpu.py shows that they reach every built shape): per shape one
row, one row more than a workgroup covers per trip, and ``cap * RPB + RPB / 2 + 1`` rows -- a second, ragged trip of the
row loop (the gather's narrow shapes hold two rows per iteration: there that count fills the second row, and one
more count past twice the cap takes the loop's second trip).

Yardstick: ``loss_reference.Judge`` -- the kernel's error against float64 is at most 4 x the error of the same expression
in float32 torch on the device, plus a floor; ``y`` / ``dx`` / ``rstd`` relative to the tensor's max-abs, the three
column sums relative to the largest column's sum of |per-row term|, ``mean`` to the largest row's mean of |activation|.
Floors: about 3 x the largest kernel error measured on the MI355X (profiles/small_kernel_margins.json, ``k6.*``), never
above the 1e-5 they began at.  The backward is fed the kernel's own ``mean`` / ``rstd``, as the autograd function does.
"""
import ctypes

import pytest
import torch

import loss_reference as lr
import row_norm_cases as rn
from carved import DEV, NAN_BITS, Carved, chunk_map as _chunk_map

pytestmark = pytest.mark.gpu
E_NULL, E_SHAPE, E_FLAGS = -1, -2, -3
JUDGE = lr.Judge()
# floors of the 4 x judge: ~3 x the largest kernel error measured on the MI355X, never above 1e-5 (module docstring)
FLOOR = {"k6.y": 7.5e-7, "k6.mean": 6e-7, "k6.rstd": 6e-7, "k6.dx": 8e-7, "k6.dw": 6.5e-7, "k6.db": 2.5e-7, "k6.dpre": 6e-7,
         # x = 100 + randn: the rounding of x - mean alone is 2^-24 * 100 against a spread of 1 (6.1e-6 measured on y)
         "k6.far.y": 1e-5, "k6.far.mean": 3.5e-7, "k6.far.rstd": 4e-7, "k6.far.dx": 1e-5, "k6.far.dw": 1e-5,
         "k6.far.db": 2.5e-7, "k6.far.dpre": 5e-6,
         "k6.gather": 6e-7, "k6.slab": 6e-7, "k6.rows_ld": 6e-7, "k6.module": 4e-7}
# Rows of at most NARROW floats are judged under names of their own (``k6.narrow.*``): with so few elements a row's variance
# is now and then far below eps or its centred values cancel (D = 2: xhat = +-1 and dx = 0 up to rounding), so the float32
# error relative to the tensor's scale is that of the problem, in torch as in the kernels (measured: 7.4e-2 on dx for both)
# -- the 4 x e_torch32 term carries those cases, their floors stay at 1e-5 where 3 x the measurement exceeds it, and under
# the names of the wider shapes they would only hide what those achieve.
NARROW = 16
FLOOR.update({"k6.narrow.y": 1e-5, "k6.narrow.mean": 4.5e-7, "k6.narrow.rstd": 1e-5, "k6.narrow.dx": 1e-5,
              "k6.narrow.dw": 9e-7, "k6.narrow.db": 2e-7, "k6.narrow.dpre": 1e-5, "k6.narrow.gather": 1e-5,
              "k6.narrow.slab": 1e-5, "k6.narrow.far.y": 1e-5, "k6.narrow.far.mean": 5e-7, "k6.narrow.far.rstd": 4e-7,
              "k6.narrow.far.dx": 1e-5, "k6.narrow.far.dw": 1e-5, "k6.narrow.far.db": 2.5e-7, "k6.narrow.far.dpre": 1e-5})


def _prefix(D, far=False):
    return "k6." + ("narrow." if D <= NARROW else "") + ("far." if far else "")


@pytest.fixture(autouse=True, scope="module")
def _record_margins():
    yield
    JUDGE.dump()


def _lib():
    from onpolicy import _native
    return _native.lib()


def _cap():
    return _lib().mappo_layernorm_max_blocks()


def _stream():
    from onpolicy import _native
    return _native.stream_of(DEV)


def _tag(shape):
    return "v%d.l%d.e%d" % shape


def _ptr(c):
    return None if c is None else c.ptr()


def _forward(inp, act, off):
    """-> (y, mean, rstd) as Carved outputs; ``off``: operand name -> floats past the 16-byte boundary."""
    rows, D = inp["x"].shape
    x = Carved(rows * D, off.get("x", 0), inp["x"])
    w = Carved(D, off.get("weight", 0), inp["weight"])
    b = Carved(D, off.get("bias", 0), inp["bias"])
    pre = None if inp["pre"] is None else Carved(D, off.get("pre_bias", 0), inp["pre"])
    y, mean, rstd = Carved(rows * D, off.get("y", 0)), Carved(rows), Carved(rows)
    rc = _lib().mappo_bias_act_layernorm_fwd(x.ptr(), _ptr(pre), w.ptr(), b.ptr(), y.ptr(), mean.ptr(), rstd.ptr(), rows, D,
                                             rn.EPS, act, _stream())
    assert rc == 0, rc
    return y, mean, rstd


def _backward(inp, act, mean, rstd, off, need_dx=True, need_dpre=False):
    """-> dict of Carved outputs dx (or None), dw, db, dpre (or None), partials."""
    rows, D = inp["x"].shape
    x = Carved(rows * D, off.get("x", 0), inp["x"])
    dy = Carved(rows * D, off.get("dy", 0), inp["dy"])
    w = Carved(D, off.get("weight", 0), inp["weight"])
    pre = None if inp["pre"] is None else Carved(D, off.get("pre_bias", 0), inp["pre"])
    dx = Carved(rows * D, off.get("dx", 0)) if need_dx else None
    dw, db = Carved(D), Carved(D)
    dpre = Carved(D) if need_dpre else None
    partials = Carved((3 if need_dpre else 2) * _cap() * D)         # exactly what the header promises to use
    rc = _lib().mappo_bias_act_layernorm_bwd(dy.ptr(), x.ptr(), _ptr(pre), mean.ptr(), rstd.ptr(), w.ptr(), _ptr(dx), dw.ptr(),
                                             db.ptr(), _ptr(dpre), partials.ptr(), rows, D, act, _stream())
    assert rc == 0, rc
    return dict(dx=dx, dw=dw, db=db, dpre=dpre, partials=partials)


def _judge_case(prefix, tag, inp, act, off=None, what=""):
    """Forward, backward with dx (and dpre_bias where the launcher takes it), backward without dx: every output against
    float64 under the judge, every canary intact."""
    off = off or {}
    rows, D = inp["x"].shape
    ref64 = rn.reference(inp["x"], inp["pre"], inp["weight"], inp["bias"], inp["dy"], act, torch.float64)
    ref32 = rn.reference(inp["x"], inp["pre"], inp["weight"], inp["bias"], inp["dy"], act, torch.float32)
    what = "%s flags=D=%d rows=%d act=%d pre=%d %s" % (tag, D, rows, act, inp["pre"] is not None, what)

    def check(name, mine, scale=None):
        shape = ref64[name].shape
        JUDGE.check(prefix + name, mine.t.view(shape), ref32[name], ref64[name], FLOOR[prefix + name],
                    scale=None if scale is None else float(ref64[scale]), what=what)
        assert mine.intact(), (name, what)

    y, mean, rstd = _forward(inp, act, off)
    check("y", y)
    check("mean", mean, "scale_mean")
    check("rstd", rstd)
    need_dpre = inp["pre"] is not None and D <= 1024
    out = _backward(inp, act, mean, rstd, off, need_dx=True, need_dpre=need_dpre)
    check("dx", out["dx"])
    check("dw", out["dw"], "scale_dw")
    check("db", out["db"], "scale_db")
    if need_dpre:
        check("dpre", out["dpre"], "scale_dpre")
    assert out["partials"].intact(), what
    nodx = _backward(inp, act, mean, rstd, off, need_dx=False)
    check("dw", nodx["dw"], "scale_dw")
    check("db", nodx["db"], "scale_db")
    assert nodx["partials"].intact(), what
    assert mean.intact() and rstd.intact()


# ------------------------------------------------------------------------------------ LayerNorm, every shape
@pytest.mark.parametrize("D", rn.ALIGNED + rn.SCALAR)
def test_layernorm_every_shape_against_float64(D):
    shape = rn.shape_of(_lib(), D, 1)
    assert shape is not None and shape[0] == (4 if D % 4 == 0 else 1)
    counts = rn.row_counts(shape[1], _cap())
    for rows in counts:
        for act in (0, 1, 2):
            for with_pre in (False, True):
                inp = rn.make_inputs(rows, D, DEV, seed=act, relu_zeros=(act == 2), with_pre=with_pre)
                _judge_case(_prefix(D), _tag(shape), inp, act)
    # x = 100 + randn: a one-pass variance E[x^2] - E[x]^2 has lost its digits here
    inp = rn.make_inputs(counts[1], D, DEV, seed=7, far=True)
    _judge_case(_prefix(D, far=True), _tag(shape), inp, 0, what="far")


@pytest.mark.parametrize("operand", ["x", "y", "weight", "bias", "pre_bias", "dy", "dx"])
@pytest.mark.parametrize("D", rn.MISALIGNED)
def test_layernorm_operand_off_a_16_byte_boundary(D, operand):
    """One operand one float past the boundary (4-byte aligned, as every float pointer must be): the launchers demote the
    call to the scalar shape of that width."""
    shape = rn.shape_of(_lib(), D, 0)
    assert shape is not None and shape[0] == 1
    for rows in rn.row_counts(shape[1], _cap()):
        inp = rn.make_inputs(rows, D, DEV, seed=3)
        _judge_case(_prefix(D), _tag(shape), inp, 1, off={operand: 1}, what="off16=" + operand)


def test_width_one_is_exact():
    """D = 1: the row is its own mean -- y = bias, dx = 0, dw = 0 and db = sum dy, all exactly (dy: small integers, so
    that the sum is exact in any order)."""
    shape = rn.shape_of(_lib(), 1, 1)
    for rows in rn.row_counts(shape[1], _cap()):
        inp = rn.make_inputs(rows, 1, DEV, seed=1, with_pre=False)
        g = torch.Generator(device=DEV).manual_seed(rows)
        inp["dy"] = torch.randint(-8, 9, (rows, 1), device=DEV, generator=g).float()
        for act in (0, 1, 2):
            y, mean, rstd = _forward(inp, act, {})
            out = _backward(inp, act, mean, rstd, {})
            assert bool((y.t == inp["bias"][0]).all())
            assert bool((out["dx"].t == 0).all()) and bool((out["dw"].t == 0).all())
            assert float(out["db"].t[0]) == float(inp["dy"].double().sum())
            assert all(c.intact() for c in (y, mean, rstd, out["dx"], out["dw"], out["db"], out["partials"]))


@pytest.mark.parametrize("D", [64, 11, 1285])
def test_one_nan_row_stays_in_its_row(D):
    shape = rn.shape_of(_lib(), D, 1)
    rows = rn.row_counts(shape[1], _cap())[2]
    inp = rn.make_inputs(rows, D, DEV, seed=2)
    bad = rows // 2 + 1
    y0, mean0, rstd0 = _forward(inp, 1, {})
    dx0 = _backward(inp, 1, mean0, rstd0, {})["dx"]
    inp["x"] = inp["x"].clone()
    inp["x"][bad, D // 2] = float("nan")
    y1, mean1, rstd1 = _forward(inp, 1, {})
    dx1 = _backward(inp, 1, mean1, rstd1, {})["dx"]
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[bad] = False
    bits = lambda c, shape: c.t.view(torch.int32).view(shape)
    for a, b in ((y0, y1), (dx0, dx1)):
        assert bool(torch.isnan(b.t.view(rows, D)[bad]).all())
        assert torch.equal(bits(a, (rows, D))[keep], bits(b, (rows, D))[keep])
    for a, b in ((mean0, mean1), (rstd0, rstd1)):
        assert torch.equal(bits(a, (rows,))[keep], bits(b, (rows,))[keep])


@pytest.mark.parametrize("D", [64, 150, 1024])
def test_backward_twice_is_bit_identical(D):
    shape = rn.shape_of(_lib(), D, 1)
    rows = rn.row_counts(shape[1], _cap())[2]
    inp = rn.make_inputs(rows, D, DEV, seed=4)
    y, mean, rstd = _forward(inp, 2, {})
    a = _backward(inp, 2, mean, rstd, {}, need_dpre=True)
    b = _backward(inp, 2, mean, rstd, {}, need_dpre=True)
    for k in ("dx", "dw", "db", "dpre"):
        assert torch.equal(a[k].t.view(torch.int32), b[k].t.view(torch.int32)), k


def test_refusals_return_their_code_and_launch_nothing():
    lib = _lib()
    rows = 2
    bufs = {k: Carved(rows * 2052) for k in ("dy", "x", "pre", "mean", "rstd", "w", "b", "y", "dx", "dw", "db", "dpre", "part")}
    p = {k: c.ptr() for k, c in bufs.items()}
    fwd = lambda D, act=0: lib.mappo_bias_act_layernorm_fwd(p["x"], p["pre"], p["w"], p["b"], p["y"], p["mean"], p["rstd"],
                                                           rows, D, rn.EPS, act, _stream())
    bwd = lambda D, act=0, dx=p["dx"], dpre=None: lib.mappo_bias_act_layernorm_bwd(
        p["dy"], p["x"], p["pre"], p["mean"], p["rstd"], p["w"], dx, p["dw"], p["db"], dpre, p["part"], rows, D, act, _stream())
    assert fwd(1537) == E_SHAPE and bwd(1537) == E_SHAPE
    assert fwd(2052) == E_SHAPE and bwd(2052) == E_SHAPE
    assert bwd(1028, dpre=p["dpre"]) == E_SHAPE
    assert bwd(64, dx=None, dpre=p["dpre"]) == E_NULL
    assert fwd(64, act=3) == E_FLAGS and bwd(64, act=3) == E_FLAGS
    torch.cuda.synchronize()
    for k, c in bufs.items():           # nothing was written anywhere
        assert bool((c.buf.view(torch.int32) == NAN_BITS).all()), k


# ------------------------------------------------------------------------------------ the standardising gather
SRC_ROWS = 1008
CHUNK = dict(L=3, T=7, N=16, A=9)           # T % L != 0; T * N * A = SRC_ROWS


def _gather_counts(shape):
    """The three row counts; shapes of at most two accesses per lane hold two rows per iteration (RI = 2 in
    gather_std_kernel), so past the cap the second row is live but the loop still makes one trip: one more count, past
    twice the cap, for its second trip."""
    counts = rn.row_counts(shape[1], _cap())
    if shape[2] <= 2:
        rpb = rn.THREADS // shape[1]
        counts += (2 * _cap() * rpb + rpb // 2 + 1,)
    return counts


def _gather(src, dst, idx, mb, D, chunk=None, first=None):
    """``mappo_gather_rows`` / ``mappo_gather_chunks`` with standardize = 1; ``first``: a first_only field alongside."""
    from onpolicy import _native
    n = 1 if first is None else 2
    fields = (_native.Field * n)()
    fields[0] = _native.Field(src.ptr(), dst.ptr(), D, 0, 0, 1)
    if first is not None:
        fields[1] = _native.Field(src.ptr(), first.ptr(), D, 1, 0, 1)
    if chunk is None:
        rc = _lib().mappo_gather_rows(fields, n, idx.data_ptr(), mb, None, _stream())
    else:
        rc = _lib().mappo_gather_chunks(fields, n, idx.data_ptr(), mb, chunk["L"], chunk["T"], chunk["N"], chunk["A"], None,
                                        _stream())
    assert rc == 0, rc


def _judge_gather(tag, src, dst, rows_map, D, what):
    rows = rows_map.numel()
    picked = src.t.view(SRC_ROWS, D)[rows_map].contiguous()
    out = dst.t.view(rows, D)
    JUDGE.check(_prefix(D) + "gather", out, rn.standardized(picked, torch.float32), rn.standardized(picked),
                FLOOR[_prefix(D) + "gather"],
                what="%s flags=D=%d rows=%d %s" % (tag, D, rows, what))
    assert dst.intact(), what
    # the same rows gathered first by torch indexing, then standardised in place order: the statistics' arithmetic does
    # not depend on where the row came from, so any difference is a wrong source row
    # (an operand off its boundary on one side, one on the other: the same kernel shape runs both)
    again = Carved(rows * D, 0 if dst.ptr() % 16 == 0 and src.ptr() % 16 == 0 else 1)
    ident = torch.arange(rows, dtype=torch.int64, device=DEV)
    from onpolicy import _native
    fields = (_native.Field * 1)(_native.Field(picked.data_ptr(), again.ptr(), D, 0, 0, 1))
    assert _lib().mappo_gather_rows(fields, 1, ident.data_ptr(), rows, None, _stream()) == 0
    assert torch.equal(out.view(torch.int32), again.t.view(rows, D).view(torch.int32)), what
    assert again.intact(), what


@pytest.mark.parametrize("D", rn.ALIGNED + rn.SCALAR)
def test_standardising_gather_every_shape(D):
    shape = rn.shape_of(_lib(), D, 1)
    tag = _tag(shape)
    g = torch.Generator(device=DEV).manual_seed(D)
    src = Carved(SRC_ROWS * D, 0, 3.0 * torch.randn(SRC_ROWS, D, device=DEV, generator=g) + 1.0)
    for rows in _gather_counts(shape):
        idx = torch.randint(0, SRC_ROWS, (rows,), device=DEV, generator=g)
        dst = Carved(rows * D)
        _gather(src, dst, idx, rows, D)
        _judge_gather(tag, src, dst, idx, D, "rows")
        # chunk mode: L output rows per index (the counts rounded up to a multiple of L), one first_only field alongside
        L = CHUNK["L"]
        mb = (rows + L - 1) // L
        idx = torch.randint(0, SRC_ROWS // L, (mb,), device=DEV, generator=g)
        dst, first = Carved(mb * L * D), Carved(mb * D)
        _gather(src, dst, idx, mb, D, chunk=CHUNK, first=first)
        _judge_gather(tag, src, dst, _chunk_map(idx, mb, **CHUNK), D, "chunks")
        _judge_gather(tag, src, first, _chunk_map(idx, mb, first_only=True, **CHUNK), D, "chunks first_only")


@pytest.mark.parametrize("operand", ["src", "dst"])
@pytest.mark.parametrize("D", rn.MISALIGNED)
def test_standardising_gather_off_a_16_byte_boundary(D, operand):
    shape = rn.shape_of(_lib(), D, 0)
    g = torch.Generator(device=DEV).manual_seed(D + 1)
    src = Carved(SRC_ROWS * D, 1 if operand == "src" else 0, 3.0 * torch.randn(SRC_ROWS, D, device=DEV, generator=g) + 1.0)
    for rows in _gather_counts(shape):
        idx = torch.randint(0, SRC_ROWS, (rows,), device=DEV, generator=g)
        dst = Carved(rows * D, 1 if operand == "dst" else 0)
        _gather(src, dst, idx, rows, D)
        _judge_gather(_tag(shape), src, dst, idx, D, "rows off16=" + operand)


# ------------------------------------------------------------------------------------ the resident copies' standardisers
def _check_padded(name, out, x, D, ld, dst, what):
    rows = x.shape[0]
    out = out.view(rows, ld)
    JUDGE.check(name, out[:, :D], rn.standardized(x, torch.float32), rn.standardized(x), FLOOR[name],
                what="D=%d flags=rows=%d ld=%d %s" % (D, rows, ld, what))
    assert bool((out[:, D:] == 0).all()), what          # padding columns: exactly zero
    assert dst.intact(), what


def _slab_std(descs, slabs=()):
    from onpolicy import _native
    std = (_native.StdSlab * len(descs))(*[_native.StdSlab(s, d, rows, D, ld, rn.EPS) for s, d, rows, D, ld in descs])
    cp = (_native.Slab * len(slabs))(*[_native.Slab(s, d, n) for s, d, n in slabs]) if slabs else None
    rc = _lib().mappo_slab_copy_std(cp, len(slabs), std, len(descs), _stream())
    assert rc == 0, rc


SLAB_ROWS = (1, 17, 16 * 1024 + 9)          # the last: two trips per 16-lane group (kCUs * 4 workgroups of 16 groups)


@pytest.mark.parametrize("D", [1, 3, 4, 11, 18, 54, 63, 64, 65, 370, 1285, 2166])
def test_slab_copy_std_against_float64(D):
    g = torch.Generator(device=DEV).manual_seed(D + 2)
    for ld in ((D + 3) // 4 * 4, D + 7):
        for rows in SLAB_ROWS:
            x = 3.0 * torch.randn(rows, D, device=DEV, generator=g) + 1.0
            dst = Carved(rows * ld)
            _slab_std([(x.data_ptr(), dst.ptr(), rows, D, ld)])
            _check_padded(_prefix(D) + "slab", dst.t, x, D, ld, dst, "one descriptor")
    # the last count again as four unequal descriptors, with copy slabs (16-byte and float units) in the same launch
    rows, ld = SLAB_ROWS[-1], (D + 3) // 4 * 4
    x = 3.0 * torch.randn(rows, D, device=DEV, generator=g) + 1.0
    one = Carved(rows * ld)
    _slab_std([(x.data_ptr(), one.ptr(), rows, D, ld)])
    cuts = [0, 1, rows // 4 + 1, rows - rows // 40, rows]
    four = Carved(rows * ld)
    descs = [(x[a:b].data_ptr(), four.ptr() + 4 * a * ld, b - a, D, ld) for a, b in zip(cuts[:-1], cuts[1:])]
    c_src = [torch.randn(n, device=DEV, generator=g) for n in (4 * 4096 + 8, 100003)]
    c_dst = [Carved(t.numel()) for t in c_src]
    _slab_std(descs, [(s.data_ptr(), d.ptr(), s.numel()) for s, d in zip(c_src, c_dst)])
    _check_padded(_prefix(D) + "slab", four.t, x, D, ld, four, "four descriptors + copies")
    assert torch.equal(four.t.view(torch.int32), one.t.view(torch.int32))        # a row does not depend on its descriptor
    for s, d in zip(c_src, c_dst):
        assert torch.equal(s, d.t) and d.intact()


ROWS_LD = (1, 17, 32 * 1024 + 9)            # the last: two trips per 16-lane group (2048 workgroups of 16 groups)


@pytest.mark.parametrize("D", [64, 65, 256, 257, 512, 513, 1285])
def test_standardize_rows_ld_against_float64(D):
    """Either side of every dispatch boundary of mlp::standardize_rows (NV = 1 | 4 | 8 | 0 register pieces per lane)."""
    g = torch.Generator(device=DEV).manual_seed(D + 3)
    for ld in ((D + 3) // 4 * 4, D + 7):
        for rows in ROWS_LD:
            x = 3.0 * torch.randn(rows, D, device=DEV, generator=g) + 1.0
            dst = Carved(rows * ld)
            rc = _lib().mappo_standardize_rows_ld(x.data_ptr(), rows, D, rn.EPS, dst.ptr(), ld, _stream())
            assert rc == 0, rc
            _check_padded("k6.rows_ld", dst.t, x, D, ld, dst, "")


# ------------------------------------------------------------------------------------ the module on a misaligned view
@pytest.mark.parametrize("misaligned", ["x", "x dy", "x weight bias"])
@pytest.mark.parametrize("D", [2048, 1600])
def test_fused_layernorm_on_a_misaligned_contiguous_view(D, misaligned):
    """A contiguous view that starts one float past a 16-byte boundary: above 1536 floats the kernels have no scalar
    shape for it (MAPPO_E_SHAPE); FusedLayerNorm still normalises -- through the HIP kernels, from aligned copies."""
    from onpolicy import _native
    from onpolicy.algorithms.utils.fused_norm import FusedLayerNorm
    rows = 37
    inp = rn.make_inputs(rows, D, DEV, seed=5, with_pre=False)
    assert _lib().mappo_layernorm_shape(D, 0) == 0 and _lib().mappo_layernorm_shape(D, 1) != 0
    off = {k: 1 for k in misaligned.split()}
    x = Carved(rows * D, off.get("x", 0), inp["x"]).t.view(rows, D).detach().requires_grad_(True)
    dy = Carved(rows * D, off.get("dy", 0), inp["dy"]).t.view(rows, D)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    ln = FusedLayerNorm(D).to(DEV)
    ln.weight.data = Carved(D, off.get("weight", 0), inp["weight"]).t
    ln.bias.data = Carved(D, off.get("bias", 0), inp["bias"]).t
    _native.count_calls(True)
    try:
        y = ln(x)
        y.backward(dy)
        calls = _native.calls()
    finally:
        _native.count_calls(False)
    assert calls.get("mappo_bias_act_layernorm_fwd") == 1 and calls.get("mappo_bias_act_layernorm_bwd") == 1, calls
    ref64 = rn.reference(inp["x"], None, inp["weight"], inp["bias"], inp["dy"], 0, torch.float64)
    ref32 = rn.reference(inp["x"], None, inp["weight"], inp["bias"], inp["dy"], 0, torch.float32)
    for name, mine, scale in (("y", y.detach(), None), ("dx", x.grad, None), ("dw", ln.weight.grad, "scale_dw"),
                              ("db", ln.bias.grad, "scale_db")):
        JUDGE.check("k6.module", mine, ref32[name], ref64[name], FLOOR["k6.module"],
                    scale=None if scale is None else float(ref64[scale]),
                    what="D=%d flags=%s off16=%s" % (D, name, misaligned))
