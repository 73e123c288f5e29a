"""-m gpu: the copy kernels of on-policy_amd/csrc/mappo_copy.hip through the C ABI -- K2 (``mappo_slab_copy``), K3 / K4
(``mappo_gather_rows`` / ``mappo_gather_chunks`` without ``standardize``) and the packed records (``mappo_pack_records``,
``mappo_gather_records``).

``SharedReplayBuffer`` only ever hands these kernels tensors on 256-byte boundaries; here every operand is a
``carved.Carved`` one, so the 8-byte and 4-byte paths, operands off a 16-byte boundary, the refusal codes and a second trip
of every persistent grid are reached.  Every comparison is on int32 views -- a copy is a copy of bits, and the sources hold
a few -0.0, infinities and NaN payloads besides randn -- and the NaN canaries around every output have to survive.

Constants the shapes are built from: 256 threads per workgroup; the slab tile is 256 x 8 units (a unit is 4 floats when
the count is a multiple of 4 and both pointers are 16-byte aligned, else 1 float) on at most 256 x 8 workgroups; the gather
tile is 256 x 2 units (4, 2 or 1 floats by width and alignment), ``rows_per_tile = 512 // units_per_row`` (1 from 512 units
per row on), on 256 x (workgroups per CU) workgroups.
"""
import numpy as np
import pytest
import torch

from carved import DEV, NAN_BITS, Carved, chunk_map
from oracle import oracle

pytestmark = pytest.mark.gpu
E_NULL, E_SHAPE, E_TOO_MANY, E_ALIGN = -1, -2, -4, -5
SRC_ROWS = 1008
CHUNK = dict(L=3, T=7, N=16, A=9)           # T % L != 0; T * N * A = SRC_ROWS
STATS = (0.37, 1.9)
# -0.0, +-inf, quiet NaNs with payloads of either sign, a signalling NaN
SPECIALS = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001, 0x7F800001], dtype=np.uint32).view(np.int32)


def _lib():
    from onpolicy import _native
    return _native.lib()


def _stream():
    from onpolicy import _native
    return _native.stream_of(DEV)


def _values(n, seed, nan=True):
    """``n`` floats: randn with the special bit patterns scattered in (without the NaNs for a field that gets normalised)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    v = torch.randn(n, device=DEV, generator=g)
    sp = torch.from_numpy(SPECIALS if nan else SPECIALS[:3]).to(DEV)
    pos = (torch.arange(sp.numel(), device=DEV) * 7919 + 3) % n
    v.view(torch.int32)[pos] = sp
    return v


def _bits(t):
    return t.contiguous().view(torch.int32)


def _all_nan(c):
    return bool((c.buf.view(torch.int32) == NAN_BITS).all())


# --------------------------------------------------------------------------------------------------------- K2: slabs
SLAB_COUNTS = (1, 3, 4, 2047, 2049, 4 * 2048, 4 * 2048 + 4, 4 * 4096 + 8, 100003)


def _slab_copy(triples):
    from onpolicy import _native
    arr = (_native.Slab * len(triples))(*[_native.Slab(s, d, n) for s, d, n in triples])
    return _lib().mappo_slab_copy(arr, len(triples), _stream())


def _check_slabs(cases, what):
    """``cases``: (count, source offset, destination offset) per slab of ONE launch."""
    src = [Carved(n, so, _values(n, n + k)) for k, (n, so, _) in enumerate(cases)]
    dst = [Carved(n, do) for n, _, do in cases]
    assert _slab_copy([(s.ptr(), d.ptr(), s.n) for s, d in zip(src, dst)]) == 0, what
    for s, d, case in zip(src, dst, cases):
        assert torch.equal(_bits(d.t), _bits(s.t)), (what, case)
        assert d.intact() and s.intact(), (what, case)


def test_slab_copy_counts_and_alignments():
    for n in SLAB_COUNTS:
        _check_slabs([(n, 0, 0)], "one slab")
    # a count divisible by 4 with one operand a float past the boundary: the 4-byte path
    for n in (4 * 2048, 4 * 4096 + 8):
        _check_slabs([(n, 1, 0)], "source off")
        _check_slabs([(n, 0, 1)], "destination off")
    small = SLAB_COUNTS[:-1]
    _check_slabs([(small[k % len(small)], k % 2 if k % 3 == 0 else 0, 1 if k % 5 == 4 else 0) for k in range(16)], "16 slabs")


def test_slab_copy_second_trip_of_the_grid():
    n = 2048 * 2048 + 2048 + 5              # float units: 2050 tiles on 2048 workgroups
    assert n % 4 != 0
    _check_slabs([(n, 0, 0)], "2050 tiles")


def test_slab_copy_refusals_write_nothing():
    src, dst = Carved(64, 0, _values(64, 1)), Carved(64)
    ok = (src.ptr(), dst.ptr(), 64)
    assert _slab_copy([ok] * 17) == E_TOO_MANY
    assert _slab_copy([ok, (None, dst.ptr(), 64)]) == E_NULL
    assert _slab_copy([ok, (src.ptr(), None, 64)]) == E_NULL
    assert _lib().mappo_slab_copy(None, 1, _stream()) == E_NULL
    assert _slab_copy([ok, (src.ptr(), dst.ptr(), 0)]) == E_SHAPE
    assert _slab_copy([ok, (src.ptr() + 1, dst.ptr(), 8)]) == E_ALIGN
    torch.cuda.synchronize()
    assert _all_nan(dst)


# ------------------------------------------------------------------------------------------------- K3 / K4: gathers
GATHER_WIDTHS = (1, 2, 3, 4, 5, 6, 48, 370, 384, 1285)
OFFSETS = [(w, 0, 0) for w in GATHER_WIDTHS] + \
          [(w, so, do) for w in (2, 4, 384) for so, do in ((2, 2), (1, 0), (0, 1))]      # 8-byte path; 4-byte path twice


def _rows_per_tile(width, so, do):
    vec = 4 if width % 4 == 0 and so % 4 == 0 and do % 4 == 0 else 2 if width % 2 == 0 and so % 2 == 0 and do % 2 == 0 else 1
    upr = width // vec
    return 1 if upr >= 512 else 512 // upr


assert 258 * _rows_per_tile(1, 0, 0) + 1 == 132097 and 258 * _rows_per_tile(384, 0, 0) + 1 == 1291


def _gather(fields, idx, mb, chunk=None, stats=None):
    """``fields``: (src pointer, dst pointer, width, first_only, normalize) each -> the return code."""
    from onpolicy import _native
    arr = (_native.Field * len(fields))(*[_native.Field(s, d, w, fo, nz, 0) for s, d, w, fo, nz in fields])
    st = None if stats is None else stats.data_ptr()
    if chunk is None:
        return _lib().mappo_gather_rows(arr, len(fields), idx.data_ptr(), mb, st, _stream())
    return _lib().mappo_gather_chunks(arr, len(fields), idx.data_ptr(), mb, chunk["L"], chunk["T"], chunk["N"], chunk["A"],
                                      st, _stream())


def _check_rows(src, width, do, rows, g, what):
    idx = torch.randint(0, SRC_ROWS, (rows,), device=DEV, generator=g)
    dst = Carved(rows * width, do)
    assert _gather([(src.ptr(), dst.ptr(), width, 0, 0)], idx, rows) == 0, what
    assert torch.equal(_bits(dst.t.view(rows, width)), _bits(src.t.view(SRC_ROWS, width)[idx])), what
    assert dst.intact(), what


@pytest.mark.parametrize("width,so,do", OFFSETS)
def test_gather_rows_and_chunks_copy_bits(width, so, do):
    g = torch.Generator(device=DEV).manual_seed(width + 16 * so + 4 * do)
    src = Carved(SRC_ROWS * width, so, _values(SRC_ROWS * width, width))
    table = src.t.view(SRC_ROWS, width)
    rpt = _rows_per_tile(width, so, do)
    L = CHUNK["L"]
    for rows in (1, rpt, rpt + 1, 3 * rpt - 1):
        what = "width=%d off=(%d, %d) rows=%d" % (width, so, do, rows)
        _check_rows(src, width, do, rows, g, what)
        # chunk mode: L output rows per index (the count rounded up to a multiple of L), one first_only field alongside
        mb = (rows + L - 1) // L
        idx = torch.randint(0, SRC_ROWS // L, (mb,), device=DEV, generator=g)
        dst, first = Carved(mb * L * width, do), Carved(mb * width, do)
        assert _gather([(src.ptr(), dst.ptr(), width, 0, 0), (src.ptr(), first.ptr(), width, 1, 0)], idx, mb, CHUNK) == 0
        assert torch.equal(_bits(dst.t.view(mb * L, width)), _bits(table[chunk_map(idx, mb, **CHUNK)])), what
        assert torch.equal(_bits(first.t.view(mb, width)), _bits(table[chunk_map(idx, mb, first_only=True, **CHUNK)])), what
        assert dst.intact() and first.intact(), what
    # one workgroup per CU (256 workgroups): a ragged second trip of the tile loop
    old = _lib().mappo_gather_set_variant(5 | (1 << 4))
    try:
        _check_rows(src, width, do, 258 * rpt + 1, g, "width=%d off=(%d, %d) second trip" % (width, so, do))
    finally:
        _lib().mappo_gather_set_variant(old)
    assert src.intact()


@pytest.mark.parametrize("chunked", [False, True])
def test_gather_normalisation_against_the_host_oracle(chunked):
    """(v - mean) / (std + 1e-5f) in IEEE float32, as oracle.adv_normalize computes it on the host; widths 1 and 5 take the
    4-byte path, 2 and 4 the 8- and 16-byte ones."""
    g = torch.Generator(device=DEV).manual_seed(11)
    stats = torch.tensor(STATS, device=DEV)
    rows = 700
    mb = rows // CHUNK["L"] + 1 if chunked else rows
    idx = torch.randint(0, SRC_ROWS // CHUNK["L"] if chunked else SRC_ROWS, (mb,), device=DEV, generator=g)
    rows_map = chunk_map(idx, mb, **CHUNK) if chunked else idx
    widths = (1, 5, 2, 4)
    src = [Carved(SRC_ROWS * w, 0, _values(SRC_ROWS * w, 100 + w, nan=False)) for w in widths]
    dst = [Carved(rows_map.numel() * w) for w in widths]
    fields = [(s.ptr(), d.ptr(), w, 0, 1) for s, d, w in zip(src, dst, widths)]
    assert _gather(fields, idx, mb, CHUNK if chunked else None, stats) == 0
    for s, d, w in zip(src, dst, widths):
        picked = s.t.view(SRC_ROWS, w)[rows_map].cpu().numpy()
        exp = oracle.adv_normalize(picked, *STATS).reshape(-1, w)
        out = d.t.view(-1, w).cpu().numpy()
        assert np.array_equal(out.view(np.int32), exp.view(np.int32)), w
        assert d.intact(), w
    # normalize without stats is refused before anything is launched
    fresh = Carved(rows_map.numel())
    assert _gather([(src[0].ptr(), fresh.ptr(), 1, 0, 1)], idx, mb, CHUNK if chunked else None, None) == E_NULL
    torch.cuda.synchronize()
    assert _all_nan(fresh)


def test_gather_field_limit():
    g = torch.Generator(device=DEV).manual_seed(12)
    rows = 77
    idx = torch.randint(0, SRC_ROWS, (rows,), device=DEV, generator=g)
    widths = [GATHER_WIDTHS[k % 9] for k in range(17)]
    src = [Carved(SRC_ROWS * w, 0, _values(SRC_ROWS * w, 200 + k)) for k, w in enumerate(widths)]
    dst = [Carved(rows * w) for w in widths]
    fields = [(s.ptr(), d.ptr(), w, 0, 0) for s, d, w in zip(src, dst, widths)]
    assert _gather(fields, idx, rows) == E_TOO_MANY
    torch.cuda.synchronize()
    assert all(_all_nan(d) for d in dst)
    assert _gather(fields[:16], idx, rows) == 0
    for s, d, w in zip(src[:16], dst[:16], widths):
        assert torch.equal(_bits(d.t.view(rows, w)), _bits(s.t.view(SRC_ROWS, w)[idx])) and d.intact(), w
    assert _all_nan(dst[16])


def test_gather_hook_low_bits_do_not_matter():
    g = torch.Generator(device=DEV).manual_seed(13)
    rows, widths = 1500, (1, 6, 384)
    idx = torch.randint(0, SRC_ROWS, (rows,), device=DEV, generator=g)
    src = [Carved(SRC_ROWS * w, 0, _values(SRC_ROWS * w, 300 + w)) for w in widths]
    old = _lib().mappo_gather_set_variant(5)
    try:
        for variant in (0, 3, 5):
            assert _lib().mappo_gather_set_variant(variant) in (0, 3, 5)
            dst = [Carved(rows * w) for w in widths]
            assert _gather([(s.ptr(), d.ptr(), w, 0, 0) for s, d, w in zip(src, dst, widths)], idx, rows) == 0
            for s, d, w in zip(src, dst, widths):
                assert torch.equal(_bits(d.t.view(rows, w)), _bits(s.t.view(SRC_ROWS, w)[idx])) and d.intact(), (variant, w)
    finally:
        _lib().mappo_gather_set_variant(old)


# ------------------------------------------------------------------------------------------------ the packed records
RECORDS = [(4, (1, 1, 1, 1)), (12, (1, 5, 1, 1, 1, 1, 1, 1)), (16, (1, 5, 1, 1, 1, 1, 1, 1)), (32, (7, 8, 8, 8, 1))]


def _rec_fields(ptrs, widths, normalized, packing):
    from onpolicy import _native
    offs = np.concatenate([[0], np.cumsum(widths)[:-1]])
    return (_native.RecordField * len(widths))(*[
        _native.RecordField(p if packing else None, None if packing else p, w, int(o), int(k == normalized and not packing), 0)
        for k, (p, w, o) in enumerate(zip(ptrs, widths, offs))])


def _pack(src, widths, rw, rows):
    """-> the Carved records of ``rows`` source rows, checked against the concatenated fields with zero padding."""
    rec = Carved(rows * rw)
    rc = _lib().mappo_pack_records(_rec_fields([s.ptr() for s in src], widths, -1, True), len(widths), rec.ptr(), rw, rows,
                                   _stream())
    assert rc == 0, rc
    exp = torch.zeros(rows, rw, device=DEV)
    exp[:, :sum(widths)] = torch.cat([s.t.view(rows, w) for s, w in zip(src, widths)], dim=1)
    assert torch.equal(_bits(rec.t.view(rows, rw)), _bits(exp)) and rec.intact(), (rw, rows)
    return rec


def _check_records(rw, widths, out_rows, g, chunked=False):
    normalized = len(widths) - 1                # a width-1 field in every layout
    src = [Carved(SRC_ROWS * w, 0, _values(SRC_ROWS * w, 400 + rw + k, nan=(k != normalized))) for k, w in enumerate(widths)]
    rec = _pack(src, widths, rw, SRC_ROWS)
    stats = torch.tensor(STATS, device=DEV)
    for rows in out_rows:
        mb = (rows + CHUNK["L"] - 1) // CHUNK["L"] if chunked else rows
        n_out = mb * CHUNK["L"] if chunked else rows
        idx = torch.randint(0, SRC_ROWS // CHUNK["L"] if chunked else SRC_ROWS, (mb,), device=DEV, generator=g)
        geo = (CHUNK["L"], CHUNK["T"], CHUNK["N"], CHUNK["A"]) if chunked else (0, 1, 1, 1)
        dst = [Carved(n_out * w) for w in widths]
        rc = _lib().mappo_gather_records(rec.ptr(), rw, _rec_fields([d.ptr() for d in dst], widths, normalized, False),
                                         len(widths), idx.data_ptr(), mb, *geo, stats.data_ptr(), _stream())
        assert rc == 0, rc
        # the header's promise: bit-identical to gathering the fields one by one
        one = [Carved(n_out * w) for w in widths]
        fields = [(s.ptr(), d.ptr(), w, 0, int(k == normalized)) for k, (s, d, w) in enumerate(zip(src, one, widths))]
        assert _gather(fields, idx, mb, CHUNK if chunked else None, stats) == 0
        rows_map = chunk_map(idx, mb, **CHUNK) if chunked else idx
        for k, (s, d, o, w) in enumerate(zip(src, dst, one, widths)):
            what = "rw=%d rows=%d field=%d" % (rw, rows, k)
            assert torch.equal(_bits(d.t), _bits(o.t)), what
            assert d.intact() and o.intact(), what
            if k != normalized:
                assert torch.equal(_bits(d.t.view(n_out, w)), _bits(s.t.view(SRC_ROWS, w)[rows_map])), what
    assert rec.intact()


@pytest.mark.parametrize("rw,widths", RECORDS)
def test_records_equal_the_fields_gathered_one_by_one(rw, widths):
    g = torch.Generator(device=DEV).manual_seed(rw)
    _check_records(rw, widths, (1, 255, 256, 257), g)


def test_records_chunk_mode():
    _check_records(12, RECORDS[1][1], (257,), torch.Generator(device=DEV).manual_seed(14), chunked=True)


def test_records_second_trip_of_the_gather_grid():
    _check_records(32, RECORDS[3][1], (1280 * 256 + 300,), torch.Generator(device=DEV).manual_seed(15))


def test_pack_second_trip_of_its_grid():
    rows, widths = 256 * 8 * 256 + 257, (1, 1, 1, 1)
    _pack([Carved(rows * w, 0, _values(rows * w, 500 + k)) for k, w in enumerate(widths)], widths, 4, rows)
