"""The reference side of the K7 device tests (tests/loss_reference.py) checked on its own, without a device: the float32
and float64 evaluations are the same expression, the input generator produces the rows the masked tests rely on, the
near-boundary rows that gradient comparisons leave out stay under the cap for every (actions, mode) the device tests use,
and the exact-tie table is what float32 autograd gives."""
import pytest
import torch

import loss_reference as lr

HP = dict(clip=0.2, huber_delta=0.8, entropy_coef=0.01, value_loss_coef=1.3)
NORM = (2.5, 0.7)
# rows of K7's multi-pass case: one pass of the capped grid (2048 workgroups of 256 rows) + three workgroups + 17 rows
MULTI_PASS_ROWS = 2048 * 256 + 3 * 256 + 17
# every (actions, mask, mode, rows) the device tests take gradients at against float64 (tests/test_gpu_fused_loss.py)
DEVICE_CASES = [(5, False, "plain", MULTI_PASS_ROWS), (19, True, "plain", MULTI_PASS_ROWS),
                (48, True, "plain", MULTI_PASS_ROWS), (77, True, "plain", MULTI_PASS_ROWS)] + \
               [(na, m, "plain", 4099) for na in (8, 9) for m in (False, True)] + \
               [(75, True, "plain", 4099), (76, True, "plain", 4099), (149, False, "plain", 4099),
                (150, False, "plain", 4099), (5, True, "wide", 4099), (19, True, "wide", 4099),
                (5, False, "wide", 4099), (19, False, "wide", 4099)]


def _loss_and_grads(inp, dtype, flags):
    d = lr.to(inp, dtype=dtype)
    logits = d["logits"].clone().requires_grad_(True)
    values = d["values"].clone().requires_grad_(True)
    norm = torch.tensor(NORM, dtype=dtype)
    pl, ent, vl, ratio = lr.torch_loss(logits, d["avail"], d["actions"], d["old_logp"], d["adv"], d["active"], d["factor"],
                                       values, d["value_preds"], d["returns"], norm, **lr.flag_kwargs(flags), **HP)
    (pl - ent * HP["entropy_coef"]).backward()
    (vl * HP["value_loss_coef"]).backward()
    return pl.detach(), ent.detach(), vl.detach(), ratio.detach(), logits.grad, values.grad


@pytest.mark.parametrize("flags", [0, 5, 10, 15])
def test_float32_and_float64_evaluate_the_same_expression(flags):
    inp = lr.make_inputs(4099, 19, with_avail=True, seed=1, with_factor=True)
    lo, hi = _loss_and_grads(inp, torch.float32, flags), _loss_and_grads(inp, torch.float64, flags)
    assert all(t.dtype == torch.float32 for t in lo) and all(t.dtype == torch.float64 for t in hi)
    for a, b in zip(lo[:3], hi[:3]):
        assert float(a) == pytest.approx(float(b), rel=1e-5, abs=1e-6)
    torch.testing.assert_close(lo[3].double(), hi[3], rtol=1e-5, atol=0)
    p_rows, v_rows = lr.near_boundary(inp, NORM, clip=HP["clip"], huber_delta=HP["huber_delta"])
    for a, b, rows in ((lo[4], hi[4], p_rows), (lo[5], hi[5], v_rows)):
        keep = ~rows
        err = (a.double() - b)[keep].abs().max() / b.abs().max()
        assert float(err) < 1e-5


@pytest.mark.parametrize("na,mode", [(5, "plain"), (19, "plain"), (77, "wide"), (2, "plain")])
def test_generator_masks_do_not_favour_action_zero(na, mode):
    inp = lr.make_inputs(20011, na, with_avail=True, mode=mode, seed=3)
    avail, actions = inp["avail"], inp["actions"].long()
    assert bool((avail.sum(-1) >= 1).all())
    assert bool((avail.gather(1, actions) == 1).all())                 # never an unavailable action
    assert float((avail[:, 0] == 0).float().mean()) > (0.2 if na > 2 else 0.15)
    single = avail.sum(-1) == 1
    assert 0.02 < float(single.float().mean()) < (0.2 if na > 2 else 0.5)
    where = avail[single].argmax(-1)
    assert len(torch.unique(where)) == na                              # the lone action sits at every index
    assert bool((actions[single].squeeze(-1) == where).all())
    # a different seed gives different inputs, the same seed the same ones
    again, other = lr.make_inputs(20011, na, with_avail=True, mode=mode, seed=3), \
        lr.make_inputs(20011, na, with_avail=True, mode=mode, seed=4)
    assert torch.equal(again["logits"], inp["logits"]) and not torch.equal(other["logits"], inp["logits"])


def test_wide_mode_is_wide_and_finite():
    inp = lr.make_inputs(4099, 19, with_avail=True, mode="wide", seed=0)
    d = lr.to(inp, dtype=torch.float32)
    logp = torch.log_softmax(lr.masked_logits(d["logits"], d["avail"]), -1).gather(1, d["actions"].long())
    ratio = torch.exp(logp - d["old_logp"])
    assert bool(torch.isfinite(ratio).all()) and float(ratio.max()) > 1e4 and float(ratio.min()) < 1e-4
    assert float(d["logits"].abs().max()) > 90 and float(d["adv"].abs().max()) > 2e3
    out = _loss_and_grads(inp, torch.float32, 15)
    assert all(bool(torch.isfinite(t).all()) for t in out)


@pytest.mark.parametrize("na,with_avail,mode,rows", DEVICE_CASES)
def test_near_boundary_share_stays_under_the_cap(na, with_avail, mode, rows):
    """The share of rows a gradient comparison against float64 may leave out is capped at 0.5 % per half; measured at
    525,073 rows it is ~0.05 % (policy) and ~0.15 % (value)."""
    inp = lr.make_inputs(rows, na, with_avail=with_avail, mode=mode, seed=0)
    p_rows, v_rows = lr.near_boundary(inp, NORM, clip=HP["clip"], huber_delta=HP["huber_delta"])
    p, v = float(p_rows.float().mean()), float(v_rows.float().mean())
    print("near-boundary share na=%d %s rows=%d: policy %.4f %% value %.4f %%" % (na, mode, rows, 100 * p, 100 * v))
    assert p <= lr.SKIP_CAP and v <= lr.SKIP_CAP
    if rows == MULTI_PASS_ROWS:                                        # (enough rows for the share to be a measurement)
        assert 0.0001 < p < 0.0012 and 0.0007 < v < 0.0025


@pytest.mark.parametrize("na", [5, 19])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_clear_rows_leave_nothing_to_skip(na, rows):
    """The row-count edge cases (1, 255, 256, 257 rows: 0.5 % of them is at most one row) take rows clear of every branch
    point, so nothing is skipped there."""
    pool = lr.make_inputs(1024, na, with_avail=True, seed=2)
    inp = lr.clear_rows(pool, rows, NORM, clip=HP["clip"], huber_delta=HP["huber_delta"])
    assert inp["logits"].shape == (rows, na) and inp["avail"].shape == (rows, na) and inp["values"].shape == (rows, 1)
    p_rows, v_rows = lr.near_boundary(inp, NORM, clip=HP["clip"], huber_delta=HP["huber_delta"])
    assert not bool(p_rows.any()) and not bool(v_rows.any())


def test_near_boundary_marks_what_it_should():
    z = lambda *v: torch.tensor(v, dtype=torch.float32).reshape(-1, 1)
    inp = dict(logits=torch.zeros(4, 2), avail=None, actions=z(0, 0, 0, 0),
               old_logp=torch.log(torch.tensor(0.5)) - torch.log(z(1.2, 0.8 + 5e-5, 1.0, 1.2 + 2e-4)),
               adv=z(1, 1, 1, 1), active=z(1, 1, 1, 1), factor=None,
               values=z(0.2 + 2e-5, 0.0, 0.8 - 5e-5, 0.1), value_preds=z(0, 0, 0.7, 0), returns=z(0, 0, 0, 0.3))
    p_rows, v_rows = lr.near_boundary(inp, None, clip=0.2, huber_delta=0.8)
    assert p_rows.tolist() == [True, True, False, False]
    assert v_rows.tolist() == [True, False, True, False]


@pytest.mark.parametrize("use_huber", [False, True])
@pytest.mark.parametrize("rows", [16, 64, 1024])
def test_tie_table_is_what_float32_autograd_gives(use_huber, rows):
    """On the rows of the tie table float32 autograd gives clamp's closed interval, the closed huber knee and half the
    gradient per argument of torch.max on a tie -- bit for bit the table's closed-form column, in float32 as in float64."""
    want = lr.tie_table(rows)[4 if use_huber else 3]
    got32, got64 = lr.tie_autograd(use_huber, rows), lr.tie_autograd(use_huber, rows, torch.float64)
    assert got32.dtype == torch.float32 and torch.equal(got32, want)
    assert torch.equal(got64, want.double())
    v, vp, ret, _, _ = lr.tie_table(rows)
    d = (v - vp).abs()
    assert int((d == lr.TIE_CLIP).sum()) >= 3 * (rows // 12)          # on the clip
    assert int(((ret - v).abs() == lr.TIE_DELTA).sum()) >= 3 * (rows // 12)      # on the knee
    assert int(((d > lr.TIE_CLIP) & (want != 0)).sum()) >= 3 * (rows // 12)
