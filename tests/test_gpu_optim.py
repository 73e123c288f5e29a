"""-m gpu: K13 (mappo_clip_adam): gradient clipping + Adam of one network as two launches, against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (the calls of the reference's ppo_update, r_mappo.py:146-167;
optimiser of rMAPPOPolicy.py:31-37) on the same tensors over several steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nets(seed, shapes, dev):
    g = torch.Generator().manual_seed(seed)
    make = lambda: [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    g.manual_seed(seed)
    a = make()
    g.manual_seed(seed)
    b = make()
    return a, b


@pytest.mark.parametrize("max_norm,wd", [(10.0, 0.0), (0.05, 0.0), (None, 0.0), (0.5, 0.01)])
def test_clip_adam_matches_torch(max_norm, wd):
    from onpolicy.algorithms.utils import fused_optim
    dev = torch.device("cuda", 0)
    shapes = [(64, 48), (64,), (64,), (64,), (64, 64), (64,), (5, 64), (5,), (192, 64), (3, 1000, 7)]
    pa, pb = _nets(3, shapes, dev)
    kw = dict(lr=7e-4, eps=1e-5, weight_decay=wd)
    oa = torch.optim.Adam(pa, fused=True, **kw)
    ob = torch.optim.Adam(pb, fused=True, **kw)
    g = torch.Generator().manual_seed(11)
    for step in range(5):
        grads = [torch.randn(s, generator=g).to(dev) * (0.1 if step % 2 else 3.0) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        if step == 3:
            for o in (oa, ob):
                o.param_groups[0]["lr"] = 3e-4          # lr_decay between updates
        assert fused_optim.supported(oa, pa)
        na = fused_optim.clip_and_step(oa, pa, max_norm)
        if max_norm:
            nb = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        else:
            nb = torch.sqrt(sum(q.grad.norm() ** 2 for q in pb))
        ob.step()
        torch.testing.assert_close(na, nb.reshape(()), rtol=2e-6, atol=0)
        for i, (p, q) in enumerate(zip(pa, pb)):
            torch.testing.assert_close(p.grad, q.grad, rtol=2e-6, atol=1e-9, msg="grad %d step %d" % (i, step))
            torch.testing.assert_close(p.data, q.data, rtol=3e-7, atol=1e-8, msg="param %d step %d" % (i, step))      # ~2 ulp
            for k in ("exp_avg", "exp_avg_sq", "step"):     # (sums that can cancel: absolute floor of a few ulp of the terms)
                torch.testing.assert_close(oa.state[p][k], ob.state[q][k], rtol=2e-6, atol=3e-7, msg=k)
    # the state is torch.optim.Adam's own: a plain step() continues from it
    for p, q in zip(pa, pb):
        p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    oa.step()
    ob.step()
    for p, q in zip(pa, pb):
        torch.testing.assert_close(p.data, q.data, rtol=5e-7, atol=1e-8)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_gradient_norm_behaves_like_clip_grad_norm(bad):
    """torch.nn.utils.clip_grad_norm_ (error_if_nonfinite=False): a NaN norm makes the clip coefficient NaN and poisons
    EVERY gradient; an infinite norm gives coefficient 0 (finite entries -> 0, the infinite one -> NaN).  The kernel must
    not quietly map a NaN coefficient to 1 and step on unclipped gradients."""
    from onpolicy.algorithms.utils import fused_optim
    dev = torch.device("cuda", 0)
    shapes = [(64, 48), (64,), (5, 64)]
    pa, pb = _nets(5, shapes, dev)
    oa = torch.optim.Adam(pa, fused=True, lr=7e-4, eps=1e-5)
    g = torch.Generator().manual_seed(12)
    grads = [torch.randn(s, generator=g).to(dev) for s in shapes]
    grads[1][7] = bad
    for p, q, gr in zip(pa, pb, grads):
        p.grad, q.grad = gr.clone(), gr.clone()
    na = fused_optim.clip_and_step(oa, pa, 10.0)
    nb = torch.nn.utils.clip_grad_norm_(pb, 10.0)
    torch.testing.assert_close(na, nb.reshape(()), rtol=0, atol=0, equal_nan=True)
    for i, (p, q) in enumerate(zip(pa, pb)):
        torch.testing.assert_close(p.grad, q.grad, rtol=0, atol=0, equal_nan=True, msg="grad %d" % i)
    if bad != bad:
        assert all(torch.isnan(p.grad).all() for p in pa)


def test_unsupported_optimisers_fall_back():
    from onpolicy.algorithms.utils import fused_optim
    dev = torch.device("cuda", 0)
    p = [torch.nn.Parameter(torch.randn(4, 4, device=dev))]
    p[0].grad = torch.randn(4, 4, device=dev)
    assert not fused_optim.supported(torch.optim.Adam(p, amsgrad=True), p)
    assert not fused_optim.supported(torch.optim.SGD(p, lr=0.1), p)
    q = [torch.nn.Parameter(torch.randn(4, 4, device=dev))]
    assert not fused_optim.supported(torch.optim.Adam(q), q)        # no gradient


def test_fused_valuenorm_update_matches_the_tensor_ops():
    """mappo_valuenorm_update (ValueNorm.update + running_mean_var, valuenorm.py:32-55) against the same module on the
    CPU: statistics and the [sigma, mu] pair after several batches, local batches and given (all-reduced) moments; the
    cached pair is dropped as soon as somebody edits the statistics."""
    from onpolicy.utils.valuenorm import ValueNorm
    dev = torch.device("cuda", 0)
    a, b = ValueNorm(1, device=dev), ValueNorm(1)
    g = torch.Generator().manual_seed(2)
    for i in range(6):
        x = torch.randn(100003 if i % 2 else 257, 1, generator=g) * (3.0 + i) + 1.5
        if i == 4:
            mom = (x.mean(0), (x ** 2).mean(0))
            a.update(None, batch_moments=tuple(t.to(dev) for t in mom))
            b.update(None, batch_moments=mom)
        else:
            a.update(x.to(dev))
            b.update(x)
        assert a._denorm_key is not None
        for name in ("running_mean", "running_mean_sq", "debiasing_term"):
            torch.testing.assert_close(getattr(a, name).cpu(), getattr(b, name), rtol=2e-5, atol=1e-10, msg=name)
        torch.testing.assert_close(a.denorm_scalars().cpu(), b.denorm_scalars(), rtol=2e-5, atol=1e-8)
        torch.testing.assert_close(a.normalize(x.to(dev)).cpu(), b.normalize(x), rtol=1e-4, atol=1e-5)
    a.running_mean.fill_(7.0)       # an in-place edit: the cached pair must not be served any more
    b.running_mean.fill_(7.0)
    torch.testing.assert_close(a.denorm_scalars().cpu(), b.denorm_scalars(), rtol=2e-5, atol=1e-8)


@pytest.mark.parametrize("policy_masked,value_masked", [(True, True), (True, False), (False, False)])
def test_minibatch_scales_match_the_tensor_ops(policy_masked, value_masked):
    """mappo_minibatch_sums / mappo_minibatch_scales (DataParallel.minibatch_scales: loss denominators of r_mappo.py:135-139,
    :84-87 and the returns' batch moments of :65) against float64 tensor arithmetic, one rank."""
    from onpolicy.utils.dist import DataParallel
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    for n in (1, 257, 1_000_003):
        active = (torch.rand(n, 1, generator=g) > 0.3).float()
        active[0] = 1.0
        ret = torch.randn(n, 1, generator=g) * 4.0 + 2.0
        dp = DataParallel(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), dev)
        out = dp.minibatch_scales(active.to(dev), ret.to(dev), policy_masked, value_masked)
        assert out is not None and out.shape == (8,)
        a, r = active.double(), ret.double()
        den_p = a.sum() if policy_masked else float(n)
        den_v = a.sum() if value_masked else float(n)
        want = torch.tensor([1 / den_p, 1 / den_v, 1 / den_p, 1 / den_p, 1 / den_v, 1 / n, r.mean(), (r * r).mean()])
        torch.testing.assert_close(out.cpu().double(), want, rtol=3e-7, atol=0)
    # columns that do not qualify fall back to the tensor ops
    assert dp.minibatch_scales(active.to(dev).double(), ret.to(dev), True, True) is None


@pytest.mark.parametrize("din,ld", [(48, 48), (30, 32), (435, 436), (7, 8)])
def test_fold_input_norm_kernels_match_autograd(din, ld):
    """mappo_fold_input_norm_forward / _backward (the input LayerNorm's affine half folded into the first Linear,
    mlp.py:47-48 + :20) against the tensor expression they replace, values and all four gradients."""
    from onpolicy.algorithms.utils.fused_mlp import _FoldInputNormFn
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(din)
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
    w, b, gamma, beta = mk(64, din), mk(64), mk(din), mk(din)
    wf, bf = _FoldInputNormFn.apply(w, b, gamma, beta, ld)
    ref = [t.detach().double().requires_grad_(True) for t in (w, b, gamma, beta)]
    wr = torch.nn.functional.pad(ref[0] * ref[2], (0, ld - din))
    br = ref[1] + ref[0] @ ref[3]
    torch.testing.assert_close(wf.double(), wr.detach(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(bf.double(), br.detach(), rtol=1e-5, atol=1e-5)
    dwf, dbf = torch.randn(64, ld, generator=g).to(dev), torch.randn(64, generator=g).to(dev)
    torch.autograd.backward([wf, bf], [dwf, dbf])
    torch.autograd.backward([wr, br], [dwf.double(), dbf.double()])
    for got, want, name in zip((w, b, gamma, beta), ref, ("w", "b", "gamma", "beta")):
        torch.testing.assert_close(got.grad.double(), want.grad, rtol=2e-5, atol=2e-5, msg=name)


# ------------------------------------------------------------------------------------------------------------------
# K13 and the moment launches at the sizes where their grids are capped.
import loss_reference as lr      # noqa: E402  (the 4 x judge and its record)

JUDGE = lr.Judge()
# floors of the 4 x judge relative to the tensor's scale: ~3 x the largest kernel error measured on the MI355X
# (profiles/small_kernel_margins.json); never raised to make a case pass
FLOOR = {"k13.param": 1.5e-7, "k13.exp_avg": 3e-7, "k13.exp_avg_sq": 3.5e-7, "k13.norm": 1.5e-7}
# mappo_clip_adam: kMaxBlocks = 256 blocks of 256 threads x 8 elements; the one-block fold of the second launch reads exactly
# that many partials.  A changed cap has to change these numbers too.
ADAM_BLOCK, ADAM_CAP = 256 * 8, 256
ADAM_EDGE = ADAM_BLOCK * ADAM_CAP
# mappo_valuenorm_update / mappo_minibatch_sums: kMaxSumBlocks = 1024 blocks of 256 threads x 16 elements
SUM_BLOCK, SUM_CAP = 256 * 16, 1024
SUM_SIZES = (SUM_BLOCK * SUM_CAP + 3 * SUM_BLOCK + 5, 13_107_200)


@pytest.fixture(autouse=True, scope="module")
def _record_margins():
    yield
    JUDGE.dump()


def _sixty_four_shapes(total):
    """64 tensors with ``total`` elements: five of one element, small vectors, matrices, and one large tensor in the middle
    that takes up the rest (so the blocks' element ranges cross tensor borders everywhere)."""
    small = [(1,), (1,), (64,), (1, 1), (512,), (64, 64), (1,), (7, 9), (4096,), (1,)] + [(64,), (33, 5), (512,)] * 7
    tail = [(48, 64), (5, 64), (5,), (1000,)] * 8
    shapes = small + [None] + tail
    assert len(shapes) == 64
    used = sum(int(torch.Size(s).numel()) for s in shapes if s is not None)
    shapes[len(small)] = (total - used,)
    assert total - used > 0 and sum(int(torch.Size(s).numel()) for s in shapes) == total
    assert sum(1 for s in shapes if torch.Size(s).numel() == 1) >= 5
    return shapes


def _adam64(p, g, m, v, step, *, lr_, b1, b2, eps, wd, max_norm):
    """One clip + Adam step in float64 from float32 state (torch.optim.Adam, no amsgrad; clip_grad_norm_)."""
    g = [x.double() for x in g]
    norm = torch.sqrt(sum((x * x).sum() for x in g))
    coef = min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm else 1.0
    outs = []
    for w, x, mm, vv in zip(p, g, m, v):
        w, mm, vv = w.double(), mm.double(), vv.double()
        x = x * coef
        if wd:
            x = x + wd * w
        mm = b1 * mm + (1 - b1) * x
        vv = b2 * vv + (1 - b2) * x * x
        denom = vv.sqrt() / (1 - b2 ** step) ** 0.5 + eps
        outs.append((w - lr_ / (1 - b1 ** step) * mm / denom, mm, vv))
    return norm, outs


@pytest.mark.parametrize("total,max_norm,wd", [
    (ADAM_EDGE - ADAM_BLOCK, 0.5, 0.0),         # 255 blocks: one short of the fold's width
    (ADAM_EDGE, 0.5, 0.0),                      # 256 blocks of exactly 2048 elements
    (ADAM_EDGE + ADAM_BLOCK, 0.5, 0.0),         # capped: 256 blocks of 2056
    (ADAM_EDGE + ADAM_BLOCK, None, 0.0),
    (1_500_003, 0.5, 0.0), (1_500_003, 10000.0, 0.01), (1_500_003, 0.5, 0.01)])
def test_clip_adam_at_the_grid_cap_against_float64(total, max_norm, wd):
    """64 tensors (the most the launch takes) around and beyond the capped grid: the second step of a run, by the kernel and
    by torch's fused Adam from the same state, both judged against a float64 step."""
    from onpolicy.algorithms.utils import fused_optim
    dev = torch.device("cuda", 0)
    assert fused_optim._native.lib().mappo_adam_workspace_floats() == ADAM_CAP
    shapes = _sixty_four_shapes(total)
    pa, pb = _nets(total % 1000, shapes, dev)
    kw = dict(lr=7e-4, eps=1e-5, weight_decay=wd)
    oa, ob = torch.optim.Adam(pa, fused=True, **kw), torch.optim.Adam(pb, fused=True, **kw)
    g = torch.Generator().manual_seed(total % 977)
    for step in (1, 2):
        grads = [torch.randn(s, generator=g).to(dev) * (0.02 if step == 1 else 1.0) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        if step == 1:                       # both optimisers take torch's step: identical state to start from
            oa.step()
            ob.step()
            for p, q in zip(pa, pb):
                assert torch.equal(p.data, q.data) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
            continue
        before = [(p.data.clone(), oa.state[p]["exp_avg"].clone(), oa.state[p]["exp_avg_sq"].clone()) for p in pa]
        norm64, want = _adam64([b[0] for b in before], grads, [b[1] for b in before], [b[2] for b in before], 2,
                               lr_=kw["lr"], b1=0.9, b2=0.999, eps=kw["eps"], wd=wd, max_norm=max_norm)
        assert fused_optim.supported(oa, pa)
        na = fused_optim.clip_and_step(oa, pa, max_norm)
        if max_norm:
            nb = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        else:
            nb = torch.sqrt(sum(q.grad.norm() ** 2 for q in pb))
        ob.step()
        what = "total=%d max_norm=%s wd=%g" % (total, max_norm, wd)
        JUDGE.check("k13.norm", na, nb.reshape(()), norm64, FLOOR["k13.norm"], what=what)
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
        for name, i in (("param", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
            mine = cat([p.data if i == 0 else oa.state[p][name] for p in pa])
            theirs = cat([q.data if i == 0 else ob.state[q][name] for q in pb])
            JUDGE.check("k13." + name, mine, theirs, cat([w[i] for w in want]), FLOOR["k13." + name], what=what)
        # the parameters moved (the judge is on the scale of the parameters: look at the step itself too)
        moved = cat([p.data for p in pa]).double() - cat([b[0] for b in before]).double()
        moved_t = cat([q.data for q in pb]).double() - cat([b[0] for b in before]).double()
        moved_64 = cat([w[0] for w in want]) - cat([b[0] for b in before]).double()
        assert float(moved_64.abs().max()) > 1e-4
        e_mine, e_theirs = JUDGE.errors(moved, moved_t, moved_64)
        # (floor: the step is read off float32 parameters -- one ulp of the largest of them, relative to the largest step)
        ulp = 2.0 ** -23 * float(cat([b[0] for b in before]).abs().max()) / float(moved_64.abs().max())
        print("step itself: kernel %.3e torch32 %.3e floor %.3e" % (e_mine, e_theirs, ulp))
        assert e_mine <= 4 * e_theirs + ulp, (what, e_mine, e_theirs, ulp)
        for p, q in zip(pa, pb):
            assert float(oa.state[p]["step"]) == 2.0 == float(ob.state[q]["step"])


def test_clip_adam_refuses_a_65th_tensor():
    from onpolicy.algorithms.utils import fused_optim
    dev = torch.device("cuda", 0)
    for n, ok in ((64, True), (65, False)):
        ps = [torch.nn.Parameter(torch.randn(3, device=dev)) for _ in range(n)]
        for p in ps:
            p.grad = torch.randn(3, device=dev)
        assert fused_optim.supported(torch.optim.Adam(ps, fused=True), ps) == ok


@pytest.mark.parametrize("total", [100_000, ADAM_EDGE + ADAM_BLOCK])
def test_clip_adam_lr_device_is_the_same_rate(total):
    """``lr_device`` (the rate a captured launch reads from the device) gives bit for bit what the same rate passed as ``lr``
    gives -- also after the device value changed between two steps -- and it is the device value that counts."""
    from onpolicy.algorithms.utils import fused_optim
    dev = torch.device("cuda", 0)
    shapes = _sixty_four_shapes(total)
    pa, pb = _nets(8, shapes, dev)
    oa = torch.optim.Adam(pa, fused=True, lr=1.0, eps=1e-5)             # a rate the kernel must NOT use
    ob = torch.optim.Adam(pb, fused=True, lr=7e-4, eps=1e-5)
    lr_dev = torch.tensor([7e-4], dtype=torch.float64, device=dev)
    g = torch.Generator().manual_seed(21)
    for step, rate in enumerate((7e-4, 7e-4, 3.1e-4, 1.3e-5)):
        lr_dev.fill_(rate)
        ob.param_groups[0]["lr"] = rate
        grads = [torch.randn(s, generator=g).to(dev) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        na = fused_optim.clip_and_step(oa, pa, 0.5, lr_device=lr_dev)
        nb = fused_optim.clip_and_step(ob, pb, 0.5)
        assert torch.equal(na, nb)
        for p, q in zip(pa, pb):
            assert torch.equal(p.data, q.data) and torch.equal(p.grad, q.grad), step
            for k in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(oa.state[p][k], ob.state[q][k]), (k, step)


@pytest.mark.parametrize("n", SUM_SIZES)
def test_fused_valuenorm_update_beyond_the_grid_cap(n):
    """More elements than 1024 blocks of 4096 cover in one pass (every block loops; the fold walks 1024 partials 64 at a
    time), and the 13 M elements of the north star: against float64 sums, at the tolerance of the small cases."""
    from onpolicy.utils.valuenorm import ValueNorm
    assert n > SUM_BLOCK * SUM_CAP
    dev = torch.device("cuda", 0)
    vn = ValueNorm(1, device=dev)
    g = torch.Generator().manual_seed(n % 1000)
    # (a block-dependent offset: partials that differ, so that a fold which skips or repeats some is off by far more than 2e-5)
    x = torch.randn(n, 1, generator=g) * 3.0 + 1.5 + (torch.arange(n).reshape(n, 1) % 40960 >= 4096 * 3).float() * 2.0
    xd = x.double()
    beta = vn.beta
    m1 = m2 = d = 0.0
    for i in range(2):
        vn.update(x.to(dev) if i == 0 else (x * 0.5).to(dev))
        xs = xd if i == 0 else (x * 0.5).double()
        m1 = m1 * beta + float(xs.mean()) * (1 - beta)
        m2 = m2 * beta + float((xs * xs).mean()) * (1 - beta)
        d = d * beta + (1 - beta)
        assert vn._denorm_key is not None
        want = torch.tensor([m1, m2, d], dtype=torch.float64)
        got = torch.stack([vn.running_mean.reshape(()), vn.running_mean_sq.reshape(()), vn.debiasing_term.reshape(())])
        torch.testing.assert_close(got.cpu().double(), want, rtol=2e-5, atol=1e-10)
        mu = m1 / max(d, 1e-5)
        var = max(m2 / max(d, 1e-5) - mu * mu, 1e-2)
        torch.testing.assert_close(vn.denorm_scalars().cpu().double(), torch.tensor([var ** 0.5, mu], dtype=torch.float64),
                                   rtol=2e-5, atol=1e-8)


@pytest.mark.parametrize("n", SUM_SIZES)
@pytest.mark.parametrize("active_kind,policy_masked,value_masked", [("random", True, True), ("ones", False, True),
                                                                    ("ones", False, False), ("one", True, False)])
def test_minibatch_scales_beyond_the_grid_cap(n, active_kind, policy_masked, value_masked):
    from onpolicy.utils.dist import DataParallel
    assert n > SUM_BLOCK * SUM_CAP
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(n % 1000 + len(active_kind))
    if active_kind == "random":
        active = (torch.rand(n, 1, generator=g) > 0.3).float()
    elif active_kind == "ones":
        active = torch.ones(n, 1)
    else:                                   # a single active entry, in a later pass of its block
        active = torch.zeros(n, 1)
        active[SUM_BLOCK * SUM_CAP + SUM_BLOCK + 77] = 1.0
    ret = torch.randn(n, 1, generator=g) * 4.0 + 2.0 + (torch.arange(n).reshape(n, 1) % 40960 >= 4096 * 3).float() * 2.0
    dp = DataParallel(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), dev)
    out = dp.minibatch_scales(active.to(dev), ret.to(dev), policy_masked, value_masked)
    assert out is not None and out.shape == (8,)
    a, r = active.double(), ret.double()
    if active_kind == "one":
        assert float(a.sum()) == 1.0
    den_p = a.sum() if policy_masked else float(n)
    den_v = a.sum() if value_masked else float(n)
    want = torch.tensor([1 / den_p, 1 / den_v, 1 / den_p, 1 / den_p, 1 / den_v, 1 / n, r.mean(), (r * r).mean()])
    torch.testing.assert_close(out.cpu().double(), want, rtol=3e-7, atol=0)
