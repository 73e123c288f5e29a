"""-m gpu: the fused PPO loss kernel (K7, mappo_ppo_loss_f32) against the same loss written with torch ops
and differentiated by autograd (a float32 torch reference of the op: r_mappo.py:52-89, :119-153), for every
flag combination, and the trainer with / without the fused path."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import loss_reference as lr
from helpers import Box, Discrete, make_args, fill_buffer_arrays, buffer_shapes, load_into
from loss_reference import torch_loss as _torch_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("na,with_avail,with_factor,with_norm", [(5, False, False, True), (5, True, True, False),
                                                                   (48, True, False, True), (64, False, False, True), (200, True, False, True),
                                                                  (19, True, False, True), (1, False, False, False),
                                                                  (38, False, True, True), (40, True, False, True)])
# (40 / 48 actions + mask: 84 / 100 KB of LDS, granted above 64 KB -- round 4; 200 + mask: wider than the staged variant takes)
def test_fused_loss_matches_autograd(na, with_avail, with_factor, with_norm):
    from onpolicy.algorithms.utils import fused_loss
    R = 10007
    g = torch.Generator(device="cpu").manual_seed(na * 7 + 1)
    rnd = lambda *s: torch.randn(*s, generator=g)
    logits0 = (rnd(R, na) * 2).to(DEV)
    avail = None
    if with_avail:
        avail = (torch.rand(R, na, generator=g) < 0.6).float()
        avail.scatter_(1, torch.randint(0, na, (R, 1), generator=g), 1.0)      # one available action, at a random index
        avail = avail.to(DEV)
    probs = torch.softmax(logits0 if avail is None else torch.where(avail == 0, torch.full_like(logits0, -1e10), logits0), -1)
    actions = torch.multinomial(probs.cpu(), 1, generator=g).float().to(DEV)
    old_logp = (torch.log(probs.gather(1, actions.long())) + rnd(R, 1).to(DEV) * 0.2)
    adv = rnd(R, 1).to(DEV)
    active = (torch.rand(R, 1, generator=g) < 0.8).float().to(DEV)
    factor = (torch.rand(R, 1, generator=g) + 0.5).to(DEV) if with_factor else None
    values0 = rnd(R, 1).to(DEV)
    value_preds = (values0 + rnd(R, 1).to(DEV) * 0.3)
    returns = (rnd(R, 1) * 3 + 1).to(DEV)
    norm = torch.tensor([2.5, 0.7], device=DEV) if with_norm else None
    hp = dict(clip=0.2, huber_delta=0.8, entropy_coef=0.01, value_loss_coef=1.3)
    for use_huber, use_clipped, p_active, v_active in itertools.product([True, False], repeat=4):
        logits = logits0.clone().requires_grad_(True)
        values = values0.clone().requires_grad_(True)
        pl, ent, vl, ratio = _torch_loss(logits, avail, actions, old_logp, adv, active, factor, values, value_preds,
                                         returns, norm, use_huber=use_huber, use_clipped=use_clipped,
                                         p_active=p_active, v_active=v_active, **hp)
        (pl - ent * hp["entropy_coef"]).backward()
        (vl * hp["value_loss_coef"]).backward()
        n = torch.tensor(float(R), device=DEV)
        inv = (1.0 / torch.stack([active.sum() if p_active else n, active.sum() if v_active else n])).contiguous()
        sums = torch.zeros(4, dtype=torch.float64, device=DEV)
        dlogits, dvalues = fused_loss.ppo_loss(
            logits.detach(), avail, actions, old_logp, adv, active, factor, values.detach(), value_preds, returns, norm,
            inv, sums, use_huber=use_huber, use_clipped_value_loss=use_clipped, policy_active_masks=p_active,
            value_active_masks=v_active, **hp)
        tag = (use_huber, use_clipped, p_active, v_active)
        s = sums.cpu().numpy()
        assert s[0] * float(inv[0]) == pytest.approx(float(pl.detach()), rel=2e-5, abs=1e-6), tag
        assert s[1] * float(inv[0]) == pytest.approx(float(ent.detach()), rel=2e-5, abs=1e-6), tag
        assert s[2] * float(inv[1]) == pytest.approx(float(vl.detach()), rel=2e-5, abs=1e-6), tag
        assert s[3] / R == pytest.approx(float(ratio.detach().mean()), rel=2e-5), tag
        scale = float(logits.grad.abs().max())
        np.testing.assert_allclose(dlogits.cpu().numpy(), logits.grad.cpu().numpy(), rtol=2e-4, atol=2e-6 * max(scale, 1e-3) + 1e-10,
                                   err_msg=str(tag))
        np.testing.assert_allclose(dvalues.cpu().numpy(), values.grad.cpu().numpy(), rtol=2e-5, atol=1e-10, err_msg=str(tag))
        if avail is not None:
            assert float(dlogits[avail == 0].abs().sum()) == 0.0


@pytest.mark.parametrize("recurrent", [False, True])
def test_trainer_fused_equals_unfused(monkeypatch, recurrent):
    """One train() with the fused loss and one without, from identical seeds: same logged scalars and
    parameters within float32 tolerance."""
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from onpolicy.algorithms.r_mappo.r_mappo import R_MAPPO
    from onpolicy.utils.shared_buffer import SharedReplayBuffer
    T, N, A, Do, Ds, na, H = 20, 16, 3, 6, 18, 5, 16
    results = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MAPPO_FUSED_LOSS", flag)
        args = make_args(episode_length=T, n_rollout_threads=N, hidden_size=H, ppo_epoch=3, num_mini_batch=2,
                         use_recurrent_policy=recurrent, data_chunk_length=5, sampler_rng="host",
                         algorithm_name="rmappo" if recurrent else "mappo")
        spaces = Box((Do,)), Box((Ds,)), Discrete(na)
        torch.manual_seed(5)
        policy = R_MAPPOPolicy(args, *spaces, device=DEV)
        trainer = R_MAPPO(args, policy, device=DEV)
        assert trainer._fused_loss == (flag == "1")
        buf = SharedReplayBuffer(args, A, *spaces, device=DEV)
        arrays = fill_buffer_arrays(buffer_shapes(T, N, A, Do, Ds, na, H), np.random.default_rng(3), na=na)
        load_into(buf, arrays)
        buf.compute_returns(arrays["next_value"], trainer.value_normalizer)
        trainer.prep_training()
        torch.manual_seed(9)
        info = trainer.train(buf)
        results.append((info, [p.detach().clone() for p in policy.actor.parameters()],
                        [p.detach().clone() for p in policy.critic.parameters()],
                        trainer.value_normalizer.running_mean.clone()))
    (i1, a1, c1, n1), (i0, a0, c0, n0) = results
    for k in i0:
        assert i1[k] == pytest.approx(i0[k], rel=2e-4, abs=2e-6), (k, i1[k], i0[k])
    for p, q in zip(a1 + c1, a0 + c0):
        np.testing.assert_allclose(p.cpu().numpy(), q.cpu().numpy(), rtol=1e-4, atol=2e-5)
    assert torch.allclose(n1, n0, rtol=1e-6, atol=1e-10)


@pytest.mark.parametrize("cname", ["mlp", "gru"])
def test_row_span_microbatching_is_equivalent_on_device(gold, cname):
    """The device twin of tests/test_networks_trainer_cpu.py::test_row_span_microbatching_is_equivalent: the fused loss (K7)
    evaluated in several row spans -- rows for the feed-forward case, whole chunks for the recurrent one -- accumulates
    gradients and the four sums into the same update as one pass, to the CPU test's own tolerances.  Several spans stay
    eager: nothing of such a minibatch is replayed from a graph."""
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from onpolicy.algorithms.r_mappo.r_mappo import R_MAPPO
    from onpolicy.utils.shared_buffer import SharedReplayBuffer
    z = gold.npz("trainer_cases")
    key = "trn_%s_" % cname
    spec = gold.meta("trainer_cases")[cname]["spec"]
    # 200 elements / 11 features -> at most 18 rows (3 chunks of 5 steps) per span, 60 rows (12 chunks) per minibatch
    rows = spec["T"] * spec["N"] * spec["A"] // spec["args"]["num_mini_batch"]
    per_span = 200 // max(spec["Do"], spec["Ds"])
    if cname == "gru":
        per_span = per_span // spec["args"]["data_chunk_length"] * spec["args"]["data_chunk_length"]
    assert -(-rows // per_span) >= 3
    results = []
    for cap in (1 << 30, 200):
        args = make_args(episode_length=spec["T"], n_rollout_threads=spec["N"], sampler_rng="host", **spec["args"])
        spaces = Box((spec["Do"],)), Box((spec["Ds"],)), Discrete(spec["na"])
        torch.manual_seed(1)
        np.random.seed(1)
        policy = R_MAPPOPolicy(args, *spaces, device=DEV)
        trainer = R_MAPPO(args, policy, device=DEV)
        assert trainer._fused_loss
        trainer.MAX_TENSOR_ELEMENTS = cap
        buf = SharedReplayBuffer(args, spec["A"], *spaces, device=DEV)
        for name in ("share_obs", "obs", "rnn_states", "rnn_states_critic", "actions", "value_preds", "masks",
                     "bad_masks", "active_masks", "action_log_probs", "available_actions", "rewards"):
            dst = getattr(buf, name)
            if dst.stride()[0] != 0:
                dst.copy_(torch.from_numpy(z[key + "buf_" + name]))
        buf.compute_returns(z[key + "next_value"], trainer.value_normalizer)
        trainer.prep_training()
        torch.manual_seed(21)
        info = trainer.train(buf)
        if cap == 200:
            assert trainer._update_graph.replays == 0
        results.append((info, {k: v.cpu() for k, v in policy.actor.state_dict().items()},
                        {k: v.cpu() for k, v in policy.critic.state_dict().items()}))
    (i0, a0, c0), (i1, a1, c1) = results
    for k in i0:
        print("row spans on device %s %s: %.9g one pass, %.9g in spans" % (cname, k, i0[k], i1[k]))
        assert i1[k] == pytest.approx(i0[k], rel=1e-4, abs=1e-6), k
    for sd0, sd1 in ((a0, a1), (c0, c1)):
        for k in sd0:
            np.testing.assert_allclose(sd1[k].numpy(), sd0[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("na,with_avail", [(5, False), (5, True), (18, True), (48, True), (1, False)])
def test_categorical_sample_kernel_vs_the_framework_rule(na, with_avail):
    """K14 (``mappo_categorical_sample``): masking + one draw per row + its log-probability in one launch, against the
    framework formulas on the SAME Exponential(1) noise (torch.multinomial's rule for one sample: argmax p / q; reference
    distributions.py:14-28, :55-68).  Actions identical, log-probs to float32 rounding; the empirical action frequencies of
    many draws match the probabilities."""
    from onpolicy.algorithms.utils import distributions, fused_loss
    dev = torch.device("cuda", 0)
    distributions.set_sampling_rng("device")
    g = torch.Generator(device=dev).manual_seed(na)
    rows = 4099
    logits = torch.randn(rows, na, device=dev, generator=g) * 2.0
    avail = None
    if with_avail:
        avail = (torch.rand(rows, na, device=dev, generator=g) < 0.7).float()
        avail[:, 0] = 1.0
    with torch.no_grad():
        assert fused_loss.sample_supported(logits)
        torch.manual_seed(123)
        actions, logp = fused_loss.sample_categorical(logits, avail)
        torch.manual_seed(123)
        noise = torch.empty_like(logits).exponential_(1.0)
    x = logits if avail is None else torch.where(avail == 0, torch.full_like(logits, -1e10), logits)
    ref_l = x - x.logsumexp(-1, keepdim=True)
    ref_a = (ref_l.exp() / noise).argmax(-1, keepdim=True)
    assert actions.shape == (rows, 1) and actions.dtype == torch.int64 and logp.shape == (rows, 1)
    same = (actions == ref_a)
    # (a near-tie of p / q can flip under expf's last bit: allow a handful, and require equal probabilities there)
    assert same.float().mean() > 0.999
    torch.testing.assert_close(logp[same.squeeze(-1)], ref_l.gather(-1, ref_a)[same.squeeze(-1)], rtol=1e-5, atol=1e-6)
    if avail is not None:
        assert bool((avail.gather(-1, actions) == 1).all())             # never an unavailable action
    # frequencies: one row's distribution sampled 20 000 times
    if na > 1:
        row = logits[:1].expand(20000, na).contiguous()
        with torch.no_grad():
            a, _ = fused_loss.sample_categorical(row, None)
        freq = torch.bincount(a.reshape(-1), minlength=na).float() / 20000
        torch.testing.assert_close(freq, torch.softmax(logits[0], -1), rtol=0, atol=0.015)


# ------------------------------------------------------------------------------------------------------------------
# K7 at full size and at its edges, judged against float64.  Both float32 results -- the kernel's and the same torch
# expression's on the device -- are measured against the float64 evaluation of tests/loss_reference.py; the kernel gets
# 4 x torch's error + a floor (the idiom of the LayerNorm kernels, test_gpu_parity.py), per tensor on its max-abs scale,
# the four sums on sum |per-row term|.  Gradient rows within 1e-4 of a branch point (loss_reference.near_boundary) are
# left out, at most 0.5 % per half.
HP = dict(clip=0.2, huber_delta=0.8, entropy_coef=0.01, value_loss_coef=1.3)
NORM = (2.5, 0.7)
# K7's grid is capped at kCUs * 8 = 2048 workgroups of 256 rows (mappo_ppo_loss_f32): one full pass of the capped grid, three
# more workgroups and a ragged tail of 17 rows.  A changed cap has to change this number too.
GRID_CAP_BLOCKS, BLOCK_ROWS = 256 * 8, 256
MULTI_PASS_ROWS = GRID_CAP_BLOCKS * BLOCK_ROWS + 3 * BLOCK_ROWS + 17
# floors of the 4 x judge, relative to the tensor's scale: ~3 x the largest kernel error measured on the MI355X
# (profiles/small_kernel_margins.json holds the measurements); never raised to make a case pass
# (wide-mode dlogits: the kernel's largest error is 1.9e-5 where torch's is 2.1e-4, so its floor stays at the 1e-5 it began at)
FLOOR = {"k7.dlogits": 2e-6, "k7.dlogits.wide": 1e-5, "k7.dvalues": 1.2e-6, "k7.sums": 2.5e-6}
JUDGE = lr.Judge()
SUM_NAMES = ("policy", "entropy", "value", "ratio")


@pytest.fixture(autouse=True, scope="module")
def _record_margins():
    yield
    JUDGE.dump()


def _device_inputs(inp):
    return lr.to(inp, device=DEV)


def _inv_denoms(d, flags):
    rows = d["active"].shape[0]
    act = float(d["active"].double().sum())
    den_p = act if flags & 4 else float(rows)
    den_v = act if flags & 8 else float(rows)
    return torch.tensor([1.0 / den_p, 1.0 / den_v], dtype=torch.float32, device=DEV), den_p, den_v


def _k7(d, flags, inv, *, norm=None, hp=HP, lo=0, hi=None, sums=None, out=None, drop=()):
    """One ``mappo_ppo_loss_f32`` launch straight through the ABI on rows [lo, hi) of the device inputs ``d``; the names in
    ``drop`` are passed as NULL.  -> (dlogits, dvalues, sums): full-height tensors pre-filled with NaN (``out`` to write
    into the ones of an earlier call), float64[4] sums (``sums`` to accumulate into an earlier call's)."""
    from onpolicy import _native
    rows, na = d["logits"].shape
    hi = rows if hi is None else hi
    if out is None:
        out = (torch.full((rows, na), float("nan"), device=DEV), torch.full((rows, 1), float("nan"), device=DEV))
    if sums is None:
        sums = torch.zeros(4, dtype=torch.float64, device=DEV)

    def at(t, name=None):
        if t is None or name in drop:
            return None
        assert t.is_contiguous() and t.dtype in (torch.float32, torch.float64)
        return t.data_ptr() + lo * (t.shape[1] if t.dim() == 2 else 1) * t.element_size()
    p = _native.ptr
    a = _native.PPOLoss(at(d["logits"], "logits"), at(d["avail"]), at(d["actions"]), at(d["old_logp"]), at(d["adv"]),
                        at(d["active"], "active"), at(d["factor"]), at(d["values"], "values"), at(d["value_preds"]),
                        at(d["returns"]), p(norm), p(inv), at(out[0], "dlogits"), at(out[1], "dvalues"),
                        None if "sums" in drop else p(sums), hi - lo, na, hp["clip"], hp["huber_delta"],
                        hp["entropy_coef"], hp["value_loss_coef"], flags)
    _native.check(_native.lib().mappo_ppo_loss_f32(ctypes.byref(a), _native.stream_of(DEV)), "mappo_ppo_loss_f32")
    torch.cuda.synchronize()
    return out[0], out[1], sums


def _reference(d, dtype, flags, norm, hp=HP):
    """``torch_loss`` and its autograd gradients in ``dtype`` on the device -> dict."""
    x = lr.to(d, dtype=dtype)
    logits = x["logits"].clone().requires_grad_(True)
    values = x["values"].clone().requires_grad_(True)
    n = None if norm is None else norm.to(dtype)
    terms = {}
    pl, ent, vl, ratio = _torch_loss(logits, x["avail"], x["actions"], x["old_logp"], x["adv"], x["active"], x["factor"],
                                     values, x["value_preds"], x["returns"], n, terms=terms, **lr.flag_kwargs(flags), **hp)
    (pl - ent * hp["entropy_coef"]).backward()
    (vl * hp["value_loss_coef"]).backward()
    return dict(policy=pl.detach(), entropy=ent.detach(), value=vl.detach(), ratio=ratio.detach().sum(),
                dlogits=logits.grad, dvalues=values.grad, terms=terms)


def _judge_against_float64(d, flags, norm_pair, tag, skip=True, outputs=None):
    """The kernel and float32 torch on the inputs ``d``, both against float64 -> the kernel's (dlogits, dvalues, sums) and
    the reordering bound of the sums (1e-12 * sum |per-row term|)."""
    norm = None if norm_pair is None else torch.tensor(norm_pair, dtype=torch.float32, device=DEV)
    rows = d["logits"].shape[0]
    inv, den_p, den_v = _inv_denoms(d, flags)
    dlogits, dvalues, sums = outputs if outputs is not None else _k7(d, flags, inv, norm=norm)
    r64 = _reference(d, torch.float64, flags, norm)
    r32 = _reference(d, torch.float32, flags, norm)
    keep_p = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep_v = keep_p.clone()
    if skip:
        p_rows, v_rows = lr.near_boundary(lr.to(d, device="cpu"), norm_pair, clip=HP["clip"], huber_delta=HP["huber_delta"])
        share_p, share_v = float(p_rows.float().mean()), float(v_rows.float().mean())
        print("skipped near-boundary rows %s: policy %.4f %% value %.4f %%" % (tag, 100 * share_p, 100 * share_v))
        assert share_p <= lr.SKIP_CAP and share_v <= lr.SKIP_CAP, (tag, share_p, share_v)
        keep_p, keep_v = ~p_rows.to(DEV), ~v_rows.to(DEV)
    what = "%s flags=%d" % (tag, flags)
    name = "k7.dlogits.wide" if " wide" in tag else "k7.dlogits"
    JUDGE.check(name, dlogits[keep_p], r32["dlogits"][keep_p], r64["dlogits"][keep_p], FLOOR[name], what=what)
    JUDGE.check("k7.dvalues", dvalues[keep_v], r32["dvalues"][keep_v], r64["dvalues"][keep_v], FLOOR["k7.dvalues"], what=what)
    dens = (den_p, den_p, den_v, 1.0)
    for i, name in enumerate(SUM_NAMES):
        exact = r64["terms"][name].sum()
        scale = float(r64["terms"][name].abs().sum())
        theirs = r32[name].double() * dens[i]
        JUDGE.check("k7.sums", sums[i], theirs, exact, FLOOR["k7.sums"], scale=scale, what=what + " " + name)
    if d["avail"] is not None:
        assert float(dlogits[d["avail"] == 0].abs().sum()) == 0.0
    bound = torch.stack([r64["terms"][n].abs().sum() for n in SUM_NAMES]) * 1e-12
    return dlogits, dvalues, sums, bound


FLAG_SETS = (0, 15, 5, 10)          # every flag both ways


@pytest.mark.parametrize("na,with_avail,with_factor,with_norm", [
    (5, False, False, False),       # register form, staged
    (19, True, True, True),         # generic form, staged
    (48, True, False, True),        # staged with LDS granted above 64 KB
    (77, True, False, True)])       # unstaged (2 * 256 * 77 * 4 B > 150 KB)
def test_fused_loss_multi_pass_against_float64(na, with_avail, with_factor, with_norm):
    """More rows than the capped grid covers in one pass: every workgroup loops, the second pass reuses the staged tile, the
    last pass is ragged.  A second launch on the same inputs gives bit-identical gradients."""
    assert MULTI_PASS_ROWS == 525073 and MULTI_PASS_ROWS > GRID_CAP_BLOCKS * BLOCK_ROWS
    d = _device_inputs(lr.make_inputs(MULTI_PASS_ROWS, na, with_avail=with_avail, with_factor=with_factor, seed=0))
    norm_pair = NORM if with_norm else None
    norm = None if norm_pair is None else torch.tensor(norm_pair, dtype=torch.float32, device=DEV)
    for flags in FLAG_SETS:
        dl, dv, sums, bound = _judge_against_float64(d, flags, norm_pair, "multi-pass na=%d" % na)
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dv).all())       # every row was written
        dl2, dv2, sums2 = _k7(d, flags, _inv_denoms(d, flags)[0], norm=norm)
        assert torch.equal(dl, dl2) and torch.equal(dv, dv2)
        _same_sums(sums2, sums, bound, False)
        del dl, dv, dl2, dv2


@pytest.mark.parametrize("na,with_avail,mode", [
    (8, False, "plain"), (8, True, "plain"), (9, False, "plain"), (9, True, "plain"),     # register form up to 8 actions
    (75, True, "plain"), (76, True, "plain"),       # with a mask: 2 * 256 * 75 * 4 = 153,600 B is staged, 76 (stride 77) is not
    (149, False, "plain"), (150, False, "plain"),   # without: 256 * 149 * 4 = 152,576 B is staged, 150 (stride 151) is not
    (5, True, "wide"), (19, True, "wide"), (5, False, "wide"), (19, False, "wide")])
def test_fused_loss_dispatch_edges_against_float64(na, with_avail, mode):
    lds = (2 if with_avail else 1) * 256 * (na | 1) * 4
    assert (lds <= 150 * 1024) == (na not in (76, 150))                  # the cases sit on the edge they are named for
    d = _device_inputs(lr.make_inputs(4099, na, with_avail=with_avail, mode=mode, seed=0))
    for flags in FLAG_SETS:
        _judge_against_float64(d, flags, NORM, "edge na=%d%s %s" % (na, "+mask" if with_avail else "", mode))


@pytest.mark.parametrize("na", [5, 19])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_fused_loss_row_count_edges_against_float64(na, rows):
    """One row, one short of a workgroup, exactly one, one more.  The rows are chosen clear of every branch point
    (0.5 % of them is at most one row), so every row is compared."""
    pool = lr.make_inputs(1024, na, with_avail=True, seed=2)
    d = _device_inputs(lr.clear_rows(pool, rows, NORM, clip=HP["clip"], huber_delta=HP["huber_delta"]))
    for flags in FLAG_SETS:
        dl, dv, _, _ = _judge_against_float64(d, flags, NORM, "rows=%d na=%d" % (rows, na), skip=False)
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dv).all())


@pytest.mark.parametrize("na", [5, 19, 77])
def test_fused_loss_masks_away_from_action_zero(na):
    """Rows whose first action is unavailable, and rows with exactly one available action (anywhere): the sampled action
    is that one, the row's entropy is exactly 0 and so is its whole dlogits row."""
    d = _device_inputs(lr.make_inputs(4099, na, with_avail=True, seed=5, single_share=0.1))
    avail = d["avail"]
    assert float((avail[:, 0] == 0).float().mean()) > 0.2
    single = avail.sum(-1) == 1
    assert int(single.sum()) > 200 and int((single & (avail[:, 0] == 0)).sum()) > 100
    assert torch.equal(d["actions"][single].long().squeeze(-1), avail[single].argmax(-1))
    for flags in (15, 0):
        dl, _, _, _ = _judge_against_float64(d, flags, NORM, "masks na=%d" % na)
        assert float(dl[avail == 0].abs().max()) == 0.0
        assert float(dl[single].abs().max()) == 0.0
        assert float(dl[~single].abs().max()) > 0.0
        # the single-action rows on their own: their entropy terms sum to exactly 0
        only = {k: (None if v is None else v[single].contiguous()) for k, v in d.items()}
        dl1, _, sums1 = _k7(only, flags, _inv_denoms(only, flags)[0])
        assert float(sums1[1]) == 0.0 and float(dl1.abs().max()) == 0.0
        assert float(sums1[3]) > 0.0


def _sum_bound(d, flags, norm):
    """1e-12 * sum |per-row term| of the four sums: what a different order of the float64 additions may change."""
    terms = _reference(d, torch.float64, flags, norm)["terms"]
    return torch.stack([terms[n].abs().sum() for n in SUM_NAMES]) * 1e-12


def _same_sums(a, b, bound, one_workgroup, which=range(4)):
    for i in which:
        if one_workgroup:           # a single workgroup adds its partials in a fixed order
            assert float(a[i]) == float(b[i]), (i, float(a[i]), float(b[i]))
        else:                       # the workgroups' atomic adds arrive in any order
            assert abs(float(a[i]) - float(b[i])) <= float(bound[i]), (i, float(a[i]), float(b[i]), float(bound[i]))


@pytest.mark.parametrize("na", [5, 19])
@pytest.mark.parametrize("rows", [200, 4099])
def test_fused_loss_half_calls_and_null_outputs(na, rows):
    """The ABI's promises that the trainer never uses: logits == NULL skips the actor half, values == NULL the critic half,
    each of dlogits / dvalues / sums may be NULL, active == NULL means all ones.  Whatever is still computed is bit-equal
    to the full call (sums of more than one workgroup: to the order of their atomic additions)."""
    d = _device_inputs(lr.make_inputs(rows, na, with_avail=True, with_factor=True, seed=7))
    norm = torch.tensor(NORM, dtype=torch.float32, device=DEV)
    flags = 15
    inv = _inv_denoms(d, flags)[0]
    bound, one = _sum_bound(d, flags, norm), rows <= BLOCK_ROWS
    sentinel = torch.tensor([3.0, 5.0, 7.0, 11.0], dtype=torch.float64, device=DEV)
    dl, dv, sums = _k7(d, flags, inv, norm=norm, sums=sentinel.clone())
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dv).all())
    # critic half alone
    dl_c, dv_c, sums_c = _k7(d, flags, inv, norm=norm, sums=sentinel.clone(), drop=("logits",))
    assert torch.equal(dv_c, dv) and bool(torch.isnan(dl_c).all())
    _same_sums(sums_c, sums, bound, one, which=[2])
    assert [float(sums_c[i]) for i in (0, 1, 3)] == [3.0, 5.0, 11.0]
    # actor half alone
    dl_a, dv_a, sums_a = _k7(d, flags, inv, norm=norm, sums=sentinel.clone(), drop=("values",))
    assert torch.equal(dl_a, dl) and bool(torch.isnan(dv_a).all())
    _same_sums(sums_a, sums, bound, one, which=[0, 1, 3])
    assert float(sums_a[2]) == 7.0
    # each output NULL on its own
    for name in ("dlogits", "dvalues", "sums"):
        before = sentinel.clone()
        dl_n, dv_n, sums_n = _k7(d, flags, inv, norm=norm, sums=before, drop=(name,))
        assert bool(torch.isnan(dl_n).all()) if name == "dlogits" else torch.equal(dl_n, dl)
        assert bool(torch.isnan(dv_n).all()) if name == "dvalues" else torch.equal(dv_n, dv)
        if name == "sums":
            assert torch.equal(before, sentinel)
        else:
            _same_sums(sums_n, sums, bound, one)
    # active == NULL is active == ones
    ones = dict(d, active=torch.ones_like(d["active"]))
    inv1 = _inv_denoms(ones, flags)[0]
    dl_1, dv_1, sums_1 = _k7(ones, flags, inv1, norm=norm)
    dl_0, dv_0, sums_0 = _k7(ones, flags, inv1, norm=norm, drop=("active",))
    assert torch.equal(dl_0, dl_1) and torch.equal(dv_0, dv_1)
    assert not torch.equal(dl_1, dl)                                    # (the masks did matter)
    _same_sums(sums_0, sums_1, _sum_bound(ones, flags, norm), one)


@pytest.mark.parametrize("na,rows,cut", [(5, 4099, 1000), (19, 4099, 2049), (48, 4099, 255),
                                         (19, MULTI_PASS_ROWS, 300001), (77, 4099, 1)])
def test_fused_loss_spans_accumulate(na, rows, cut):
    """"The gradients of successive spans simply accumulate": two calls over [0, cut) and [cut, rows) with the same
    inv_denoms and the same sums give the gradients of one call bit for bit, and its sums up to the order of additions."""
    assert cut % BLOCK_ROWS != 0
    d = _device_inputs(lr.make_inputs(rows, na, with_avail=True, seed=9))
    norm = torch.tensor(NORM, dtype=torch.float32, device=DEV)
    for flags in (15, 2):
        inv = _inv_denoms(d, flags)[0]
        dl, dv, sums = _k7(d, flags, inv, norm=norm)
        dl_s, dv_s, sums_s = _k7(d, flags, inv, norm=norm, hi=cut)
        assert bool(torch.isnan(dl_s[cut:]).all()) and bool(torch.isnan(dv_s[cut:]).all())      # nothing beyond its span
        _k7(d, flags, inv, norm=norm, lo=cut, sums=sums_s, out=(dl_s, dv_s))
        assert torch.equal(dl_s, dl) and torch.equal(dv_s, dv)
        _same_sums(sums_s, sums, _sum_bound(d, flags, norm), False)


@pytest.mark.parametrize("na,with_avail", [(5, True), (5, False), (19, True), (48, True)])
def test_fused_loss_one_bad_row_stays_alone(na, with_avail):
    """A NaN logit in one row in the middle of a staged tile: that row's gradient and the actor's sums are NaN, every other
    row's dlogits and all of dvalues are bit-equal to the clean run."""
    rows, bad = 4099, 3 * BLOCK_ROWS + 100
    d = _device_inputs(lr.make_inputs(rows, na, with_avail=with_avail, seed=11))
    norm = torch.tensor(NORM, dtype=torch.float32, device=DEV)
    flags = 15
    inv = _inv_denoms(d, flags)[0]
    dl, dv, sums = _k7(d, flags, inv, norm=norm)
    k = int(d["actions"][bad])                                          # an available action of that row
    poisoned = dict(d, logits=d["logits"].clone())
    poisoned["logits"][bad, k] = float("nan")
    dl_b, dv_b, sums_b = _k7(poisoned, flags, inv, norm=norm)
    others = torch.ones(rows, dtype=torch.bool, device=DEV)
    others[bad] = False
    assert torch.equal(dl_b[others], dl[others]) and torch.equal(dv_b, dv)
    live = torch.ones(na, dtype=torch.bool, device=DEV) if d["avail"] is None else d["avail"][bad] == 1
    assert bool(torch.isnan(dl_b[bad][live]).all()) and float(dl_b[bad][~live].abs().sum()) == 0.0
    assert all(bool(torch.isnan(sums_b[i])) for i in (0, 1, 3))
    _same_sums(sums_b, sums, _sum_bound(d, flags, norm), False, which=[2])


@pytest.mark.parametrize("rows", [64, 1024])
@pytest.mark.parametrize("flags", [2, 3, 10, 11])
def test_fused_loss_exact_ties(flags, rows):
    """The tie table of tests/loss_reference.py -- value-loss rows from dyadic numbers that sit exactly on the clip, on the
    huber knee and on l_c == l_o: dvalues is bit-equal to what float32 autograd gives there (clamp's closed interval, the
    closed knee, half the gradient per branch of torch.max on a tie)."""
    v, vp, ret, want_mse, want_huber = lr.tie_table(rows)
    want = want_huber if flags & 1 else want_mse
    assert torch.equal(lr.tie_autograd(bool(flags & 1), rows), want)
    d = dict(logits=torch.zeros(rows, 3), avail=None, actions=torch.zeros(rows, 1), old_logp=torch.zeros(rows, 1),
             adv=torch.ones(rows, 1), active=torch.ones(rows, 1), factor=None, values=v, value_preds=vp, returns=ret)
    d = _device_inputs(d)
    inv = torch.tensor([1.0 / rows, 1.0 / rows], dtype=torch.float32, device=DEV)
    hp = dict(clip=lr.TIE_CLIP, huber_delta=lr.TIE_DELTA, entropy_coef=0.0, value_loss_coef=1.0)
    for drop in ((), ("logits",)):
        _, dv, _ = _k7(d, flags, inv, hp=hp, drop=drop)
        assert torch.equal(dv.cpu(), want), (dv.cpu() - want).abs().max()


# ------------------------------------------------------------------------------------------------------------------
# K14 away from the benign cases: masks that do not favour action 0, lone actions, 64 actions, row-count edges, wide logits.
def _sampler_masks(rows, na, kind, g):
    if kind == "none":
        return None
    avail = (torch.rand(rows, na, device=DEV, generator=g) < 0.6).float()
    if kind == "last_only":             # half of the rows: the last action and nothing else
        lone = torch.rand(rows, 1, device=DEV, generator=g) < 0.5
        lone[0] = True
        avail = torch.where(lone, torch.zeros_like(avail), avail)
        avail[:, -1] = torch.where(lone.squeeze(-1), torch.ones(rows, device=DEV), avail[:, -1])
    keep = torch.randint(0, na, (rows, 1), device=DEV, generator=g)
    avail.scatter_(1, torch.where(avail.sum(-1, keepdim=True) == 0, keep, avail.argmax(-1, keepdim=True)), 1.0)
    return avail


def check_sampler_against_float64(actions, logp, logits, avail, noise):
    """The same-noise rule in float64: log p = x - logsumexp(x) on the masked logits, action = argmax p / q.  At least
    99.9 % of the actions equal it; where they do not, the kernel's choice has the same p / q as the argmax to 1e-5 in
    float64 (a near-tie that float32 rounding may decide either way -- never a wrong action hiding in the 0.1 %).
    Log-probs of the chosen actions to float32 rounding: 1e-5 relative + 1e-6 as for the benign cases, + one float32 ulp of
    the largest logit (2^-23 max |x|), which is what rounding logsumexp(x) to float32 costs at wide logits."""
    x = logits.double() if avail is None else torch.where(avail == 0, torch.full_like(logits, -1e10).double(), logits.double())
    ref_l = x - x.logsumexp(-1, keepdim=True)
    score = ref_l.exp() / noise.double()
    ref_a = score.argmax(-1, keepdim=True)
    same = actions == ref_a
    assert float(same.float().mean()) >= 0.999
    mine, best = score.gather(-1, actions), score.gather(-1, ref_a)
    assert bool(((best - mine).abs() <= 1e-5 * best)[~same].all()), (best[~same], mine[~same])
    atol = 1e-6 + 2.0 ** -23 * float(logits.abs().max())
    torch.testing.assert_close(logp.double(), ref_l.gather(-1, actions), rtol=1e-5, atol=atol)
    if avail is not None:
        assert bool((avail.gather(-1, actions) == 1).all())
    return same


@pytest.mark.parametrize("na,rows,scale,masks", [
    (5, 4099, 2.0, "random"), (18, 4099, 2.0, "random"), (48, 4099, 2.0, "random"), (64, 4099, 2.0, "random"),
    (64, 4099, 2.0, "none"), (64, 1, 2.0, "random"), (64, 256, 2.0, "none"), (64, 257, 2.0, "random"),
    (5, 1, 2.0, "none"), (5, 256, 2.0, "random"), (5, 257, 2.0, "last_only"), (5, 262145, 2.0, "random"),
    (64, 262145, 2.0, "last_only"), (18, 4099, 2.0, "last_only"), (2, 4099, 2.0, "last_only"),
    (5, 4099, 30.0, "random"), (48, 4099, 30.0, "none"), (64, 4099, 30.0, "last_only")])
def test_categorical_sample_kernel_edges(na, rows, scale, masks):
    from onpolicy.algorithms.utils import distributions, fused_loss
    distributions.set_sampling_rng("device")
    g = torch.Generator(device=DEV).manual_seed(na * 1000 + rows)
    logits = torch.randn(rows, na, device=DEV, generator=g) * scale
    avail = _sampler_masks(rows, na, masks, g)
    with torch.no_grad():
        assert fused_loss.sample_supported(logits)
        torch.manual_seed(321)
        actions, logp = fused_loss.sample_categorical(logits, avail)
        torch.manual_seed(321)
        noise = torch.empty_like(logits).exponential_(1.0)
    assert actions.shape == (rows, 1) and actions.dtype == torch.int64 and logp.shape == (rows, 1)
    check_sampler_against_float64(actions, logp, logits, avail, noise)
    if masks == "random" and rows >= 4099:
        assert float((avail[:, 0] == 0).float().mean()) > 0.2
        off = avail[:, 0] == 0
        assert bool((actions[off] != 0).all())
    if masks == "last_only":
        lone = (avail.sum(-1) == 1) & (avail[:, -1] == 1)
        assert bool(lone[0]) and (rows < 100 or int(lone.sum()) > rows // 3)
        assert bool((actions[lone] == na - 1).all())
        assert float(logp[lone].abs().max()) == 0.0                     # log 1, exactly


def test_sampler_refuses_what_it_cannot_take():
    from onpolicy.algorithms.utils import distributions, fused_loss
    distributions.set_sampling_rng("device")
    x64, x65 = torch.zeros(3, 64, device=DEV), torch.zeros(3, 65, device=DEV)
    with torch.no_grad():
        assert fused_loss.sample_supported(x64) and not fused_loss.sample_supported(x65)
        assert fused_loss.multi_sample_supported(x64, [57, 7]) and fused_loss.multi_sample_supported(x64, [8] * 8)
        assert not fused_loss.multi_sample_supported(x65, [58, 7])       # total width 65
        assert not fused_loss.multi_sample_supported(x64, [7] * 9)       # 9 heads
        assert not fused_loss.multi_sample_supported(x64, [])
