"""``R_MAPPO.ppo_update`` as a captured HIP graph.

One update of the reference (onpolicy/algorithms/r_mappo/r_mappo.py:91-169: evaluate_actions, the two losses, two backward
passes, two clip_grad_norm_ + Adam steps) is ~30 launches on the feed-forward route of this implementation and ~100 on the
recurrent one (K9 / K12 / K7 / K13 + the library GEMMs, reductions and concatenations of the GRU's weight gradients).  On
small minibatches -- BASELINE configs[1], or the 64-threads-per-GPU shard of configs[3] -- those launches, not the kernels,
set the pace.  Nothing in an update depends on the host, and every update of a ``train()`` runs the same kernels on
tensors of the same shapes, so the update is captured once into a HIP graph and replayed:

    eager per update:   sampler gather (1-3 launches) -> scalar prologue (2 launches, + its collective in a multi-GPU job)
                        -> ONE batched copy of the minibatch into the graph's static input tensors
    graph "front":      zero_grad, row table, K9 / K12 forward, ValueNorm update, K7, backward of both networks
    eager (multi-GPU):  gradients -> flat bucket, ONE all-reduce (DataParallel)
    graph "back":       clip + Adam of both networks (K13; the learning rate is read from device memory, so lr_decay between
                        replays needs no re-capture)

A graph belongs to a *signature*: the shapes / dtypes of the minibatch tuple, the observation matrices the lazy ``RowSource``
minibatches point into (their addresses are baked into the graph), ``update_actor`` and the arithmetic of the networks.  The
first update with a new signature runs eagerly (it is also the warm-up: GEMM tuning, lazily created state), the second is
captured, the rest replay.  Minibatches of more than ``MAPPO_UPDATE_GRAPH_MAX_ROWS`` rows (default 2^20) stay eager: their
kernels run for milliseconds, the host enqueues them far ahead of the device anyway, and a graph launch has a fixed cost of its
own (measured on the MI355X, profiles/r05_ab_update_graph.json: 64-thread SMAC shard 31.2 -> 18.6 ms per step, 128-thread
recurrent north-star shard 36.6 -> 27.0, configs[1] 15.04 -> 14.92, but a 512-thread feed-forward north-star shard -- 1.6 M
rows per update -- 29.6 -> 32.4); a graph would also keep the update's activations (14 GB at the north star) alive for good.
``MAPPO_UPDATE_GRAPH=0`` disables the whole thing; so does the class itself when captures do not pay (six captures with fewer
than four replays each: a caller whose minibatches point into matrices that move between ``train()`` calls).

Not captured (the eager ``ppo_update`` runs): PopArt heads (``update`` rebinds the parameters' storage), trainers without the
fused loss / fused optimiser kernels, ``update_actor=False``, host minibatches, minibatches cut into several row spans,
subclasses that override ``ppo_update``.

What else a graph bakes in, and how a stale one is kept from replaying: the addresses of the parameters, of
their ``.grad`` targets and of the Adam state (``exp_avg``, ``exp_avg_sq``, ``step``), and the kernel-argument
hyper-parameters (``clip_param``, ``entropy_coef``, ``value_loss_coef``, ``max_grad_norm``, ``huber_delta`` and the loss
flags).  The hyper-parameters are part of every signature (a trainer that anneals ``entropy_coef`` gets a new capture, not stale
coefficients); the addresses are compared once per ``train()`` (``begin_train``: after ``optimizer.load_state_dict``, a
re-created optimiser or ``net.to()`` every entry is dropped and captured again), and ``invalidate()`` does the same on demand.

Failures (VERDICT r5 "next" #8): only the CAPTURE may fail quietly, and only while nothing has executed -- the eager update then
runs the whole minibatch.  In a multi-GPU job the front half has already run for real (ValueNorm fed, gradients
all-reduced) when the back half is captured; if that capture fails the update is FINISHED eagerly from the reduced gradients
(``_update_back``) instead of being run a second time.  Errors during a replay propagate.  ``capture_failures`` counts the
events (bench.py prints it).
"""
import os

import torch

from onpolicy.algorithms.r_mappo.r_mappo import Minibatch
from onpolicy.algorithms.utils.fused_mlp import RowSource, matrix_arithmetic_of
from onpolicy.utils.graph_capture import capturing


class _Entry(object):
    """What ``UpdateGraph`` holds per signature.  ``state`` is "warm" (seen once, the eager update was the warm-up), "ready"
    (captured, replays) or "failed" (its capture failed: the shape stays eager); everything else is set by the capture."""
    __slots__ = (
        "state",
        "static", "inputs",         # the Minibatch the graphs read (clones of the captured one) and its device tensors
        "loaded",                   # ((id, version) of the tensors the static inputs hold a copy of, those tensors)
        "scales", "scales_src",     # static copy of the scalar prologue, and the tensor it was last copied from
        "lr", "lr_val",             # per optimiser: the learning rate in device memory (K13 reads it there) and on the host
        "front",                    # graph: zero_grad .. backward of both networks (one process: the optimiser steps too)
        "back", "front_grads",      # multi-GPU: graph of clip + Adam, after the eager exchange of the front's gradients
        "front_done",               # multi-GPU: the front already ran for the minibatch that triggered the capture
        "grads", "out")             # what a caller finds in .grad after an update; the six tensors ppo_update returns

    def __init__(self, state="warm"):
        for name in self.__slots__:
            setattr(self, name, None)
        self.state = state

    def fail(self):
        """Let go of everything captured; the signature stays eager from here on."""
        self.__init__("failed")


class UpdateGraph(object):
    MAX_ENTRIES = 4
    MAX_CAPTURES_WITHOUT_PAYOFF = 6     # ... then at least four replays per capture, or the graphs are switched off

    def __init__(self, trainer):
        self.t = trainer
        self.entries = {}           # signature -> entry
        self.order = []             # signatures, least recently used first
        self.pool = None
        self.replays = self.captures = self.warmups = self.capture_failures = self.invalidations = 0
        self._state = None          # addresses of parameters / optimiser state the live entries were captured with
        self.max_rows = int(os.environ.get("MAPPO_UPDATE_GRAPH_MAX_ROWS", str(1 << 20)))
        self.off = os.environ.get("MAPPO_UPDATE_GRAPH", "1") == "0"

    # ------------------------------------------------------------------------------------------------ eligibility
    def _trainer_ok(self):
        t = self.t
        if self.off or torch.device(t.device).type != "cuda" or not t._fused_loss or t._use_popart:
            return False
        from onpolicy.algorithms.utils import fused_optim
        return fused_optim.enabled()

    def _signature(self, sample, update_actor):
        """-> (hashable signature, rows) or (None, 0) when the minibatch cannot be captured."""
        t = self.t
        parts = []
        for x in sample:
            if x is None:
                parts.append(None)
            elif isinstance(x, RowSource):
                parts.append(("rows", x.src.data_ptr(), tuple(x.src.shape), None if x.idx is None else tuple(x.idx.shape),
                              x.chunk, x.standardized, x.width))
            elif torch.is_tensor(x) and x.is_cuda and x.is_contiguous():
                parts.append((tuple(x.shape), x.dtype))
            elif torch.is_tensor(x) and x.is_cuda:
                # a view (the stride-0 zero RNN states a feed-forward buffer hands out): read in place, its address is part of
                # the graph like a RowSource's matrix
                parts.append(("view", x.data_ptr(), tuple(x.shape), tuple(x.stride()), x.dtype))
            else:
                return None, 0
        rows = sample.adv_targ.shape[0]
        if rows > self.max_rows or not update_actor:
            return None, 0          # (update_actor = False leaves the actor without gradients: the PyTorch optimiser path)
        if len(t._row_spans(sample).spans) != 1:
            return None, 0
        arith = tuple(matrix_arithmetic_of(m) for net in (t.policy.actor, t.policy.critic) for m in net.modules()
                      if hasattr(m, "matrix_arithmetic"))
        # scalars that travel as kernel ARGUMENTS (K7, K13) and are therefore frozen into a capture
        hyper = (float(t.clip_param), float(t.entropy_coef), float(t.value_loss_coef), float(t.max_grad_norm),
                 float(t.huber_delta), bool(t._use_max_grad_norm), bool(t._use_clipped_value_loss), bool(t._use_huber_loss),
                 bool(t._use_policy_active_masks), bool(t._use_value_active_masks), bool(t._use_valuenorm))
        return (tuple(parts), bool(update_actor), bool(t._obs_standardized), arith, hyper), rows

    def _state_key(self):
        """Addresses a capture bakes in besides the minibatch: parameters and the optimisers' state tensors."""
        t = self.t
        key = []
        for net, opt in ((t.policy.actor, t.policy.actor_optimizer), (t.policy.critic, t.policy.critic_optimizer)):
            key.append(id(opt))
            for p in net.parameters():
                st = opt.state.get(p, {})
                key.append((p.data_ptr(),) + tuple(v.data_ptr() for v in st.values() if torch.is_tensor(v)))
        return tuple(key)

    def invalidate(self):
        """Drop every captured update (restore / load paths that rebind parameters or optimiser state call this; train()
        also notices by itself, ``begin_train``)."""
        if self.entries:
            self.invalidations += 1
        self.entries.clear()
        self.order.clear()
        self._state = None

    def begin_train(self):
        """Once per ``train()``: entries captured against other parameter / optimiser-state addresses are dropped."""
        if not self.entries:
            return
        key = self._state_key()
        if self._state is not None and key != self._state:
            self.invalidate()

    # ------------------------------------------------------------------------------------------------ the update
    def run(self, sample, update_actor):
        """The 6-tuple of ``ppo_update`` from a graph replay, or None: the caller runs the eager update."""
        if not self._trainer_ok():
            return None
        sample = Minibatch(*sample)     # (named, not converted: a replay only copies device tensors)
        sig, rows = self._signature(sample, update_actor)
        if sig is None:
            return None
        e = self.entries.get(sig)
        if e is None:       # first sight of this signature: the eager update is the warm-up
            self._remember(sig, _Entry())
            self.warmups += 1
            return None
        if e.state == "failed":
            return None
        self.order.remove(sig)
        self.order.append(sig)
        t = self.t
        scales = t.dp.minibatch_scales(sample.active_masks, sample.returns, t._use_policy_active_masks,
                                       t._use_value_active_masks)
        if scales is None:
            return None
        if e.state == "warm":
            if self.captures >= self.MAX_CAPTURES_WITHOUT_PAYOFF and self.replays < 4 * self.captures:
                # the signatures keep changing (addresses of the matrices the minibatches point into that do not survive a
                # train(), ...): captures cost ~100 ms each and are not paying for themselves -- stay eager from here on
                print("update graph: %d captures for %d replays; updates stay eager" % (self.captures, self.replays))
                self.off = True
                return None
            try:
                finished = self._capture(e, sample, update_actor, scales)
            except Exception as exc:
                # Nothing of this minibatch has executed (a capture only records; _capture itself deals with a failure AFTER the
                # front half ran): whatever the capture cannot take stays eager, loudly.
                e.fail()
                self.capture_failures += 1
                print("update graph: capture failed (%s: %s); this update shape stays eager" % (type(exc).__name__, exc))
                torch.cuda.synchronize(t.device)
                return None
            if finished is not None:        # the back capture failed after the front had run: the update was completed eagerly
                return finished
        return self._replay(e, sample, scales)

    def _remember(self, sig, entry):
        while len(self.order) >= self.MAX_ENTRIES:
            self.entries.pop(self.order.pop(0), None)
        self.entries[sig] = entry
        self.order.append(sig)

    @staticmethod
    def _tensors(sample):
        """The device tensors of a minibatch that a replay must find in the static inputs (index lists of RowSources included)."""
        out = []
        for x in sample:
            if isinstance(x, RowSource):
                if x.idx is not None:
                    out.append(x.idx)
            elif torch.is_tensor(x) and x.is_contiguous():
                out.append(x)
        return out

    def _capture(self, e, sample, update_actor, scales):
        t = self.t
        dev = torch.device(t.device)
        static = []
        for x in sample:
            if isinstance(x, RowSource):
                static.append(RowSource.all_rows(x.src, x.standardized, x.width) if x.idx is None else
                              RowSource(x.src, x.idx.clone(), x.chunk, x.standardized, x.width))
            elif torch.is_tensor(x) and x.is_contiguous():
                static.append(x.clone())
            else:
                static.append(x)            # None, or a view that is read in place (see _signature)
        e.static = Minibatch(*static)
        e.inputs = self._tensors(static)
        cur = self._tensors(sample)             # the static inputs start out as copies of this minibatch
        e.loaded = ([(id(x), x._version) for x in cur], cur)
        e.scales = scales.clone()
        e.scales_src = scales
        opts = (t.policy.actor_optimizer, t.policy.critic_optimizer)
        e.lr = [torch.full((1,), float(o.param_groups[0]["lr"]), dtype=torch.float64, device=dev) for o in opts]
        e.lr_val = [float(o.param_groups[0]["lr"]) for o in opts]
        params = [p for net in (t.policy.actor, t.policy.critic) for p in net.parameters() if p.requires_grad]
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        front = torch.cuda.CUDAGraph()
        # (thread_local: the capture must not outlaw what OTHER threads do meanwhile -- RCCL's watchdog polls the events of
        # earlier collectives -- while the autograd thread's launches into the capturing stream are recorded all the same)
        with capturing(front, pool=self.pool, capture_error_mode="thread_local"):
            value_loss, policy_loss, dist_entropy, ratio = t.ppo_update(e.static, update_actor, _front_only=True,
                                                                        _scales=e.scales)
            if not t.dp.active:
                norms = t._update_back(update_actor, lr_devices=e.lr)
        e.front = front
        if t.dp.active:
            # the gradient exchange stays eager between the two halves (one batched copy + ONE collective, utils/dist.py)
            e.front_grads = [p.grad for p in t.dp._params]
            front.replay()                      # (a capture executes nothing: run the front once so that the bucket is real)
            t.dp.all_reduce_grads()             # -> every param.grad is a view of the reduced flat bucket
            # From here on this minibatch HAS been evaluated: ValueNorm fed, gradients reduced, one collective issued on
            # every rank.  If the back half cannot be captured the update is finished eagerly from those gradients -- running
            # the eager ppo_update instead would feed the normaliser twice and issue a collective the other ranks do not.
            try:
                back = torch.cuda.CUDAGraph()
                with capturing(back, pool=self.pool, capture_error_mode="thread_local"):
                    if os.environ.get("MAPPO_TEST_FAIL_BACK_CAPTURE", "0") == "1":     # (tests/test_gpu_update_graph.py)
                        raise RuntimeError("forced by MAPPO_TEST_FAIL_BACK_CAPTURE")
                    norms = t._update_back(update_actor, lr_devices=e.lr)
            except Exception as exc:
                torch.cuda.synchronize(dev)
                print("update graph: capture of the optimiser half failed after the front half ran (%s: %s); this update "
                      "is finished eagerly, the shape stays eager" % (type(exc).__name__, exc))
                norms = t._update_back(update_actor)
                out = tuple(x.detach().clone() for x in (value_loss, norms[1], policy_loss, dist_entropy, norms[0], ratio))
                e.fail()
                self.capture_failures += 1
                return out
            e.back = back
            e.front_done = True
        e.grads = [(p, p.grad) for p in params]
        e.out = (value_loss, norms[1], policy_loss, dist_entropy, norms[0], ratio)
        e.state = "ready"
        self.captures += 1
        self._state = self._state_key()
        return None

    def _replay(self, e, sample, scales):
        t = self.t
        for i, o in enumerate((t.policy.actor_optimizer, t.policy.critic_optimizer)):
            lr = float(o.param_groups[0]["lr"])
            if lr != e.lr_val[i]:
                e.lr[i].fill_(lr)
                e.lr_val[i] = lr
        if e.front_done:
            # (multi-GPU capture: the front and the gradient exchange already ran for this very minibatch)
            e.front_done = False
            e.back.replay()
        else:
            # inputs: one batched copy, skipped when this very minibatch (same tensor objects, unchanged) is already loaded --
            # the whole-batch tuple of a one-minibatch epoch is handed out again in every epoch
            cur = self._tensors(sample)
            key = [(id(x), x._version) for x in cur]
            if e.loaded is None or e.loaded[0] != key:
                torch._foreach_copy_(e.inputs, cur)
                e.loaded = (key, cur)           # (holding the sources keeps their ids from being recycled)
            if e.scales_src is not scales:
                e.scales.copy_(scales)
                e.scales_src = scales
            e.front.replay()
            if e.back is not None:
                t.dp.all_reduce_from(e.front_grads)
                e.back.replay()
        for p, g in e.grads:                    # what a caller finds in .grad after an update (clipped, reduced)
            p.grad = g
        self.replays += 1
        return e.out
