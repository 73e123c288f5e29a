"""What the two host-free Hanabi routes share (runner/shared/hanabi_moves.py) without a GPU: the packed counter block of the
operand base under both operand classes, and ``build`` on a device that cannot capture."""
import types

import numpy as np
import pytest
import torch

from onpolicy.runner.shared import hanabi_eval, hanabi_moves, hanabi_turns

CPU = torch.device("cpu")


def _turn_operands(n, cls=hanabi_turns.TurnOperands):
    turn = types.SimpleNamespace(**{name: torch.zeros(n, 2, w) for name, w in zip(hanabi_turns.ROW_FIELDS, (5, 6, 3))})
    for name in hanabi_turns.SCALAR_FIELDS:
        setattr(turn, name, torch.zeros(n, 2, 1))
    return cls(turn, torch.zeros(n, 5), torch.zeros(n, 6), torch.zeros(n, 3))


def _eval_operands(n, cls=hanabi_eval.EvalOperands):
    return cls(torch.zeros(n, 5), torch.zeros(n, 3), 2, 1, 4, True)


@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("make,cls", [(_turn_operands, hanabi_turns.TurnOperands), (_eval_operands, hanabi_eval.EvalOperands)],
                         ids=["turn", "eval"])
def test_counter_views_are_aligned_tile_the_block_and_read_back(make, cls, n):
    """Every counter of ``COUNTERS`` is a view [n] of its dtype into ``counter_block`` that starts at a multiple of its
    element size; the views tile the block in ``COUNTERS``' order, nothing between or behind them; ``read_counters``
    returns what the views hold (each filled with its own pattern); and the same counters with uint8 in front of int64 --
    misaligned at these odd n -- are refused at construction."""
    o = make(n)
    assert isinstance(o, hanabi_moves.MoveOperands) and (o.n, o.players, o.device) == (n, 2, CPU)
    assert o.can_move.dtype == o.env_actions.dtype == torch.int32 and not o.can_move.any() and bool((o.env_actions == -1).all())
    block = o.counter_block
    assert block.dtype == torch.uint8 and block.data_ptr() % 8 == 0 and any(t is block for t in o.state_tensors())
    at = 0
    for k, (name, dt) in enumerate(cls.COUNTERS):
        view, size = getattr(o, name), torch.empty((), dtype=dt).element_size()
        assert view.dtype == dt and view.shape == (n,) and view.is_contiguous()
        start = view.data_ptr() - block.data_ptr()
        assert start == at and start % size == 0, (name, start, at)
        at += n * size
        view.copy_((torch.arange(n) * 7 + 31 * k + 1).to(dt))
    read = o.read_counters()
    assert at == block.numel() and list(read) == [name for name, _ in cls.COUNTERS]
    for k, (name, _) in enumerate(cls.COUNTERS):
        assert isinstance(read[name], np.ndarray) and np.array_equal(read[name], np.arange(n) * 7 + 31 * k + 1), name
        assert np.array_equal(read[name], getattr(o, name).numpy()), name

    class Misordered(cls):
        COUNTERS = cls.COUNTERS[::-1]           # uint8 first, int64 last
    with pytest.raises(ValueError, match="COUNTERS"):
        make(n, Misordered)


@pytest.mark.parametrize("what,with_value_head", [("Hanabi move", True), ("Hanabi eval move", False)])
def test_build_returns_none_on_a_cpu_device_without_constructing_a_graph(monkeypatch, what, with_value_head):
    """With its switch on and tables that could be captured, ``build`` as either route calls it answers None for a CPU
    device before any graph object exists (through the runner: ``turn_graphs is None`` / ``graphs is None`` in
    tests/test_hanabi_turns_cpu.py and tests/test_hanabi_eval_cpu.py)."""
    def never(*args, **kwargs):
        raise AssertionError("a graph was constructed for a CPU device")
    monkeypatch.setattr(hanabi_moves, "MoveGraph", never)
    monkeypatch.setattr(hanabi_moves.rollout_graph, "captured", never)
    runner, envs = types.SimpleNamespace(num_agents=2), types.SimpleNamespace(graph_safe=True)
    assert hanabi_moves.build(runner, object(), envs, 7, CPU, with_value_head, enabled=True, what=what) is None
