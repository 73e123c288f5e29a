"""K11 wide for simple_world_comm (``mappo_simple_world_comm_step_wide``) without a GPU: what the entry refuses before
anything is launched, and that worlds held on the CPU stay on the tensor path."""
import ctypes

from onpolicy import _native

from test_mpe_world_comm_cpu import make


def test_wide_entry_refuses_bad_calls():
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)       # validation returns before anything is enqueued: a host buffer serves as pointer
    fn = _native.lib().mappo_simple_world_comm_step_wide
    call = lambda ptrs, agents, adv, obstacles: fn(*ptrs, 4, agents, adv, obstacles, 25, 1, None)      # noqa: E731
    assert call([None] + [p] * 11, 17, 13, 2) == -1
    assert call([p] * 4 + [None] + [p] * 7, 17, 13, 2) == -1       # comm
    assert call([p] * 6 + [None] + [p] * 5, 17, 13, 2) == -1       # fresh_pos, with auto_reset
    assert call([p] * 12, 17, 0, 2) == -2 and call([p] * 12, 17, 17, 2) == -2 and call([p] * 12, 17, 13, 0) == -2
    assert call([p] * 12, 65, 13, 2) == -4 and call([p] * 12, 17, 13, 61) == -4
    assert not any(buf)


def test_cpu_worlds_of_17_agents_stay_on_the_tensor_path():
    assert not make(2, 13, 4, 2, wide=True).graph_safe
