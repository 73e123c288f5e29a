"""K11 wide for simple_tag (``mappo_simple_tag_step_wide``) without a GPU: what the entry refuses before anything is
launched, and that worlds held on the CPU stay on the tensor path."""
import ctypes

from onpolicy import _native


def test_wide_entry_refuses_bad_calls():
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)       # validation returns before anything is enqueued: a host buffer serves as pointer
    fn = _native.lib().mappo_simple_tag_step_wide
    call = lambda ptrs, agents, adv, landmarks: fn(*ptrs, 4, agents, adv, landmarks, 25, 1, None)      # noqa: E731
    assert call([None] + [p] * 10, 17, 13, 2) == -1
    assert call([p] * 5 + [None] + [p] * 5, 17, 13, 2) == -1       # fresh_pos, with auto_reset
    assert call([p] * 11, 17, 0, 2) == -2 and call([p] * 11, 17, 17, 2) == -2
    assert call([p] * 11, 65, 13, 2) == -4 and call([p] * 11, 17, 13, 65) == -4
    assert not any(buf)


def test_cpu_worlds_of_17_agents_stay_on_the_tensor_path():
    from onpolicy.envs.mpe.simple_tag import TorchSimpleTag
    assert not TorchSimpleTag(2, 17, 2, num_adversaries=13, wide=True).graph_safe
