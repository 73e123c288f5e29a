"""K11 wide for simple_push (``mappo_simple_push_step_wide``) without a GPU: what the entry refuses before anything is
launched, and that worlds held on the CPU stay on the tensor path."""
import ctypes

from onpolicy import _native


def test_wide_entry_refuses_bad_calls():
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)       # validation returns before anything is enqueued: a host buffer serves as pointer
    fn = _native.lib().mappo_simple_push_step_wide
    call = lambda ptrs, agents, landmarks: fn(*ptrs, 4, agents, landmarks, 25, 1, None)      # noqa: E731
    assert call([None] + [p] * 12, 17, 2) == -1
    for fresh in (6, 7, 8):         # fresh_pos, fresh_landmarks, fresh_goal, with auto_reset
        assert call([p] * fresh + [None] + [p] * (12 - fresh), 17, 2) == -1
    assert call([p] * 13, 1, 2) == -2 and call([p] * 13, 17, 0) == -2
    assert call([p] * 13, 65, 2) == -4 and call([p] * 13, 17, 3) == -4
    assert not any(buf)


def test_cpu_worlds_of_17_agents_stay_on_the_tensor_path():
    from onpolicy.envs.mpe.simple_push import TorchSimplePush
    env = TorchSimplePush(2, 17, 2, wide=True)
    assert env._wide and not env.graph_safe
    env.reset()
    pos = env.pos
    obs = env.step([[0] * 17] * 2)[0]
    assert env.pos is not pos and obs.shape == (2, sum(env.obs_dims))      # the tensor step rebinds its state
