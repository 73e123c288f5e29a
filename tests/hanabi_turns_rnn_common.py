"""TEST INFRASTRUCTURE shared by the tests of the recurrent host-free Hanabi route (tests/test_hanabi_turns_rnn_cpu.py,
tests/test_gpu_hanabi_turns_rnn.py): the recurrent stub policy whose outputs do not depend on the batch."""
import hanabi_turns_common as common


def recurrent_stub_get_actions(cent_obs, obs, rnn_states_actor, rnn_states_critic, masks, available_actions=None,
                               deterministic=False):
    """``common.stub_get_actions`` for value / action / log-prob; the new states are elementwise functions of
    ``state * mask`` and of single observation entries (every operation rounds on its own): equal rows give equal bits
    whatever else is in the batch, and the state a player carries shows in what it carries next."""
    value, action, logp, _, _ = common.stub_get_actions(cent_obs, obs, rnn_states_actor, rnn_states_critic, masks,
                                                        available_actions, deterministic)
    rows = obs.shape[0]
    m = masks.reshape(rows, 1, 1)
    new_actor = 0.5 * rnn_states_actor * m + obs[:, 3:4].reshape(rows, 1, 1) + 1.0
    new_critic = 0.25 * rnn_states_critic * m - cent_obs[:, 4:5].reshape(rows, 1, 1) + 2.0
    return value, action, logp, new_actor, new_critic
