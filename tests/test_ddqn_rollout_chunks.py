"""mxabides.ddqn.rollout_chunks: the launches of one closed-loop episode (run_episode(rollout=True))
as (first_zero, n_steps) pairs. The episode is the zero step and the periods 0 .. nh-1; when
training a launch ends after every period t with t % train_every == 0 (the learner updates there)."""
import pytest

from mxabides.ddqn import rollout_chunks

CASES = [((27, 5, True), [2, 5, 5, 5, 5, 5, 1]),
         ((27, 5, False), [28]),
         ((1, 5, True), [2]),
         ((6, 1, True), [2, 1, 1, 1, 1, 1]),
         ((5, 7, True), [2, 4])]


@pytest.mark.parametrize("args,steps", CASES)
def test_rollout_chunks(args, steps):
    nh, train_every, train = args
    chunks = rollout_chunks(*args)
    assert [k for _, k in chunks] == steps
    assert sum(k for _, k in chunks) == nh + 1
    assert [fz for fz, _ in chunks] == [True] + [False] * (len(chunks) - 1)
    # no launch spans the end of a training period: a period t with t % train_every == 0 (episode
    # row t + 1) is the last row of its launch
    row = 0
    for _, k in chunks:
        inside = range(row, row + k - 1)  # every row of the launch but its last
        if train:
            assert not [r for r in inside if r >= 1 and (r - 1) % train_every == 0], (chunks, row)
        row += k


def test_rollout_chunks_defaults():
    assert rollout_chunks() == rollout_chunks(27, 5, True)
    assert rollout_chunks() == [(True, 2)] + [(False, 5)] * 5 + [(False, 1)]
