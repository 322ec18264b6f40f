"""mxabides.ddqn.run_episode on the CPU against a scripted env: the episode loop (reset and first
step, arrival price, the act step, the per-period bookkeeping in PyTorch ops, the replay ring, the
train schedule, the result dict) must equal, exactly, the chain of oracle/ddqn_ref.py's state_ref
and period_ref over the script, for the actions the learner itself chose."""
import ctypes

import numpy as np
import pytest
import torch

import ddqn_ref
from mxabides import ddqn
from mxabides.gym import OBS_SIZE, RL_STATE_WORDS

NH, Q0, CAP, BATCH, TRAIN_EVERY = 6, 100000.0, 100, 8, 2


class ScriptedEnv:
    """the four members of VecABIDESEnv that run_episode uses, replaying canned rows: step k copies
    obs[k] and flags[k], write_rl_state copies st[k]; the action vectors it was given are kept"""

    def __init__(self, obs, flags, st):
        self.obs, self.flags, self.st = obs, flags, st
        self.n_envs = obs.shape[1]
        self.k, self.acts = -1, []

    def reset(self, seeds=None):
        self.k, self.acts = -1, []

    def step_device(self, d_actions, d_obs, d_flags):
        self.k += 1
        a = np.empty((self.n_envs, 3), dtype=np.float64)
        ctypes.memmove(a.ctypes.data, d_actions, a.nbytes)
        self.acts.append(a)
        ctypes.memmove(d_obs, self.obs[self.k].ctypes.data, self.obs[self.k].nbytes)
        ctypes.memmove(d_flags, self.flags[self.k].ctypes.data, self.flags[self.k].nbytes)

    def write_rl_state(self, d_st):
        ctypes.memmove(d_st, self.st[self.k].ctypes.data, self.st[self.k].nbytes)


def make_script(n, seed, all_dead_from_3):
    """NH + 1 steps (the first one, then one per period) of n envs. Flag bit 0 = done, bit 1 = the
    observation is valid, bit 2 = env error. By env index modulo 5:
      0  lives through; its fills have dq == 0 at period 1 and dq < 0 at period 3;
      1  never valid at the first step (so never alive), and no LOB at the first step;
      2  no LOB at the first step (arrival 1); finishes (done) at period 2;
      3  errors at period 1; its remaining time is 1 from the first step on (the last-step action);
      4  loses the observation at period 3.
    After an env has left, its script goes on with junk flags (valid ones among them) and fills.
    With all_dead_from_3 every env is done at period 2 at the latest."""
    rs = np.random.RandomState(seed)
    T = NH + 1
    kind = np.arange(n) % 5
    obs = rs.rand(T, n, OBS_SIZE) * 1000 - 500
    st = rs.rand(T, n, RL_STATE_WORDS) * 100
    flags = np.full((T, n), 2, dtype=np.int32)
    # the remaining quantity: multiples of 250 from 50250 up are where a reciprocal multiply and
    # the true division land in different bins, and odd quantities where the shares differ
    qty = np.where(rs.rand(T, n) < 0.5, 50250 + 250 * rs.randint(0, 199, (T, n)), rs.randint(0, int(Q0) + 1, (T, n)))
    for k in range(T):
        obs[k, :, 0] = NH - k  # 1 at the last period
        obs[k, :, 1] = qty[k]
    obs[:, kind == 3, 0] = 1
    dq = rs.randint(1, 4000, (T, n)).astype(np.float64)
    dq[2, kind == 0] = 0.0   # step k is period k - 1
    dq[4, kind == 0] = -3.0
    dq[0] = 0.0
    st[:, :, 2] = np.cumsum(dq, 0)
    st[:, :, 0] = 1e7 - np.cumsum(dq * rs.randint(99000, 101000, (T, n)), 0)
    st[:, :, 3] = 100000 + rs.randint(-500, 500, (T, n))
    st[:, :, 4] = st[:, :, 3] + rs.randint(1, 200, (T, n))
    st[:, :, 7] = 3
    st[0, (kind == 1) | (kind == 2), 7] = rs.choice([0.0, 1.0, 2.0], int(((kind == 1) | (kind == 2)).sum()))
    flags[0, kind == 1] = rs.choice([0, 1, 4, 5], int((kind == 1).sum()))
    flags[3, kind == 2] = 3
    flags[2, kind == 3] = 6
    flags[4, kind == 4] = rs.choice([0, 1], int((kind == 4).sum()))
    if all_dead_from_3:
        flags[3] |= 1
    # after an env has left, junk: mostly valid again
    gone = np.zeros(n, dtype=bool)
    for k in range(T):
        junk = rs.choice([2, 2, 3, 0, 6], n).astype(np.int32)
        flags[k] = np.where(gone, junk, flags[k])
        gone |= ((flags[k] & 2) == 0) | ((flags[k] & 5) != 0)
    return np.ascontiguousarray(obs), flags, np.ascontiguousarray(st)


def table_ref():
    """ExecutionTask.table restated: the reference's action table, scale * child shares of the
    parent order and the DummyRL level shares of the allocation"""
    child = int(Q0 / (NH - 1))
    acts = ddqn_ref.action_table(ddqn.SIZE_ALLOCATION, ddqn.SIZE_SCALE)
    return np.array([(max(0, round(scale * child)) / Q0,) + ddqn.LEVEL_SHARES[alloc] for alloc, scale in
                     (acts[k] for k in range(len(acts)))])


def expected(obs, flags, st, actions, train):
    """the episode by the plain references, for the actions [NH, n] the learner chose"""
    n = obs.shape[1]
    g0, g1 = ddqn.create_uniform_grid([0, 0], [1.0, 1.0], ddqn.GRID_BINS)
    table = table_ref()
    alive = ((flags[0] & 2) != 0) & ((flags[0] & 5) == 0)
    arrival = np.where(st[0][:, 7] == 3, (st[0][:, 3] + st[0][:, 4]) / 2, 1.0)
    out = {"env_steps": alive.astype(np.int64), "ring_s": np.zeros((CAP + 1, 2), np.float32),
           "ring_s2": np.zeros((CAP + 1, 2), np.float32), "ring_a": np.zeros(CAP + 1, np.int64),
           "ring_r": np.zeros(CAP + 1, np.float32), "n_dev": 0, "stored": 0}
    s = ddqn_ref.state_ref(obs[0], g0, g1, NH, Q0).astype(np.float32)
    rewards, vectors, lives, counter = [], [np.zeros((n, 3))], [], 0
    for t in range(NH):
        o = obs[t]
        last = o[:, 0] == 1
        vec = table[actions[t]]
        vec[last] = np.stack([o[last, 1] / Q0, np.ones(last.sum()), np.zeros(last.sum())], 1)
        vectors.append(vec)
        out = ddqn_ref.period_ref(n, OBS_SIZE, RL_STATE_WORDS, train, obs[t + 1], st[t + 1], st[t], arrival, flags[t + 1],
                                  alive, s, actions[t], out["env_steps"], g0, len(g0), g1, len(g1), float(NH), Q0,
                                  1e4 / Q0, out["ring_s"], out["ring_s2"], out["ring_a"], out["ring_r"], CAP,
                                  out["n_dev"], out["stored"])
        rewards.append(out["r_row"])
        lives.append(out["live"])
        if train and t % TRAIN_EVERY == 0 and min(out["n_dev"], CAP) > BATCH and out["live"]:
            counter += 1
        alive, s = out["alive_next"], out["s2"]
    returns = np.zeros(n)
    for r in rewards:
        returns = returns + r
    return dict(out, rewards=np.stack(rewards), returns=returns, vectors=np.stack(vectors), arrival=arrival,
                lives=lives, counter=counter)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,mode,all_dead_from_3", [(5, "train", False), (70, "train", False), (70, "train", True),
                                                    (5, "test", False), (70, "test", False)])
def test_run_episode_equals_the_chained_references(n, mode, all_dead_from_3):
    obs, flags, st = make_script(n, 11 + n, all_dead_from_3)
    kind = np.arange(n) % 5
    env = ScriptedEnv(obs, flags, st)
    learner = ddqn.DDQNLearner(device="cpu", seed=2, batch_size=BATCH, capacity=CAP, mode=mode)
    task = ddqn.ExecutionTask(quantity=Q0, n_horizon=NH, device="cpu")
    rec = []
    res = ddqn.run_episode(env, learner, task, seeds=list(range(n)), train_every=TRAIN_EVERY, record=rec, fused=False)
    train = mode == "train"
    actions = res["actions"].numpy()
    assert actions.dtype == np.int64 and actions.shape == (NH, n)
    assert actions.min() >= 0 and actions.max() < ddqn.N_ACTIONS
    ref = expected(obs, flags, st, actions, int(train))

    # the script holds what it is meant to hold
    assert not ref["env_steps"][kind == 1].any() and (ref["arrival"][kind == 1] == 1).all()
    assert (ref["arrival"][kind == 2] == 1).all() and (ref["env_steps"][kind == 2] == 4).all()
    assert (ref["env_steps"][kind == 3] == 3).all() and (ref["rewards"][1:, kind == 3] == 0).all()
    assert (ref["env_steps"][kind == 4] == (4 if all_dead_from_3 else 5)).all()
    assert (ref["rewards"][[1, 3]][:, kind == 0] == 0).all() and (ref["rewards"][0, kind == 0] != 0).all()
    assert (ref["env_steps"][kind == 0] == (4 if all_dead_from_3 else NH + 1)).all()
    assert ref["lives"] == ([True] * 3 + [False] * 3 if all_dead_from_3 else [True] * NH)
    if train and n == 70:
        assert ref["stored"] > CAP  # the ring wrapped
        assert ref["counter"] == (2 if all_dead_from_3 else 3)  # the update of period 4 is masked off

    assert res["steps"] == NH + 1 and env.k == NH
    assert same(res["rewards"].numpy(), ref["rewards"])
    assert same(res["returns"].numpy(), ref["returns"])
    assert same(res["env_steps"].numpy(), ref["env_steps"])
    assert same(res["flags"].numpy(), flags[NH])
    assert same(res["arrival"].numpy(), ref["arrival"])
    assert res["stored"].dtype == torch.int64 and int(res["stored"]) == ref["stored"] and (train or ref["stored"] == 0)
    # the action vectors: as recorded, and as the env was given them
    assert len(rec) == NH + 1 and same(torch.stack(rec).numpy(), ref["vectors"])
    assert same(np.stack(env.acts), ref["vectors"])
    m = learner.memory
    assert int(m.n_dev) == ref["n_dev"] == ref["stored"]
    for k, t in (("ring_s", m.s), ("ring_s2", m.s2), ("ring_a", m.a), ("ring_r", m.r)):
        assert same(t.numpy()[:CAP], ref[k][:CAP]), k  # row CAP takes the masked-out rows of add_device
    assert learner.learn_step_counter == ref["counter"]
