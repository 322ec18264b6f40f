"""k periods per launch with the Q-network policy inside the step kernel on a state of N features
(include/mxa_policy_features.h mxa_step_policy_spec): every row of a launch (observation, flags,
action index, action vector, the execution agent's state) and the env blocks (events, per-pop parity
hash, status, error, time) equal, bit for bit, the per-step sequence mxa_ddqn_state_spec,
mxa_qnet_act, mxa_step_device, mxa_write_rl_state on a second handle: rmsc03 + DummyRL with six
features and envs that end inside the launch, test and train mode, eight features on the IBM replay
tape, two splits of the episode into launches, a null state pointer. A meaning check that does not
rest on the engine's own state code: a one-layer integer net whose argmax is the bin itself, so the
actions must be the numpy digitize of the observation the env stored. And every refused call leaves
the env blocks alone."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ddqn_features_ref as R
from mxabides import _lib, ddqn, tape
from mxabides.gym import OBS_SIZE, RL_STATE_WORDS, VecABIDESEnv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NET_SEED = 5
KEYS = ("events", "hash", "status", "err", "current_time")
SPREAD_FIXTURE = "eps_rl_5_123456789_2024_7"
_CACHE = {}


def _stream():
    """one non-default stream for the handles and the learner's kernels alike"""
    if "stream" not in _CACHE:
        _CACHE["stream"] = torch.cuda.Stream()
    torch.cuda.set_stream(_CACHE["stream"])
    return _CACHE["stream"]


def _make(kind, n):
    stream = _stream()
    if kind == "replay":
        v = VecABIDESEnv(tape.Tape.load(os.path.join(GOLD, "tape_IBM_2003-01-14.npz")), n)
    else:
        v = VecABIDESEnv(seeds=(123456789 + np.arange(n)) & 0xFFFFFFFF)
    v.set_stream(stream.cuda_stream)
    v.set_parity_hash(True)
    v.reset()
    return v


class Rows:
    """the device rows of K steps of n envs, between sentinel values"""

    def __init__(self, K, n):
        f = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device="cuda")
        self.obs = f((K, n, OBS_SIZE), torch.float64, -7.25)
        self.flags = f((K, n), torch.int32, -7)
        self.a = f((K, n), torch.int64, -7)
        self.act = f((K, n, 3), torch.float64, -7.25)
        self.st = f((K, n, RL_STATE_WORDS), torch.float64, -7.25)

    def assert_equal(self, other, what, state=True):
        for name in ("flags", "a") + (("st",) if state else ()) + ("act", "obs"):
            x, y = getattr(self, name), getattr(other, name)
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)  # bit for bit
            assert torch.equal(x, y), (what, name, torch.nonzero((x != y).reshape(x.shape[0], -1).any(1))[:4].tolist())


def _setup(F, mode, eps=0.5, draw_seed=3, K=28, n=64):
    _stream()
    L = ddqn.DDQNLearner(n_state=F, device="cuda", seed=NET_SEED, fused_act=True, mode=mode)
    L._eps.fill_(eps)
    task = ddqn.ExecutionTask(device="cuda", features=R.to_features(R.FEATURE_SETS[F]))
    g = torch.Generator(device="cuda")
    g.manual_seed(draw_seed)
    u = torch.rand((K, n), generator=g, dtype=torch.float64, device="cuda")
    rnd = torch.randint(0, L.n_actions, (K, n), generator=g, device="cuda")
    return L, task, u, rnd


def _per_step(v, L, task, rows, r0, r1, first_zero, enough, u, rnd):
    """rows r0 .. r1-1 one launch per kernel: the path run_episode(rollout=False) takes"""
    n = v.n_envs
    test = L.mode == "test"
    s = torch.empty((n, task.n_state), dtype=torch.float32, device="cuda")
    for r in range(r0, r1):
        if first_zero and r == r0:
            rows.a[r].fill_(-1)
            rows.act[r].zero_()
        else:
            obs = rows.obs[r - 1]
            ddqn._call("mxa_ddqn_state_spec", n, OBS_SIZE, obs.data_ptr(), ctypes.byref(task.spec), s.data_ptr())
            ddqn._call("mxa_qnet_act", n, s.data_ptr(), L.eflat.data_ptr(), len(L._qdims) - 1, L._qdims, int(test),
                       int(enough), None if test else u[r].data_ptr(), None if test else rnd[r].data_ptr(),
                       L._eps.data_ptr(), OBS_SIZE, obs.data_ptr(), task.table.data_ptr(), task.q0, rows.a[r].data_ptr(),
                       rows.act[r].data_ptr(), None)
        v.step_device(rows.act[r].data_ptr(), rows.obs[r].data_ptr(), rows.flags[r].data_ptr())
        v.write_rl_state(rows.st[r].data_ptr())


def _launch(v, L, task, rows, r0, k, first_zero, enough, u, rnd, state=True):
    test = L.mode == "test"
    pol = L.policy(task, test, enough, None if test else u[r0:], None if test else rnd[r0:])
    v.step_policy_device(k, pol, rows.obs[r0].data_ptr(), rows.flags[r0].data_ptr(), rows.a[r0].data_ptr(),
                         rows.act[r0].data_ptr(), rows.st[r0].data_ptr() if state else None, first_zero=first_zero,
                         spec=task.spec)


def _reference(kind, F, mode, enough, K, n):
    """the per-step side of one case, run once and left unchanged: (learner, task, u, rnd, rows, summary)"""
    key = (kind, F, mode, enough, K, n)
    if key not in _CACHE:
        L, task, u, rnd = _setup(F, mode, K=K, n=n)
        v = _make(kind, n)
        rows = Rows(K, n)
        _per_step(v, L, task, rows, 0, K, True, enough, u, rnd)
        torch.cuda.synchronize()
        _CACHE[key] = (L, task, u, rnd, rows, v.summary())
        v.close()
    return _CACHE[key]


def _assert_summary(v, want, what):
    torch.cuda.synchronize()
    got = v.summary()
    for key in KEYS:
        assert (got[key] == want[key]).all(), (what, key)


@pytest.mark.parametrize("mode,enough", [("test", 0), ("train", 1)])
def test_gpu_step_policy_spec_rmsc03_rl_equals_per_step_path(mode, enough):
    K, n, F = 28, 64, 6
    assert [f[0] for f in R.FEATURE_SETS[F]] == [0, 1, 3, 4, 2, 6]
    L, task, u, rnd, ref, summ = _reference("rmsc03_rl", F, mode, enough, K, n)
    # conditions on the inputs: some env is done or errored before the last step, so the launch carries
    # finished envs through later steps; the policy is consulted on live envs; the market columns move
    ended = (ref.flags[:-1] & 5) != 0
    print("%s: envs ended after each step but the last %s; actions %s" % (
        mode, ended.sum(1).tolist(), sorted(set(ref.a[1:].reshape(-1).tolist()))))
    assert bool(ended.any()) and not bool(ended[1].all())
    assert bool((ref.a[0] == -1).all()) and int(ref.a[1:].min()) >= 0 and int(ref.a[1:].max()) < 24
    for col in (3, 4, 2, 6):
        assert len(torch.unique(ref.obs[:, :, col])) > 2, col
    if mode == "train":  # exploration: epsilon sends some envs each way
        exploit = u[1:] < 0.5
        assert 0.3 < float(exploit.double().mean()) < 0.7
        assert torch.equal(ref.a[1:][~exploit], rnd[1:][~exploit]) and not torch.equal(ref.a[1:], rnd[1:])
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, K, True, enough, u, rnd)
    torch.cuda.synchronize()
    rows.assert_equal(ref, (mode, enough))
    _assert_summary(v, summ, (mode, enough))
    v.close()


def test_gpu_step_policy_spec_eight_features_on_the_ibm_replay_tape():
    K, n, F = 40, 8, 8
    L, task, u, rnd, ref, summ = _reference("replay", F, "train", 1, K, n)
    v = _make("replay", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, K, True, 1, u, rnd)
    torch.cuda.synchronize()
    rows.assert_equal(ref, "replay")
    _assert_summary(v, summ, "replay")
    assert bool(((ref.flags & 2) != 0).any())  # observations were valid: the policy saw live states
    v.close()


@pytest.mark.parametrize("plan", ["run_episode's chunks", "per-step rows, then two launches"])
def test_gpu_step_policy_spec_splits_into_launches(plan):
    K, n, F = 28, 64, 6
    L, task, u, rnd, ref, summ = _reference("rmsc03_rl", F, "train", 1, K, n)
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    if plan == "run_episode's chunks":
        r0 = 0
        for first_zero, k in ddqn.rollout_chunks(27, 5, True):
            _launch(v, L, task, rows, r0, k, first_zero, 1, u, rnd)
            r0 += k
        assert r0 == K
    else:
        _per_step(v, L, task, rows, 0, 7, True, 1, u, rnd)
        _launch(v, L, task, rows, 7, 10, False, 1, u, rnd)
        _launch(v, L, task, rows, 17, K - 17, False, 1, u, rnd)
    torch.cuda.synchronize()
    rows.assert_equal(ref, plan)
    _assert_summary(v, summ, plan)
    v.close()


def test_gpu_step_policy_spec_null_state_pointer():
    K, n, F = 28, 64, 6
    L, task, u, rnd, ref, summ = _reference("rmsc03_rl", F, "test", 0, K, n)
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, K, True, 0, u, rnd, state=False)
    torch.cuda.synchronize()
    rows.assert_equal(ref, "null state", state=False)
    assert bool((rows.st == -7.25).all())
    _assert_summary(v, summ, "null state")
    v.close()


# ---------------------------------------------------------------- the meaning check
def _bin_net(F, f):
    """the one-layer net [F, 24] with q_a = 2 a s_f - a^2 = s_f^2 - (a - s_f)^2: integers, exact in fp32 in
    any summation order for bins below 2^11; its argmax is min(s_f, 23). The flat parameters as
    mxa_qnet_* take them: weight [24][F] row-major, then bias [24]"""
    W = np.zeros((24, F), dtype=np.float32)
    W[:, f] = 2.0 * np.arange(24)
    return torch.from_numpy(np.concatenate([W.reshape(-1), -np.arange(24.0, dtype=np.float32) ** 2])).cuda()


def _run_bin_policy(feats, f, K=28, n=64):
    """K periods of rmsc03 + DummyRL x n in one launch under the bin net in test mode; (a [K, n], obs [K, n, 9])"""
    _stream()
    F = len(feats)
    task = ddqn.ExecutionTask(device="cuda", features=R.to_features(feats))
    params = _bin_net(F, f)
    p = _lib.Policy()
    p.params, p.n_layers = params.data_ptr(), 1
    p.dims[0], p.dims[1] = F, 24
    p.q0, p.table, p.test = task.q0, task.table.data_ptr(), 1
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    v.step_policy_device(K, p, rows.obs.data_ptr(), rows.flags.data_ptr(), rows.a.data_ptr(), rows.act.data_ptr(),
                         None, first_zero=True, spec=task.spec)
    torch.cuda.synchronize()
    v.close()
    return rows.a.cpu().numpy(), rows.obs.cpu().numpy()


def _assert_actions_are_the_bins(a, obs, feats, f):
    K, n = a.shape
    assert (a[0] == -1).all()
    want = R.state_ref(obs[:-1].reshape(-1, OBS_SIZE), feats)[:, f].reshape(K - 1, n)
    assert not np.isnan(want).any()
    assert np.array_equal(a[1:], np.minimum(want, 23).astype(np.int64))
    return want


def test_gpu_step_policy_spec_actions_are_the_time_bins():
    # feature 1 of 2 (lane 1 of the wave): remaining time on 23 split points, bin = min(time, 23)
    feats = [R.IMBALANCE, (0, np.arange(23) + 0.5, 1.0, 1.0, 0.0)]
    a, obs = _run_bin_policy(feats, 1)
    want = _assert_actions_are_the_bins(a, obs, feats, 1)
    assert np.array_equal(want, np.minimum(obs[:-1, :, 0], 23))  # integer remaining times: the bin is the time
    assert len(np.unique(a[1:])) >= 20


def _fixture_spreads():
    with open(os.path.join(GOLD, SPREAD_FIXTURE + ".json")) as f:  # the observations recorded beside the .npz
        d = json.load(f)
    return np.array([st["obs"][3] for ep in d["episodes"] for st in ep["steps"] if st.get("obs")])


def _spread_splits():
    u = np.unique(_fixture_spreads())
    return (u[1:] + u[:-1]) / 2  # between every two spreads the reference run saw


def test_gpu_step_policy_spec_actions_are_the_spread_bins():
    splits = _spread_splits()
    assert len(np.unique(np.digitize(_fixture_spreads(), splits))) >= 3  # (on the CPU) the fixture's own spreads spread out
    feats = [(3, splits, 1.0, 1.0, 0.0), R.IMBALANCE]  # feature 0 of 2: the spread
    a, obs = _run_bin_policy(feats, 0)
    _assert_actions_are_the_bins(a, obs, feats, 0)
    print("spread bins across the rows:", np.unique(a[1:], return_counts=True))
    assert len(np.unique(a[1:])) >= 2  # not a constant


# ---------------------------------------------------------------- refused calls
def test_gpu_step_policy_spec_refused_calls_leave_the_envs_alone():
    K, n, F = 3, 8, 6
    L, task, u, rnd = _setup(F, "train", K=K, n=n)
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, 1, True, 1, u, rnd)  # one good step, so the blocks are mid-episode
    torch.cuda.synchronize()
    before = v.summary()
    lib = _lib.load()
    P = ctypes.c_void_p
    ptr = [P(t[1].data_ptr()) for t in (rows.obs, rows.flags, rows.a, rows.act, rows.st)]

    def rc(spec, pol=None, k=2):
        p = L.policy(task, False, 1, u[1:], rnd[1:]) if pol is None else pol
        return lib.mxa_step_policy_spec(v._h, k, 0, ctypes.byref(p), None if spec is None else ctypes.byref(spec), *ptr)

    def edited(edit):
        sp = _lib.StateSpec.from_buffer_copy(task.spec)
        edit(sp)
        return sp

    def setf(name, val, i=None):
        def f(sp):
            if i is None:
                setattr(sp, name, val)
            else:
                getattr(sp, name)[i] = val
        return f

    def decreasing(sp):
        sp.goff[2] = sp.goff[1] - 1

    def too_many(sp):
        for i in range(3, 9):
            sp.goff[i] = (1 << 20) + 1

    assert rc(None) == -1 and b"null state spec" in lib.mxa_last_error(v._h)
    for edit in (setf("n_feat", 0), setf("n_feat", 9), setf("n_feat", 5), setf("col", -1, 0), setf("col", 9, 5),
                 setf("div", 0.0, 1), setf("div", float("nan"), 2), setf("mul", float("inf"), 3),
                 setf("add", float("nan"), 4), setf("goff", 1, 0), decreasing, too_many, setf("grid", None)):
        assert rc(edited(edit)) == -1, edit  # MXA_EINVAL
        assert lib.mxa_last_error(v._h).startswith(b"mxa_step_policy_spec: ")
    # dims[0] != n_feat, from the policy's side too; and what mxa_step_policy refuses
    L2 = ddqn.DDQNLearner(device="cuda", seed=NET_SEED, fused_act=True)
    assert rc(task.spec, pol=L2.policy(ddqn.ExecutionTask(device="cuda"), False, 1, u[1:], rnd[1:])) == -1
    assert b"dims[0] != n_feat" in lib.mxa_last_error(v._h)
    assert rc(task.spec, k=0) == -1
    # mxa_step_policy itself still wants two state elements
    p6 = L.policy(task, False, 1, u[1:], rnd[1:])
    g = ddqn.ExecutionTask(device="cuda").grid
    p6.grid0, p6.n0, p6.grid1, p6.n1, p6.nh = g[0].data_ptr(), g[0].numel(), g[1].data_ptr(), g[1].numel(), 27.0
    assert p6.dims[0] == 6 and lib.mxa_step_policy(v._h, 2, 0, ctypes.byref(p6), *ptr) == -1
    torch.cuda.synchronize()
    after = v.summary()
    for key in KEYS:
        assert (before[key] == after[key]).all(), key
    assert bool((rows.a[1:] == -7).all()) and bool((rows.obs[1:] == -7.25).all())
    # and the handle still steps
    assert rc(task.spec) == 0
    torch.cuda.synchronize()
    assert (v.summary()["events"] >= before["events"]).all() and bool((rows.a[1:] >= 0).all())
    v.close()
