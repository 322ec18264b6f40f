"""k periods per launch with the Q-network policy inside the step kernel (include/mxa.h
mxa_step_policy): every row of a launch (observation, flags, action index, action vector, the
execution agent's state) and the env blocks (events, per-pop parity hash, status, error, time) equal,
bit for bit, the per-step sequence mxa_ddqn_state, mxa_qnet_act, mxa_step_device,
mxa_write_rl_state on a second handle: rmsc03 + DummyRL with envs that end inside the launch, test
and train mode, the IBM replay tape, any split of the episode into launches, a null state pointer;
and every refused argument leaves the env blocks alone."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mxabides import _lib, ddqn, tape
from mxabides.gym import OBS_SIZE, RL_STATE_WORDS, VecABIDESEnv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NET_SEED = 5
KEYS = ("events", "hash", "status", "err", "current_time")
_CACHE = {}


def _stream():
    """one non-default stream for the handles and the learner's kernels alike (a handle given the
    null stream steps on a stream of its own)"""
    if "stream" not in _CACHE:
        _CACHE["stream"] = torch.cuda.Stream()
    torch.cuda.set_stream(_CACHE["stream"])
    return _CACHE["stream"]


def _make(kind, n):
    stream = _stream()
    if kind == "replay":
        v = VecABIDESEnv(tape.Tape.load(os.path.join(GOLD, "tape_IBM_2003-01-14.npz")), n)
    else:
        v = VecABIDESEnv(seeds=(123456789 + np.arange(n)) & 0xFFFFFFFF)  # test_gpu_step_many's
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


def _setup(mode, eps=0.5, draw_seed=3, K=28, n=64):
    _stream()
    L = ddqn.DDQNLearner(device="cuda", seed=NET_SEED, fused_act=True, mode=mode)
    L._eps.fill_(eps)
    task = ddqn.ExecutionTask(device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(draw_seed)
    u = torch.rand((K, n), generator=g, dtype=torch.float64, device="cuda")
    rnd = torch.randint(0, L.n_actions, (K, n), generator=g, device="cuda")
    return L, task, u, rnd


def _per_step(v, L, task, rows, r0, r1, first_zero, enough, u, rnd):
    """rows r0 .. r1-1 one launch per kernel: the path run_episode(rollout=False) takes"""
    n = v.n_envs
    test = L.mode == "test"
    s = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    for r in range(r0, r1):
        if first_zero and r == r0:
            rows.a[r].fill_(-1)
            rows.act[r].zero_()
        else:
            obs = rows.obs[r - 1]
            ddqn._state_device(task, obs, s)
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
                         rows.act[r0].data_ptr(), rows.st[r0].data_ptr() if state else None, first_zero=first_zero)


def _reference(kind, mode, enough, K, n):
    """the per-step side of one case, run once and left unchanged: (learner, task, u, rnd, rows, summary)"""
    key = (kind, mode, enough, K, n)
    if key not in _CACHE:
        L, task, u, rnd = _setup(mode, K=K, n=n)
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


@pytest.mark.parametrize("mode,enough", [("test", 0), ("train", 0), ("train", 1)])
def test_gpu_step_policy_rmsc03_rl_equals_per_step_path(mode, enough):
    K, n = 28, 64
    L, task, u, rnd, ref, summ = _reference("rmsc03_rl", mode, enough, K, n)
    # a condition on the inputs: some env is done or errored before the last step, so the launch
    # carries finished envs through later steps; and the policy is consulted on live envs
    ended = (ref.flags[:-1] & 5) != 0
    print("%s enough %d: envs ended after each step but the last %s, %d with the env error; actions %s" % (
        mode, enough, ended.sum(1).tolist(), int(((ref.flags[:-1] & 4) != 0).any(0).sum()),
        sorted(set(ref.a[1:].reshape(-1).tolist()))[:24]))
    assert bool(ended.any()) and not bool(ended[1].all())
    assert bool((ref.a[0] == -1).all()) and int(ref.a[1:].min()) >= 0 and int(ref.a[1:].max()) < 24
    if mode == "train":  # epsilon sends some envs each way when there is enough experience
        exploit = u[1:] < 0.5
        assert 0.3 < float(exploit.double().mean()) < 0.7
        if not enough:
            assert torch.equal(ref.a[1:], rnd[1:])
        else:
            assert torch.equal(ref.a[1:][~exploit], rnd[1:][~exploit])
            assert not torch.equal(ref.a[1:], rnd[1:])
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, K, True, enough, u, rnd)
    torch.cuda.synchronize()
    rows.assert_equal(ref, (mode, enough))
    _assert_summary(v, summ, (mode, enough))
    v.close()


def test_gpu_step_policy_ibm_replay_tape():
    K, n = 40, 8
    L, task, u, rnd, ref, summ = _reference("replay", "train", 1, K, n)
    v = _make("replay", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, K, True, 1, u, rnd)
    torch.cuda.synchronize()
    rows.assert_equal(ref, "replay")
    _assert_summary(v, summ, "replay")
    assert bool(((ref.flags & 2) != 0).any())  # observations were valid: the policy saw live states
    v.close()


@pytest.mark.parametrize("plan", ["one launch", "run_episode's chunks", "per-step rows, then a launch"])
def test_gpu_step_policy_any_split_into_launches(plan):
    K, n = 28, 64
    L, task, u, rnd, ref, summ = _reference("rmsc03_rl", "train", 1, K, n)
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    if plan == "one launch":
        _launch(v, L, task, rows, 0, K, True, 1, u, rnd)
    elif plan == "run_episode's chunks":
        chunks = ddqn.rollout_chunks(27, 5, True)
        assert [k for _, k in chunks] == [2, 5, 5, 5, 5, 5, 1]
        r0 = 0
        for first_zero, k in chunks:
            _launch(v, L, task, rows, r0, k, first_zero, 1, u, rnd)
            r0 += k
    else:
        _per_step(v, L, task, rows, 0, 7, True, 1, u, rnd)
        _launch(v, L, task, rows, 7, K - 7, False, 1, u, rnd)
    torch.cuda.synchronize()
    rows.assert_equal(ref, plan)
    _assert_summary(v, summ, plan)
    v.close()


def test_gpu_step_policy_null_state_pointer():
    K, n = 28, 64
    L, task, u, rnd, ref, summ = _reference("rmsc03_rl", "test", 0, K, n)
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, K, True, 0, u, rnd, state=False)
    torch.cuda.synchronize()
    rows.assert_equal(ref, "null state", state=False)
    assert bool((rows.st == -7.25).all())
    _assert_summary(v, summ, "null state")
    v.close()


def test_gpu_step_policy_refused_arguments_leave_the_envs_alone():
    import mxabides
    K, n = 3, 8
    L, task, u, rnd = _setup("train", K=K, n=n)
    v = _make("rmsc03_rl", n)
    rows = Rows(K, n)
    _launch(v, L, task, rows, 0, 1, True, 1, u, rnd)  # one good step, so the blocks are mid-episode
    torch.cuda.synchronize()
    before = v.summary()
    lib = _lib.load()
    P = ctypes.c_void_p

    def rc(h=v._h, k=2, pol=None, edit=None, **null):
        p = L.policy(task, False, 1, u[1:], rnd[1:]) if pol is None else pol
        if edit:
            edit(p)
        ptr = {"obs": rows.obs[1].data_ptr(), "flags": rows.flags[1].data_ptr(), "a": rows.a[1].data_ptr(),
               "act": rows.act[1].data_ptr(), "st": rows.st[1].data_ptr()}
        ptr.update(null)
        return lib.mxa_step_policy(h, k, 0, ctypes.byref(p) if p is not False else None, P(ptr["obs"]), P(ptr["flags"]),
                                   P(ptr["a"]), P(ptr["act"]), P(ptr["st"]))

    def setf(name, val):
        return lambda p: setattr(p, name, val)

    def setdim(i, val):
        def f(p):
            p.dims[i] = val
        return f

    plain = mxabides.VecMarket("rmsc03", [7, 11], device=0)  # a Kernel.runner handle, not a GymKernel one
    bad = [dict(h=None), dict(h=plain._h), dict(k=0), dict(k=-1), dict(pol=False), dict(obs=None), dict(flags=None),
           dict(a=None), dict(act=None)]
    bad += [dict(edit=setf(f, None)) for f in ("params", "grid0", "grid1", "table", "u", "rnd", "eps")]
    bad += [dict(edit=setf("n_layers", 0)), dict(edit=setf("n_layers", 9)), dict(edit=setdim(0, 3)),
            dict(edit=setdim(0, 1)), dict(edit=setdim(3, 0)), dict(edit=setdim(3, 257)), dict(edit=setdim(7, -1)),
            dict(edit=setf("n0", -1)), dict(edit=setf("n1", -1))]
    for case in bad:
        assert rc(**case) == -1, case  # MXA_EINVAL
    torch.cuda.synchronize()
    after = v.summary()
    for key in KEYS:
        assert (before[key] == after[key]).all(), key
    assert bool((rows.a[1:] == -7).all()) and bool((rows.obs[1:] == -7.25).all())
    # test mode takes null u, rnd and eps; and the handle still steps
    def test_mode(p):
        p.test, p.u, p.rnd, p.eps = 1, None, None, None
    assert rc(edit=test_mode) == 0
    torch.cuda.synchronize()
    assert (v.summary()["events"] >= before["events"]).all() and bool((rows.a[1:] >= 0).all())
    plain.close() if hasattr(plain, "close") else None
    v.close()
