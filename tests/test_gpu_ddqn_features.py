"""include/mxa_ddqn_features.h (libmxa_ddqn_features.so) on the GPU: mxa_ddqn_state_spec against the plain numpy reference
(tests/ddqn_features_ref.py) at the 256-thread block edges, mxa_ddqn_period_spec against the PyTorch
ops of run_episode(fused=False) on a features task (mxabides.ddqn.period_torch) at the 1024-lane
walk's edges with a wrapping ring, both through the default spec against today's mxa_ddqn_state and
mxa_ddqn_period bit for bit, and every refused argument, which leaves the outputs alone."""
import ctypes

import numpy as np
import pytest
import torch

import ddqn_features_ref as R
import ddqn_kernel_util as U
from mxabides import _lib, ddqn

pytestmark = pytest.mark.gpu
HIP_ERROR_INVALID_VALUE = 1


def _task(feats):
    return ddqn.ExecutionTask(device="cuda", features=R.to_features(feats))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits_equal(x, y):
    """two device tensors bit for bit; in float tensors a NaN equals a NaN (a passed-through NaN's
    payload is not part of the contract)"""
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    if x.dtype in (torch.float32, torch.float64):
        ix = x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)
        iy = y.contiguous().view(ix.dtype)
        return bool(((ix == iy) | (torch.isnan(x) & torch.isnan(y))).all())
    return bool(torch.equal(x, y))


# ---------------------------------------------------------------- mxa_ddqn_state_spec
@pytest.mark.parametrize("F", [1, 2, 6, 8])
def test_gpu_state_spec_equals_numpy_reference(F):
    feats = R.FEATURE_SETS[F]
    task = _task(feats)
    for n in (1, 255, 256, 257, R.pool_rows(feats)):  # the block edges; the last walks every column's whole pool
        obs = R.edge_obs(n, feats, seed=n)
        want = R.state_ref(obs, feats)
        o = U.Guarded(obs)
        out = U.Guarded(np.full((n, F), -5.0, dtype=np.float32))
        rc = ddqn.features_lib().mxa_ddqn_state_spec(_stream(), n, R.OBS_W, o.ptr, ctypes.byref(task.spec), out.ptr)
        assert rc == 0
        torch.cuda.synchronize()
        got = out.read(("state_spec", F, n))
        assert R.same_state(got, want), (F, n, np.flatnonzero((got != want).any(1) & ~np.isnan(want).any(1))[:5])
        # the device's PyTorch ops (the fused=False path) give the same rows
        assert R.same_state(task.state(torch.from_numpy(obs).cuda()).cpu().numpy(), want), (F, n)


def test_gpu_state_spec_default_spec_is_mxa_ddqn_state_bit_for_bit():
    old = ddqn.ExecutionTask(device="cuda")
    new = ddqn.ExecutionTask(device="cuda", features=ddqn.default_features())
    feats = R.FEATURE_SETS[2]
    for n in (1, 255, 256, 257, R.pool_rows(feats)):
        obs = torch.from_numpy(R.edge_obs(n, feats, seed=3 + n)).cuda()
        a = ddqn._state_device(old, obs, torch.full((n, 2), -5.0, dtype=torch.float32, device="cuda"))
        b = ddqn._state_device(new, obs, torch.full((n, 2), -6.0, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
    # every quantity at one remaining time, the 73 where a reciprocal would differ included
    q = torch.arange(100001, dtype=torch.float64, device="cuda")
    obs = torch.zeros((len(q), 9), dtype=torch.float64, device="cuda")
    obs[:, 0], obs[:, 1] = 13.0, q
    a = ddqn._state_device(old, obs, torch.empty((len(q), 2), dtype=torch.float32, device="cuda"))
    b = ddqn._state_device(new, obs, torch.empty((len(q), 2), dtype=torch.float32, device="cuda"))
    assert torch.equal(a, b)
    assert np.array_equal(b.cpu().numpy(), R.state_ref(obs.cpu().numpy(), feats))


# ---------------------------------------------------------------- mxa_ddqn_period_spec
def _period_inputs(n, F, feats, seed):
    """one period's device inputs: ddqn_kernel_util.make_case's mixed alive / flags pattern and reward
    inputs, with edge-value observations"""
    c = U.make_case(n, seed, "half", cap=n + 3)
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return {"obs": dv(R.edge_obs(n, feats, seed=seed)), "st": dv(c["st"]), "prev": dv(c["prev"]), "arrival": dv(c["arrival"]),
            "flags": dv(c["flags"]), "alive": dv(c["alive"]), "a": dv(c["a"]), "env_steps": dv(c["env_steps"])}


def _ring(cap, F, seed):
    g = torch.Generator().manual_seed(seed)
    m = ddqn.ReplayRing(cap, F, "cuda")
    m.s = torch.randint(0, 200, (cap + 1, F), generator=g).float().cuda()
    m.s2 = torch.randint(0, 200, (cap + 1, F), generator=g).float().cuda()
    m.a = torch.randint(0, 24, (cap + 1,), generator=g).cuda()
    m.r = torch.randn(cap + 1, generator=g).float().cuda()
    m.n_dev = torch.tensor(7 * cap + cap // 2, dtype=torch.int64, device="cuda")  # mid-ring: the first call wraps already
    return m


def _two_periods(period, task, n, F, feats, cap, train, seed):
    """two chained periods through `period` (period_torch or period_kernel); every output of both"""
    m = _ring(cap, F, seed)
    stored = torch.tensor(1000, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(seed + 1)
    s = torch.randint(0, 200, (n, F), generator=g).float().cuda()
    alive, env_steps, outs = None, None, []
    for k in range(2):
        c = _period_inputs(n, F, feats, seed + 10 * k)
        alive = c["alive"] if alive is None else alive
        env_steps = c["env_steps"].clone() if env_steps is None else env_steps
        r_row = torch.full((n,), -7.25, dtype=torch.float64, device="cuda")
        spare = (torch.full((n, F), -5.0, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda"),
                 torch.zeros((), dtype=torch.bool, device="cuda"))
        s2, alive_next, live = period(task, m, train, c["obs"], c["st"], c["prev"], c["arrival"], c["flags"], alive, s,
                                      c["a"], env_steps, stored, r_row, spare)
        torch.cuda.synchronize()
        outs.append({"s2": s2.clone(), "alive_next": alive_next.clone(), "live": live.clone().reshape(()),
                     "r_row": r_row.clone(), "env_steps": env_steps.clone(), "stored": stored.clone(),
                     "n_dev": m.n_dev.clone(), "ring_s": m.s[:cap].clone(), "ring_s2": m.s2[:cap].clone(),
                     "ring_a": m.a[:cap].clone(), "ring_r": m.r[:cap].clone(),
                     "spare_row": (m.s[cap].clone(), m.s2[cap].clone(), m.a[cap].clone(), m.r[cap].clone())})
        s, alive = s2.clone(), alive_next.clone()
    return outs


def _assert_periods_equal(got, want, what, skip=("spare_row",)):
    for k, (g, w) in enumerate(zip(got, want)):
        for name in w:
            if name not in skip:
                pairs = zip(g[name], w[name]) if isinstance(w[name], tuple) else [(g[name], w[name])]
                assert all(_bits_equal(x, y) for x, y in pairs), (what, "period", k, name)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_gpu_period_spec_equals_period_torch(n):
    F, feats = 6, R.FEATURE_SETS[6]
    task = _task(feats)
    stored = 0
    for cap in (n, n + 3):
        want = _two_periods(ddqn.period_torch, task, n, F, feats, cap, True, seed=n)
        got = _two_periods(ddqn.period_kernel, task, n, F, feats, cap, True, seed=n)
        _assert_periods_equal(got, want, (n, cap))
        # the kernel never writes the ring's spare row (period_torch parks its masked-out rows there)
        fresh = _ring(cap, F, n)
        for x, y in zip(got[1]["spare_row"], (fresh.s[cap], fresh.s2[cap], fresh.a[cap], fresh.r[cap])):
            assert _bits_equal(x, y), (n, cap, "spare row")
        # conditions on the inputs: a mixed mask, rows stored, and the ring wrapped
        added = int(got[1]["stored"]) - 1000
        assert int(got[1]["n_dev"]) == 7 * cap + cap // 2 + added
        stored += added
        if n > 1:
            assert 0 < added < 2 * n and cap // 2 + added > cap, (n, cap, added)
            assert bool(got[0]["alive_next"].any()) and not bool(got[0]["alive_next"].all())
            assert bool(torch.isnan(got[0]["s2"]).any())  # a passed-through NaN reaches the rows
    assert stored > 0 or n == 1


def test_gpu_period_spec_default_spec_is_mxa_ddqn_period_bit_for_bit():
    feats = R.FEATURE_SETS[2]
    old = ddqn.ExecutionTask(device="cuda")
    new = ddqn.ExecutionTask(device="cuda", features=ddqn.default_features())
    for n in (1, 1024, 2049):
        want = _two_periods(ddqn.period_kernel, old, n, 2, feats, n + 3, True, seed=50 + n)
        got = _two_periods(ddqn.period_kernel, new, n, 2, feats, n + 3, True, seed=50 + n)
        _assert_periods_equal(got, want, n, skip=())
        assert int(got[1]["stored"]) > 1000 or n == 1


def test_gpu_period_spec_without_train_writes_no_ring_row():
    n, F, feats = 1025, 6, R.FEATURE_SETS[6]
    task = _task(feats)
    want = _two_periods(ddqn.period_torch, task, n, F, feats, n, False, seed=9)
    got = _two_periods(ddqn.period_kernel, task, n, F, feats, n, False, seed=9)
    _assert_periods_equal(got, want, "train=0", skip=("spare_row", "ring_s", "ring_s2", "ring_a", "ring_r"))
    fresh = _ring(n, F, 9)
    for name, t in (("ring_s", fresh.s), ("ring_s2", fresh.s2), ("ring_a", fresh.a), ("ring_r", fresh.r)):
        assert _bits_equal(got[1][name], t[:n]), name
    assert int(got[1]["stored"]) == 1000 and int(got[1]["n_dev"]) == 7 * n + n // 2
    assert bool((got[1]["r_row"] != 0).any())  # the other outputs were still made


# ---------------------------------------------------------------- refused arguments
def _edit(field, i, val):
    def f(sp):
        if i is None:
            setattr(sp, field, val)
        else:
            getattr(sp, field)[i] = val
    return f


def _decreasing(sp):
    sp.goff[2] = sp.goff[1] - 1


def _too_many(sp):
    for i in range(3, 9):
        sp.goff[i] = (1 << 20) + 1


BAD_SPECS = [_edit("n_feat", None, 0), _edit("n_feat", None, 9), _edit("n_feat", None, -1), _edit("col", 2, -1),
             _edit("col", 5, 9), _edit("div", 0, 0.0), _edit("div", 3, float("inf")), _edit("div", 5, float("nan")),
             _edit("mul", 1, float("inf")), _edit("mul", 4, float("nan")), _edit("add", 2, float("nan")),
             _edit("add", 0, float("-inf")), _edit("goff", 0, 1), _decreasing, _too_many, _edit("grid", None, None)]


def test_gpu_spec_exports_refuse_bad_arguments_and_write_nothing():
    n, F, feats = 300, 6, R.FEATURE_SETS[6]
    task = _task(feats)
    L = ddqn.features_lib()
    c = _period_inputs(n, F, feats, 4)
    m = _ring(n, F, 4)
    f32 = lambda *shape: torch.full(shape, -5.0, dtype=torch.float32, device="cuda")
    s, s2, out = f32(n, F), f32(n, F), f32(n, F)
    r_row = torch.full((n,), -7.25, dtype=torch.float64, device="cuda")
    alive_next = torch.zeros(n, dtype=torch.bool, device="cuda")
    live = torch.zeros((), dtype=torch.bool, device="cuda")
    stored = torch.tensor(1000, dtype=torch.int64, device="cuda")
    before = [t.clone() for t in (m.s, m.s2, m.a, m.r, m.n_dev, c["env_steps"])]

    def state(spec, n_=n, obs_w=R.OBS_W):
        return L.mxa_ddqn_state_spec(_stream(), n_, obs_w, c["obs"].data_ptr(), spec, out.data_ptr())

    def period(spec, n_=n, obs_w=R.OBS_W, st_w=8, cap=n):
        return L.mxa_ddqn_period_spec(_stream(), n_, obs_w, st_w, 1, c["obs"].data_ptr(), c["st"].data_ptr(),
                                      c["prev"].data_ptr(), c["arrival"].data_ptr(), c["flags"].data_ptr(),
                                      c["alive"].data_ptr(), alive_next.data_ptr(), live.data_ptr(), s.data_ptr(),
                                      c["a"].data_ptr(), s2.data_ptr(), r_row.data_ptr(), c["env_steps"].data_ptr(), spec,
                                      task.q0, 1e4 / task.q0, m.s.data_ptr(), m.s2.data_ptr(), m.a.data_ptr(),
                                      m.r.data_ptr(), cap, m.n_dev.data_ptr(), stored.data_ptr())

    for edit in BAD_SPECS:
        sp = _lib.StateSpec.from_buffer_copy(task.spec)
        edit(sp)
        assert state(ctypes.byref(sp)) == HIP_ERROR_INVALID_VALUE, edit
        assert period(ctypes.byref(sp)) == HIP_ERROR_INVALID_VALUE, edit
    good = ctypes.byref(task.spec)
    assert state(None) == HIP_ERROR_INVALID_VALUE and period(None) == HIP_ERROR_INVALID_VALUE  # a null spec
    assert state(good, n_=-1) == HIP_ERROR_INVALID_VALUE and state(good, obs_w=6) == HIP_ERROR_INVALID_VALUE  # column 6
    for kw in (dict(n_=-1), dict(obs_w=6), dict(st_w=2), dict(cap=0), dict(cap=n - 1)):  # mxa_ddqn_period's own guards
        assert period(good, **kw) == HIP_ERROR_INVALID_VALUE, kw
    torch.cuda.synchronize()
    assert bool((out == -5.0).all()) and bool((s2 == -5.0).all()) and bool((r_row == -7.25).all())
    assert not bool(alive_next.any()) and int(stored) == 1000
    for t, b in zip((m.s, m.s2, m.a, m.r, m.n_dev, c["env_steps"]), before):
        assert torch.equal(t, b)
    # and the good arguments are taken
    assert state(good) == 0 and period(good) == 0 and state(good, n_=0) == 0
    torch.cuda.synchronize()
    assert not bool((out == -5.0).any()) and int(stored) > 1000
