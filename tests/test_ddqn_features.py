"""A DDQN state of N features (mxabides.ddqn Feature, ExecutionTask(features=...); include/
mxa_state_spec.h) on the CPU: ExecutionTask.state in PyTorch ops equals the plain numpy reference
(tests/ddqn_features_ref.py) exactly on every edge value, the default spec is today's two-element
state for every quantity and remaining time, and the host refuses what it must."""
import numpy as np
import pytest
import torch

import ddqn_features_ref as R
from mxabides import ddqn


def _task(feats):
    return ddqn.ExecutionTask(device="cpu", features=R.to_features(feats))


@pytest.mark.parametrize("F", [1, 2, 6, 8])
def test_state_equals_numpy_reference_on_edge_values(F):
    feats = R.FEATURE_SETS[F]
    obs = R.edge_obs(R.pool_rows(feats), feats, seed=F)
    task = _task(feats)
    assert task.n_state == F and task.spec.n_feat == F
    got = task.state(torch.from_numpy(obs)).numpy()
    want = R.state_ref(obs, feats)
    assert got.dtype == np.float32 and got.shape == (len(obs), F)
    assert R.same_state(got, want), np.flatnonzero((got != want).any(1) & ~np.isnan(want).any(1))[:5]
    # conditions on the inputs: the rows hold what the test is about
    for f, (col, splits, mul, div, add) in enumerate(feats):
        x = obs[:, col]
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert (np.signbit(x) & (x == 0)).any(), "no -0.0 in column %d" % col
        if not len(splits):  # a pass-through feature: the value itself, NaN and infinities included
            assert np.isnan(want[:, f]).any() and np.isinf(want[:, f]).any()
            continue
        assert set(np.unique(want[:, f])) >= {0.0, float(len(splits))}, "below the first / above the last point"
        if (mul, div, add) == (1.0, 1.0, 0.0):  # exactly on every split point, and next to it on both sides
            for k, p in enumerate(splits):
                assert (x == p).any() and (want[x == p, f] == k + 1).all()
                assert (want[x == np.nextafter(p, -np.inf), f] == k).all()
    if F >= 6:
        assert any(len(s) == 0 for _, s, _, _, _ in feats)


def test_default_spec_is_todays_state_for_every_quantity_and_time():
    import ddqn_ref
    q = np.arange(100001, dtype=np.float64)
    t = np.arange(28, dtype=np.float64)
    obs = np.zeros((len(q) * len(t), 9))
    obs[:, 0] = np.repeat(t, len(q))
    obs[:, 1] = np.tile(q, len(t))
    x = torch.from_numpy(obs)
    old = ddqn.ExecutionTask(device="cpu")
    new = ddqn.ExecutionTask(device="cpu", features=ddqn.default_features())
    assert old.spec is None and old.features is None and old.n_state == 2 and new.n_state == 2
    got = new.state(x)
    assert got.dtype == torch.float32 and torch.equal(got, old.state(x))
    g0, g1 = ddqn.create_uniform_grid([0, 0], [1.0, 1.0], ddqn.GRID_BINS)
    want = ddqn_ref.state_ref(obs, g0, g1, 27, 1e5)
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert np.array_equal(R.state_ref(obs, R.FEATURE_SETS[2]), want.astype(np.float32))
    # the 73 quantities where a reciprocal lands one bin off are among the rows
    recip = np.digitize(2 * (q * (1.0 / 1e5)) - 1, g1)
    assert int((recip != want[:len(q), 1]).sum()) == 73
    # the spec itself: today's columns, scales and grids
    sp = new.spec
    assert (sp.n_feat, list(sp.col[:2]), list(sp.mul[:2]), list(sp.div[:2]), list(sp.add[:2]), list(sp.goff[:3])) == \
        (2, [0, 1], [2.0, 2.0], [27.0, 1e5], [-1.0, -1.0], [0, 199, 398])
    assert np.array_equal(new._points.numpy(), np.concatenate([g0, g1]))


def test_feature_grids_and_named_columns():
    f = ddqn.Feature(ddqn.OBS_SPREAD, low=0.0, high=50.0, bins=10)
    assert np.array_equal(f.splits, ddqn.create_uniform_grid([0.0], [50.0], (10,))[0]) and len(f.splits) == 9
    assert len(ddqn.Feature(ddqn.OBS_LOG_RETURN).splits) == 0
    assert [ddqn.OBS_TIME_REMAINING, ddqn.OBS_QTY_REMAINING, ddqn.OBS_LOG_RETURN, ddqn.OBS_SPREAD,
            ddqn.OBS_VOLUME_IMBALANCE, ddqn.OBS_SMART_PRICE, ddqn.OBS_VOLATILITY, ddqn.OBS_TRADE_DIRECTION,
            ddqn.OBS_EFFECTIVE_SPREAD] == list(range(9))
    task = ddqn.ExecutionTask(device="cpu", features=[f, ddqn.Feature(2), ddqn.Feature(4, splits=[0.25, 0.5])])
    sp = task.spec
    assert sp.n_feat == 3 and list(sp.goff[:4]) == [0, 9, 9, 11] and list(sp.goff[4:]) == [11] * 5
    assert sp.grid == task._points.data_ptr()
    assert ddqn.ExecutionTask(device="cpu", features=[ddqn.Feature(2)]).spec.grid is None  # no points at all


@pytest.mark.parametrize("kw", [dict(col=3, splits=[0.0, 1.0, 1.0]), dict(col=3, splits=[2.0, 1.0]),
                                dict(col=3, splits=[0.0, float("nan")]), dict(col=3, div=0.0),
                                dict(col=3, div=float("inf")), dict(col=3, mul=float("nan")),
                                dict(col=3, add=float("-inf")), dict(col=9), dict(col=-1), dict(col=2.5),
                                dict(col=3, low=0.0, high=1.0, bins=4, splits=[0.5]), dict(col=3, low=1.0, high=1.0, bins=4),
                                dict(col=3, bins=4), dict(col=3, low=0.0, high=1.0)])
def test_feature_refuses(kw):
    with pytest.raises(ValueError):
        ddqn.Feature(**kw)


def test_task_refuses_bad_feature_lists():
    for bad in ([], [ddqn.Feature(0)] * 9, [(0, 1.0)]):
        with pytest.raises(ValueError):
            ddqn.ExecutionTask(device="cpu", features=bad)


def test_features_library_exports_and_refuses_on_the_host():
    """libmxa_ddqn_features.so exports what include/mxa_ddqn_features.h declares, libmxa.so the export of
    include/mxa_policy_features.h, and a refused spec returns before any HIP call (so without a GPU)"""
    import ctypes
    import os
    import re
    import subprocess

    from mxabides import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", src)))

    L = ddqn.features_lib()
    assert L is not None, "libmxa_ddqn_features.so not built (build_lib.build_ddqn)"
    assert declared("mxa_ddqn_features.h") == ["mxa_ddqn_period_spec", "mxa_ddqn_state_spec"]
    out = subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("mxa_")}
    assert exported == set(declared("mxa_ddqn_features.h"))
    assert declared("mxa_policy_features.h") == ["mxa_step_policy_spec"] == list(_lib.POLICY_FEATURES_BINDINGS)
    assert hasattr(_lib.load(), "mxa_step_policy_spec")
    # the struct's layout is the header's: 4 + 8 * 4 (+ 4 padding) + 3 * 64 + 8 + 9 * 4 (+ 4 padding)
    assert ctypes.sizeof(_lib.StateSpec) == 280 and _lib.StateSpec.mul.offset == 40 and _lib.StateSpec.goff.offset == 240
    task = _task(R.FEATURE_SETS[6])
    ONE = ctypes.c_void_p(16)  # a non-null pointer that is never read

    def edited(edit):
        sp = _lib.StateSpec.from_buffer_copy(task.spec)
        edit(sp)
        return ctypes.byref(sp)

    def put(name, val, i=None):
        def f(sp):
            if i is None:
                setattr(sp, name, val)
            else:
                getattr(sp, name)[i] = val
        return f

    def too_many(sp):
        for i in range(3, 9):
            sp.goff[i] = (1 << 20) + 1

    bad = [None] + [edited(e) for e in (
        put("n_feat", 0), put("n_feat", 9), put("col", -1, 0), put("col", 9, 5), put("div", 0.0, 1),
        put("div", float("inf"), 2), put("div", float("nan"), 3), put("mul", float("inf"), 4), put("add", float("nan"), 5),
        put("goff", 1, 0), put("goff", 100, 2), too_many, put("grid", None))]
    for sp in bad:
        assert L.mxa_ddqn_state_spec(None, 4, 9, ONE, sp, ONE) == 1  # hipErrorInvalidValue
        assert L.mxa_ddqn_period_spec(None, 4, 9, 8, 1, *[ONE] * 13, sp, 1e5, 0.1, ONE, ONE, ONE, ONE, 8, ONE, ONE) == 1
    good = ctypes.byref(task.spec)
    assert L.mxa_ddqn_state_spec(None, 4, 6, ONE, good, ONE) == 1   # column 6 of a 6-column row
    assert L.mxa_ddqn_state_spec(None, -1, 9, ONE, good, ONE) == 1
    assert L.mxa_ddqn_state_spec(None, 0, 9, ONE, good, ONE) == 0   # nothing to do, nothing launched
    # libmxa.so: refused before any HIP call too, a null handle included
    P = _lib.Policy()
    assert _lib.load().mxa_step_policy_spec(None, 1, 0, ctypes.byref(P), good, ONE, ONE, ONE, ONE, None) == -1
    assert b"mxa_step_policy_spec: null handle" in _lib.load().mxa_last_error(None)


def test_learner_and_task_widths_must_match():
    task6 = _task(R.FEATURE_SETS[6])
    task2 = ddqn.ExecutionTask(device="cpu")
    L2 = ddqn.DDQNLearner(device="cpu", seed=1)
    L6 = ddqn.DDQNLearner(n_state=6, device="cpu", seed=1)
    assert L6.n_state == 6 and tuple(L6.memory.s.shape[1:]) == (6,)

    class NoEnv:  # never reached: the widths are compared before the env is touched
        def __getattr__(self, name):
            raise AssertionError("run_episode touched the env (%s) before refusing the widths" % name)

    for learner, task in ((L2, task6), (L6, task2)):
        with pytest.raises(ValueError, match="does not match the task's state"):
            ddqn.run_episode(NoEnv(), learner, task, fused=False)
    # a matching pair acts on the task's states
    s = task6.state(torch.from_numpy(R.edge_obs(40, R.FEATURE_SETS[6])))
    s = torch.nan_to_num(s, nan=0.0, posinf=0.0, neginf=0.0)
    a = L6.choose_action(s)
    assert a.shape == (40,) and int(a.min()) >= 0 and int(a.max()) < ddqn.N_ACTIONS
