"""include/mxa_ddqn.h on the GPU, kernel by kernel: mxa_ddqn_period, mxa_ddqn_state and
mxa_ddqn_actions called through ddqn.lib() on synthetic device buffers, at the sizes and
inputs where they can go wrong (a second and third 1024-env block, full and single-lane waves, a
ring that wraps, train off, other row widths and grids, NaN / inf, every remaining quantity).
Every output is compared with exact equality against the plain float64 references of
oracle/ddqn_ref.py, and bitwise with this project's PyTorch ops on the device; every output buffer
sits between sentinel rows that must stay untouched."""
import numpy as np
import pytest
import torch

import ddqn_kernel_util as U
import ddqn_ref
from mxabides import ddqn

pytestmark = pytest.mark.gpu
CAP = 2200
Guarded = U.Guarded


def _lib():
    L = ddqn.lib()
    assert L is not None, "libmxa_ddqn.so not built (build_lib.build_ddqn)"
    return L


def run_period(c, what):
    """one mxa_ddqn_period call on the case's inputs; every output as numpy"""
    n = c["n"]
    b = {k: Guarded(c[k]) for k in ("obs", "st", "prev", "arrival", "flags", "alive", "s", "a", "env_steps", "g0", "g1",
                                    "ring_s", "ring_s2", "ring_a", "ring_r")}
    b["alive_next"] = Guarded(np.full(n, 0x5A, dtype=np.uint8))
    b["live"] = Guarded(np.full(1, 0x5A, dtype=np.uint8))
    b["s2"] = Guarded(np.full((n, 2), -3.0, dtype=np.float32))
    b["r_row"] = Guarded(np.full(n, -3.0, dtype=np.float64))
    b["n_dev"] = Guarded(np.array([c["n_dev"]], dtype=np.int64))
    b["stored"] = Guarded(np.array([c["stored"]], dtype=np.int64))
    torch.cuda.synchronize()
    rc = _lib().mxa_ddqn_period(torch.cuda.current_stream().cuda_stream, n, c["obs_w"], c["st_w"], c["train"],
                                b["obs"].ptr, b["st"].ptr, b["prev"].ptr, b["arrival"].ptr, b["flags"].ptr, b["alive"].ptr,
                                b["alive_next"].ptr, b["live"].ptr, b["s"].ptr, b["a"].ptr, b["s2"].ptr, b["r_row"].ptr,
                                b["env_steps"].ptr, b["g0"].ptr, c["n0"], b["g1"].ptr, c["n1"], c["nh"], c["q0"],
                                c["rscale"], b["ring_s"].ptr, b["ring_s2"].ptr, b["ring_a"].ptr, b["ring_r"].ptr,
                                c["cap"], b["n_dev"].ptr, b["stored"].ptr)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    out = {k: b[k].read((what, k)) for k in b}
    for k in ("obs", "st", "prev", "arrival", "flags", "s", "a", "g0", "g1"):  # the inputs are only read
        assert U.same(out[k], np.ascontiguousarray(c[k])), (what, k)
    assert set(np.unique(out["alive_next"]).tolist()) <= {0, 1} and out["live"][0] in (0, 1), what
    got = {k: out[k] for k in U.OUTPUTS}
    got["alive_next"] = out["alive_next"].astype(bool)
    got["live"], got["n_dev"], got["stored"] = bool(out["live"][0]), int(out["n_dev"][0]), int(out["stored"][0])
    return got


def check(c, what):
    """the kernel against period_ref (everything, the ring's spare row included) and against the
    PyTorch ops on the device (whose spare ring row takes the masked-out rows); returns the
    reference's outputs"""
    ref = U.reference(c)
    got = run_period(c, what)
    U.assert_outputs_equal(got, ref, (what, "period_ref"))
    U.assert_outputs_equal(got, U.torch_period(c, "cuda"), (what, "torch ops"), ring_rows=c["cap"])
    assert not np.isnan(got["r_row"]).any() and np.all(got["r_row"][~c["alive"]] == 0), what
    return ref


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2113])
def test_gpu_period_sizes_and_ok_patterns(n):
    """one, two and three blocks of 1024 envs (the `done` carry accumulates twice at 2113), with
    every ok pattern: all (a full 16-wave prefix), none, a random half, only lane 63 or only lane 0
    of every wave, only env 1024 (the first of the second block), only the last env; the ring starts
    5 rows before its end, so every appending case wraps"""
    for pattern in U.OK_PATTERNS:
        if (pattern == "env1024" and n < 1025) or (pattern == "last" and n == 0):
            continue
        c = U.make_case(n, 7 * n + 1, pattern, cap=CAP, n_dev=CAP - 5, stored=1000)
        ref = check(c, (n, pattern))
        want = {"all": n, "none": 0, "lane63": n // 64, "lane0": (n + 63) // 64, "env1024": 1, "last": 1}
        if pattern in want:
            assert ref["n_dev"] - c["n_dev"] == want[pattern] and ref["stored"] == 1000 + want[pattern]
        elif n >= 63:
            assert 0 < ref["n_dev"] - c["n_dev"] < n
        assert ref["n_dev"] - c["n_dev"] <= CAP  # a condition on the inputs (include/mxa_ddqn.h)


@pytest.mark.parametrize("n_dev0", [0, CAP - 1, CAP - 5, 3 * CAP + 17])
def test_gpu_period_ring_positions_two_calls_in_a_row(n_dev0):
    """a ring of 2200 positions entered at its start, its last row, 5 rows before its end and on
    its fourth lap; the second call continues where the first one's counts ended"""
    for n, pattern in ((2113, "half"), (2113, "all"), (65, "half")):
        c = U.make_case(n, 100 + n, pattern, cap=CAP, n_dev=n_dev0, stored=1000)
        ref = check(c, (n_dev0, n, pattern, "first call"))
        c2 = U.chain(c, ref, 200 + n)
        ref2 = check(c2, (n_dev0, n, pattern, "second call"))
        assert ref2["n_dev"] > ref["n_dev"] > n_dev0
        if pattern == "all":
            assert ref2["n_dev"] - n_dev0 > CAP  # the two calls wrapped, wherever they started


@pytest.mark.parametrize("n", [65, 2113])
def test_gpu_period_train_off_leaves_the_ring_alone(n):
    c = U.make_case(n, 31 + n, "half", cap=CAP, n_dev=CAP - 5, stored=1000, train=0)
    ref = check(c, (n, "train = 0"))
    for k in ("ring_s", "ring_s2", "ring_a", "ring_r"):
        assert U.same(ref[k], c[k]), k
    assert ref["n_dev"] == c["n_dev"] and ref["stored"] == c["stored"]
    on = U.reference(dict(c, train=1))
    assert on["n_dev"] > c["n_dev"]
    for k in ("alive_next", "live", "s2", "r_row", "env_steps"):
        assert U.same(np.asarray(ref[k]), np.asarray(on[k])), k


@pytest.mark.parametrize("obs_w,st_w,grids,nh,q0,q0_reward", [
    (2, 3, (7, 199), 27, 1e5, None), (13, 11, (199, 7), 27, 1e5, 777.0), (9, 8, (0, 1), 5, 1e5, 3.0),
    (13, 3, (1, 0), 5, 5000.0, None), (2, 11, (7, 7), 27, 12345.0, 1e5)])
def test_gpu_period_other_widths_grids_and_scalars(obs_w, st_w, grids, nh, q0, q0_reward):
    """row widths other than 9 / 8, two grids of different lengths (7 is the irregular grid with a
    repeated split point, so swapped g0 / g1 or n0 / n1 would show), nh = 5, other quantities, and
    an rscale that is not 1e4 / q0; env_steps starts from random counts in every case"""
    g = {7: U.IRREGULAR_G0, 199: U.DEFAULT_GRID[1], 0: np.zeros(0), 1: np.array([0.1])}
    c = U.make_case(1025, 500 + obs_w + st_w, "half", obs_w, st_w, cap=CAP, n_dev=3 * CAP + 17, g0=g[grids[0]],
                    g1=g[grids[1]], nh=nh, q0=q0, q0_reward=q0_reward)
    assert (c["n0"], c["n1"]) == grids and c["env_steps"].max() > 20
    ref = check(c, (obs_w, st_w, grids))
    for d in (0, 1):  # the inputs spread over the bins of each axis
        bins = len(set(ref["s2"][:, d].tolist()))  # the repeated split point leaves bin 2 of the irregular grid empty
        assert bins == {0: 1, 1: 2, 7: 7}[grids[d]] if grids[d] < 199 else bins > 7, (d, bins)


def _state_inputs():
    """[n, 2] (remaining time, remaining quantity): every quantity 0..100000 at three times; the
    five doubles nearest to each split point's pre-image on both axes; NaN, +-inf and values whose
    feature lies below -1 or above 1"""
    q0, nh = 1e5, 27.0
    q = np.arange(100001.0)
    rows = [np.stack([np.full_like(q, t), q], 1) for t in (0.0, 13.0, 27.0)]
    near = []
    for g, scale in ((U.DEFAULT_GRID[0], nh), (U.DEFAULT_GRID[1], q0)):
        x = (g + 1) / 2 * scale
        lo1, hi1 = np.nextafter(x, -np.inf), np.nextafter(x, np.inf)
        near.append(np.concatenate([np.nextafter(lo1, -np.inf), lo1, x, hi1, np.nextafter(hi1, np.inf)]))
    rows.append(np.stack(near, 1))
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, -5.0, -1e-300, -0.0, 1e300, 1e5 + 1, 27.5, 1e-300, 4e9])
    rows.append(np.stack([odd, odd[::-1]], 1))
    return np.concatenate(rows)


def _run_state(obs, g0, g1, nh, q0, what):
    o, a0, a1 = Guarded(obs), Guarded(g0), Guarded(g1)
    s = Guarded(np.full((len(obs), 2), -3.0, dtype=np.float32))
    rc = _lib().mxa_ddqn_state(torch.cuda.current_stream().cuda_stream, len(obs), obs.shape[1], o.ptr, a0.ptr, len(g0),
                               a1.ptr, len(g1), float(nh), float(q0), s.ptr)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    return s.read(what)


def test_gpu_state_every_quantity_and_split_point():
    """mxa_ddqn_state and ExecutionTask(device="cuda").state against np.digitize of the
    reference's true divisions. With the multiplication by 1 / quantity that a device tensor /
    Python scalar division takes, both landed one bin higher at 73 quantities (the multiples of 250
    from 50250 up that lie on a split point); the failure message counts them. Measured on an
    MI355X with the reciprocal form in the kernel: 375 of the 301,010 rows differ, at 156 distinct
    quantities (those 73 integers at each of the three times, and doubles next to split points);
    with the true divisions: none"""
    obs = _state_inputs()
    g0, g1 = U.DEFAULT_GRID
    ref = ddqn_ref.state_ref(obs, g0, g1, 27, 1e5).astype(np.float32)
    task = ddqn.ExecutionTask(device="cuda")
    for name, got in (("mxa_ddqn_state", _run_state(obs, g0, g1, 27, 1e5, "state")),
                      ("ExecutionTask.state", task.state(torch.from_numpy(obs).cuda()).cpu().numpy())):
        bad = np.flatnonzero((got != ref).any(1))
        print("%s: %d of %d rows differ from state_ref" % (name, len(bad), len(obs)))
        assert got.dtype == np.float32 and U.same(got, ref), \
            "%s: %d rows differ, %d distinct quantities, first %s" % (name, len(bad), len(set(obs[bad, 1].tolist())),
                                                                      obs[bad[:8]].tolist())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_gpu_state_and_actions_sizes_and_widths(n):
    """one block, its last lane, the first lane of the next, five blocks; rows of 2, 9 and 13
    doubles; the irregular grid on the time axis; actions 0..23 with obs[0] at 1.0, its two
    neighbours, NaN and 2 (the last step is obs[0] == 1.0 exactly)"""
    pool = _state_inputs()
    rs = np.random.RandomState(n)
    table = ddqn.ExecutionTask(device="cpu").table.numpy()
    for obs_w in (2, 9, 13):
        obs = rs.rand(n, obs_w) * 1000 - 500
        obs[:, :2] = pool[rs.randint(0, len(pool), n)]
        obs[:, 0] *= 5.0 / 27
        ref = ddqn_ref.state_ref(obs, U.IRREGULAR_G0, U.DEFAULT_GRID[1], 5, 1e5).astype(np.float32)
        got = _run_state(obs, U.IRREGULAR_G0, U.DEFAULT_GRID[1], 5, 1e5, ("state", n, obs_w))
        assert U.same(got, ref), (n, obs_w)
        task = U.make_task({"q0": 1e5, "nh": 5, "g0": U.IRREGULAR_G0, "g1": U.DEFAULT_GRID[1]}, "cuda")
        assert U.same(task.state(torch.from_numpy(obs).cuda()).cpu().numpy(), ref), (n, obs_w)

        obs[:, 0] = rs.permutation(np.resize([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nan, 2.0], n))
        obs[:, 1] = rs.randint(0, 100001, n)
        a = rs.permutation(np.resize(np.arange(24), n)).astype(np.int64)
        o, ad, tb = Guarded(obs), Guarded(a), Guarded(table)
        act = Guarded(np.full((n, 3), -3.0))
        rc = _lib().mxa_ddqn_actions(torch.cuda.current_stream().cuda_stream, n, obs_w, o.ptr, ad.ptr, tb.ptr, 1e5, act.ptr)
        assert rc == 0, rc
        torch.cuda.synchronize()
        want = ddqn_ref.actions_ref(obs, a, table, 1e5)
        assert U.same(act.read(("actions", n, obs_w)), want), (n, obs_w)
        dev = ddqn.ExecutionTask(device="cuda").actions(torch.from_numpy(a).cuda(), torch.from_numpy(obs).cuda())
        assert U.same(dev.cpu().numpy(), want), (n, obs_w)
        if n >= 255:
            last = obs[:, 0] == 1.0
            assert 0.15 * n < last.sum() < 0.25 * n and np.all(want[last, 1] == 1.0) and not np.all(want[~last, 1] == 1.0)
