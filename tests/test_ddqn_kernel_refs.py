"""The plain float64 references of the DDQN device kernels (oracle/ddqn_ref.py: state_ref,
actions_ref, period_ref, qnet_ref, integer_net) against this project's PyTorch ops on the CPU and
the reference's own discretize, all with exact equality, and the argument guards of
libmxa_ddqn.so (include/mxa_ddqn.h), which return before any HIP call. CPU only; the kernels
themselves are compared with the same references in tests/test_gpu_ddqn_kernels.py and
tests/test_gpu_qnet_fused.py."""
import numpy as np
import pytest
import torch

import ddqn_kernel_util as U
import ddqn_ref
from mxabides import ddqn

HIP_ERROR_INVALID_VALUE = 1


def test_state_ref_is_discretize_for_every_quantity_and_time():
    """all 100001 remaining quantities x 28 remaining times: state_ref, ExecutionTask.state on the
    CPU and the reference's discretize (np.digitize per feature) give the same bins; and the
    reciprocal form that a CUDA tensor / Python scalar division takes would not, at 73 quantities"""
    q0, nh = 100000.0, 27
    grid = U.DEFAULT_GRID
    q_bin = np.zeros(100001, dtype=np.int64)
    t_bin = np.zeros(28, dtype=np.int64)
    for q in range(100001):  # discretize zips the features with the grid axes: one bin per feature
        t = q % 28
        t_bin[t], q_bin[q] = ddqn.discretize([2 * (t / nh) - 1, 2 * (q / q0) - 1, 0.1, 0.2, 0.3, 0.4], grid)
    obs = np.zeros((28 * 100001, 2))
    obs[:, 0] = np.repeat(np.arange(28.0), 100001)
    obs[:, 1] = np.tile(np.arange(100001.0), 28)
    ref = ddqn_ref.state_ref(obs, grid[0], grid[1], nh, q0)
    assert np.array_equal(ref[:, 0], np.repeat(t_bin, 100001)) and np.array_equal(ref[:, 1], np.tile(q_bin, 28))
    got = ddqn.ExecutionTask(device="cpu").state(torch.from_numpy(obs)).numpy()
    assert got.dtype == np.float32 and U.same(got, ref.astype(np.float32))
    q = np.arange(100001.0)
    off = np.flatnonzero(np.digitize(2 * (q * (1.0 / q0)) - 1, grid[1]) != q_bin)
    assert len(off) == 73 and off[0] == 50250 and np.all(off % 250 == 0)
    assert np.array_equal(np.digitize(2 * (np.arange(28.0) * (1.0 / nh)) - 1, grid[0]), t_bin)


def test_state_ref_edges():
    """NaN and +inf go to len(bins), -inf to 0, a repeated split point is passed over, an empty
    grid gives 0, and values outside [-1, 1] land in the end bins; ExecutionTask.state agrees"""
    c = U.make_case(64, 1, g0=U.IRREGULAR_G0, g1=np.array([0.25]), nh=5, q0=1000.0)
    c["obs"][:6, 0] = [np.nan, np.inf, -np.inf, 0.625, 1.25, 2.5]  # 2x/5-1: -0.75, -0.5, 0.0
    c["obs"][:6, 1] = [np.nan, np.inf, -np.inf, -7.0, 625.0, 5000.0]
    ref = ddqn_ref.state_ref(c["obs"], c["g0"], c["g1"], c["nh"], c["q0"])
    assert ref[:6].tolist() == [[7, 1], [7, 1], [0, 0], [1, 0], [3, 1], [5, 1]]
    got = U.make_task(c, "cpu").state(torch.from_numpy(c["obs"])).numpy()
    assert U.same(got, ref.astype(np.float32))
    assert ddqn_ref.state_ref(c["obs"], np.zeros(0), np.array([0.0]), 5, 1000.0)[:, 0].tolist() == [0] * 64


def test_actions_ref_against_execution_task_on_the_cpu():
    """table rows, and on the last step (obs[0] == 1.0 exactly) the whole remaining quantity. The
    share x is obs[1] * (1 / q0) in actions_ref (the device's arithmetic) and obs[1] / q0 in the
    CPU's torch ops: an ulp apart at some quantities, the same rint(q0 * x) shares at every one"""
    assert ddqn_ref.rint_of_share_is_exact(100000.0, 100000)
    q = np.arange(100001.0)
    assert np.array_equal(np.rint(1e5 * (q / 1e5)), q)
    task = ddqn.ExecutionTask(device="cpu")
    rs = np.random.RandomState(2)
    n = 24 * 5 * 4
    obs = rs.rand(n, 9) * 100
    obs[:, 0] = np.tile(np.repeat([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nan, 2.0], 24), 4)
    obs[:, 1] = rs.randint(0, 100001, n)
    a = np.tile(np.arange(24), 20)
    table = task.table.numpy()
    ref = ddqn_ref.actions_ref(obs, a, table, task.q0)
    got = task.actions(torch.from_numpy(a), torch.from_numpy(obs)).numpy()
    last = obs[:, 0] == 1.0
    assert int(last.sum()) == 24 * 4
    assert U.same(got[~last], ref[~last]) and U.same(ref[~last], table[a[~last]])
    assert U.same(got[last, 1:], ref[last, 1:]) and np.all(ref[last, 1] == 1.0) and np.all(ref[last, 2] == 0.0)
    assert U.same(ref[last, 0], obs[last, 1] * (1.0 / task.q0)) and U.same(got[last, 0], obs[last, 1] / task.q0)
    assert np.array_equal(np.rint(task.q0 * ref[last, 0]), obs[last, 1])
    assert np.array_equal(np.rint(task.q0 * got[last, 0]), obs[last, 1])


@pytest.mark.parametrize("n,pattern,train", [(0, "all", 1), (1, "all", 1), (65, "half", 1), (300, "half", 0),
                                             (1025, "half", 1), (1025, "env1024", 1), (130, "none", 1)])
def test_period_ref_against_torch_ops_on_the_cpu(n, pattern, train):
    """period_ref against ExecutionTask.state / .reward, ReplayRing.add_device and alive.any() on
    the CPU: every output, exactly; three periods in a row on one ring of 1100 rows, which wraps"""
    c = U.make_case(n, 10 + n, pattern, obs_w=9, st_w=8, cap=1100, n_dev=1100 - 5, stored=1000, train=train)
    if n == 1025 and pattern == "half":  # the inputs cover what they are meant to
        al = c["alive"]
        assert sorted(set((c["flags"][al] & 7).tolist())) == list(range(8)) and (c["flags"] < 0).any()
        dq = c["st"][:, 2] - c["prev"][:, 2]
        assert (dq[al] > 0).any() and (dq[al] <= 0).any() and np.isnan(dq[al]).any() and np.isnan(dq[~al]).all()
        assert ((c["arrival"] == 0) & (dq > 0) & c["want_ok"]).any()
    for rep in range(3):
        ref = U.reference(c)
        got = U.torch_period(c, "cpu")
        U.assert_outputs_equal(got, ref, (n, pattern, rep), ring_rows=c["cap"])
        assert not np.isnan(ref["r_row"]).any() and np.all(ref["r_row"][~c["alive"]] == 0)
        if pattern == "half" and train and n >= 65:
            assert ref["n_dev"] > c["n_dev"] and ref["stored"] - c["stored"] == ref["n_dev"] - c["n_dev"]
            assert rep or n < 1025 or np.isinf(ref["ring_r"]).any()  # arrival 0 with dq > 0: inf stored
        if not train:
            assert ref["n_dev"] == c["n_dev"] and U.same(ref["ring_a"], c["ring_a"])
        assert U.same(ref["ring_a"][c["cap"]:], c["ring_a"][c["cap"]:])  # the spare row is not the reference's
        c = U.chain(c, ref, 1000 + rep)


def test_period_ref_other_shapes_and_scalars():
    """obs_w / st_w other than 9 / 8, grids of different lengths (and of 0 and 1 points), an
    irregular grid, nh = 5 and an rscale that is not 1e4 / q0: the torch ops agree on the CPU"""
    for k, (obs_w, st_w, g0, g1, nh, q0r) in enumerate([(2, 3, U.IRREGULAR_G0, None, 27, None),
                                                        (13, 11, None, U.IRREGULAR_G0, 5, 777.0),
                                                        (9, 8, np.zeros(0), np.array([0.1]), 27, 3.0)]):
        c = U.make_case(200, 50 + k, "half", obs_w, st_w, cap=333, n_dev=3 * 333 + 17, g0=g0, g1=g1, nh=nh,
                        q0_reward=q0r)
        assert c["n0"] != c["n1"]
        ref = U.reference(c)
        U.assert_outputs_equal(U.torch_period(c, "cpu"), ref, (obs_w, st_w), ring_rows=c["cap"])
        assert len(set(ref["s2"][:, 1].tolist())) > 1


def test_replay_ring_add_device_wraps_as_period_ref():
    """ReplayRing.add_device alone: 40 appends of 23 rows into 37 positions"""
    R = ddqn.ReplayRing(37, 2, "cpu")
    ring = {"ring_s": R.s.numpy().copy(), "ring_s2": R.s2.numpy().copy(), "ring_a": R.a.numpy().copy(),
            "ring_r": R.r.numpy().copy(), "n_dev": 0, "stored": 0}
    for it in range(40):
        c = U.make_case(23, 300 + it, "half", cap=37)
        c.update(ring)
        ref = U.reference(c)
        ok = torch.from_numpy(c["alive"] & ((c["flags"] & 2) != 0) & ((c["flags"] & 4) == 0))
        r = ddqn.ExecutionTask.reward(torch.from_numpy(c["prev"]), torch.from_numpy(c["st"]),
                                      torch.from_numpy(c["arrival"]), c["q0"])
        k = R.add_device(torch.from_numpy(c["s"]), torch.from_numpy(c["a"]), torch.from_numpy(ref["s2"]), r, ok)
        assert int(k) == ref["n_dev"] - c["n_dev"] and R.n == ref["n_dev"]
        for key, t in (("ring_s", R.s), ("ring_s2", R.s2), ("ring_a", R.a), ("ring_r", R.r)):
            assert U.same(t.numpy()[:37], ref[key][:37]), (it, key)
        ring = {key: ref[key] for key in ring}
    assert ring["n_dev"] > 5 * 37


@pytest.mark.parametrize("dims,nnz,seed", U.INTEGER_NETS)
def test_integer_nets_are_exact_in_float32(dims, nnz, seed):
    """the builder's own assertion (every sum of magnitudes below 2**24) holds for the five nets;
    a float32 forward in another summation order (numpy's matmul) gives qnet_ref's bits; no row of
    a multi-output net has a tie at its maximum"""
    layers, x, worst = ddqn_ref.integer_net(dims, 100, seed, nnz)
    print("net %s: worst sum of magnitudes %d" % (dims, worst))
    assert worst < 2 ** 24
    q = ddqn_ref.qnet_ref(layers, x)
    assert q.shape == (100, dims[-1]) and np.all(q == np.rint(q)) and np.abs(q).max() < 2 ** 24
    h = x.astype(np.float32)
    for i, (W, b) in enumerate(layers):
        h = h @ W.astype(np.float32) + b.astype(np.float32)
        if i + 1 < len(layers):
            h = np.maximum(h, np.float32(0))
    assert h.dtype == np.float32 and U.same(h, q.astype(np.float32))
    if dims[-1] > 1:
        top = np.sort(q, axis=1)
        assert np.all(top[:, -1] > top[:, -2])
        assert len(set(np.argmax(q, axis=1).tolist())) > 1
    flat = ddqn_ref.flat_params(layers)
    assert flat.dtype == np.float32 and len(flat) == sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    assert np.array_equal(flat[:dims[0]], layers[0][0][:, 0])  # weight[out][in] row-major: neuron 0's row first


def test_qnet_ref_nan_and_inf():
    layers = [(np.array([[1.0, -1.0], [2.0, 1.0]]), np.array([0.0, np.inf])), (np.array([[1.0], [1.0]]), np.array([1.0]))]
    q = ddqn_ref.qnet_ref(layers, np.array([[1.0, 1.0], [np.nan, 0.0], [-1.0, -1.0]]))
    assert np.isinf(q[0, 0]) and np.isnan(q[1, 0]) and np.isinf(q[2, 0])
    assert ddqn_ref.qnet_ref(layers[:1], np.array([[-1.0, -1.0]])).tolist() == [[-3.0, np.inf]]


def _period_guard(L, n=4, obs_w=9, st_w=8, train=1, cap=16):
    return L.mxa_ddqn_period(None, n, obs_w, st_w, train, *([None] * 13), None, 199, None, 199, 27.0, 1e5, 0.1, None, None,
                             None, None, cap, None, None)


def test_ddqn_library_guards_return_before_any_hip_call():
    """null pointers and no device: each refused call returns hipErrorInvalidValue"""
    L = ddqn.lib()
    assert L is not None, "libmxa_ddqn.so not built (build_lib.build_ddqn)"
    assert _period_guard(L, n=-1) == HIP_ERROR_INVALID_VALUE
    assert _period_guard(L, cap=0) == HIP_ERROR_INVALID_VALUE
    assert _period_guard(L, cap=-3) == HIP_ERROR_INVALID_VALUE
    assert _period_guard(L, obs_w=1) == HIP_ERROR_INVALID_VALUE
    assert _period_guard(L, st_w=2) == HIP_ERROR_INVALID_VALUE
    assert _period_guard(L, n=17, cap=16) == HIP_ERROR_INVALID_VALUE  # two rows on one ring position
    assert _period_guard(L, n=1 << 20, cap=(1 << 20) - 1) == HIP_ERROR_INVALID_VALUE
    for n, obs_w in ((-1, 9), (4, 1), (4, 0), (-1, 1)):
        assert L.mxa_ddqn_state(None, n, obs_w, None, None, 199, None, 199, 27.0, 1e5, None) == HIP_ERROR_INVALID_VALUE
        assert L.mxa_ddqn_actions(None, n, obs_w, None, None, None, 1e5, None) == HIP_ERROR_INVALID_VALUE
    assert L.mxa_ddqn_state(None, 0, 9, None, None, 199, None, 199, 27.0, 1e5, None) == 0
    assert L.mxa_ddqn_actions(None, 0, 2, None, None, None, 1e5, None) == 0
