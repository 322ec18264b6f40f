"""The closed-loop step kernel's policy on one wave (csrc/qnet_wave_device.h) through its probe
(include/mxa.h mxa_policy_probe): the forward, the argmax and the epsilon-greedy select against
libmxa_ddqn.so's tile kernel (mxa_qnet_forward / mxa_qnet_act, whose bits the per-step path carries)
and against oracle/ddqn_ref.py's plain float64 forward on nets whose fp32 chain is exact. Every
output is written between sentinel rows."""
import ctypes

import numpy as np
import pytest
import torch

import ddqn_kernel_util as U
import ddqn_ref
from mxabides import _lib, ddqn

pytestmark = pytest.mark.gpu
_CACHE = {}
# ddqn_kernel_util.INTEGER_NETS (widths 1, 4, 12, 63, 64, 65, 129, 255, 256; eight layers of 256)
# and a one-layer net
NETS = list(U.INTEGER_NETS) + [((256, 256), None, 3), ((2, 24), None, 3)]


def _probe(params_ptr, dims, x, what, test=1, enough=0, u=None, rnd=None, eps=None, want_q=True, want_a=True):
    """mxa_policy_probe on x (numpy [n, dims[0]]): (q, a), each read back from between sentinel rows"""
    n = len(x)
    xg = U.Guarded(np.asarray(x, dtype=np.float32))
    ug = None if u is None else U.Guarded(np.asarray(u, dtype=np.float64))
    rg = None if rnd is None else U.Guarded(np.asarray(rnd, dtype=np.int64))
    eg = None if eps is None else U.Guarded(np.array([eps], dtype=np.float64))
    q = U.Guarded(np.full((n, dims[-1]), -3.0, dtype=np.float32)) if want_q else None
    a = U.Guarded(np.full(n, -3, dtype=np.int64)) if want_a else None
    ptr = lambda g: None if g is None else g.ptr
    d = (ctypes.c_int32 * len(dims))(*dims)
    rc = _lib.load().mxa_policy_probe(torch.cuda.current_stream().cuda_stream, n, xg.ptr, params_ptr, len(dims) - 1, d,
                                      int(test), int(enough), ptr(ug), ptr(rg), ptr(eg), ptr(q), ptr(a))
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    return (None if q is None else q.read((what, "q"))), (None if a is None else a.read((what, "a")))


@pytest.mark.parametrize("model", ["NNModel_1", "NNModel_2"])
def test_gpu_policy_forward_every_grid_state(model):
    """all 200 x 200 states on the learner's glorot weights: q has mxa_qnet_forward's bits and the
    test-mode action is mxa_qnet_act's"""
    L = ddqn.DDQNLearner(device="cuda", seed=5, model=model, fused_act=True, mode="test")
    g = torch.arange(200, dtype=torch.float32, device="cuda")
    x = torch.cartesian_prod(g, g).contiguous()
    want_q, want_a = L.q_values(x), L.choose_action(x)
    torch.cuda.synchronize()
    q, a = _probe(L.eflat.data_ptr(), list(L._qdims), x.cpu().numpy(), model)
    assert q.shape == (40000, 24)
    assert U.same(q, want_q.cpu().numpy()), int((q != want_q.cpu().numpy()).sum())
    assert U.same(a, want_a.cpu().numpy())
    assert len(set(a.tolist())) > 1  # a condition on the inputs: the greedy action varies over the grid


def _integer_net(dims, nnz, seed):
    key = ("int", dims)
    if key not in _CACHE:
        layers, x, _ = ddqn_ref.integer_net(dims, 100, seed, nnz)
        flat = torch.from_numpy(ddqn_ref.flat_params(layers)).cuda()
        shifted = torch.cat([torch.zeros(1, device="cuda"), flat])[1:]
        assert flat.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        _CACHE[key] = (x, ddqn_ref.qnet_ref(layers, x).astype(np.float32), flat, shifted)
    return _CACHE[key]


@pytest.mark.parametrize("dims,nnz,seed", NETS)
def test_gpu_policy_forward_integer_nets_bit_for_bit(dims, nnz, seed):
    """q equals the float64 reference's bits: widths that are no multiple of 4 or of the 64 lanes, one
    layer and eight layers of 256; one row, a wave less one, a wave, a wave and one, 100; the
    parameters on a 16-byte boundary (the 16-byte loads where in % 4 == 0) and 4 bytes past it (the
    one-float loads for every layer). The action is np.argmax of the reference"""
    x, ref, flat, shifted = _integer_net(dims, nnz, seed)
    for n in (1, 63, 64, 65, 100):
        for name, p in (("aligned", flat), ("shifted", shifted)):
            q, a = _probe(p.data_ptr(), list(dims), x[:n], (dims, n, name))
            assert U.same(q, ref[:n]), (dims, n, name, int((q != ref[:n]).sum()))
            assert U.same(a, np.argmax(ref[:n], axis=1).astype(np.int64)), (dims, n, name)
    q, none = _probe(flat.data_ptr(), list(dims), x[:5], (dims, "q only"), want_a=False)
    assert none is None and U.same(q, ref[:5])
    none, a = _probe(flat.data_ptr(), list(dims), x[:5], (dims, "a only"), want_q=False)
    assert none is None and U.same(a, np.argmax(ref[:5], axis=1).astype(np.int64))


@pytest.mark.parametrize("dims", [(2, 6), (2, 4, 6), (2, 4, 70)])
def test_gpu_policy_argmax_crafted_maxima(dims):
    """the argmax's branches: an exact tie (the lower index wins), NaN (the first NaN wins, as
    np.argmax and torch.argmax), +inf, all -inf, and a NaN input row (action 0; the NaN passes
    through the ReLU); with 70 outputs the maxima sit in the second register (index 64 and up)"""
    n_out = dims[-1]
    hi = n_out - 6  # the crafted columns are the last six: past lane 63 when n_out = 70
    rs = np.random.RandomState(len(dims))
    x = rs.randint(-4, 5, (20, 2)).astype(np.float64)
    hidden = [(rs.choice([-2.0, -1.0, 1.0, 2.0], (dims[i], dims[i + 1])), np.full(dims[i + 1], 10.0))
              for i in range(len(dims) - 2)]
    W = rs.choice([-2.0, -1.0, 1.0, 2.0], (dims[-2], n_out))
    W[:, hi + 3] = W[:, hi + 1]
    low = np.full(hi, -9000.0)
    b = np.concatenate([low, [-5000.0, 7.0, -4000.0, 7.0, -3000.0, -2000.0]])
    nan_x = x.copy()
    nan_x[3] = [np.nan, 1.0]
    tail = lambda *v: np.concatenate([low, v])
    cases = {"tie": (b, x, hi + 1), "nan": (tail(0.0, 1.0, np.nan, 2.0, np.nan, 3.0), x, hi + 2),
             "inf": (tail(0.0, np.inf, 1.0, 2.0, 3.0, 4.0), x, hi + 1), "all -inf": (np.full(n_out, -np.inf), x, 0),
             "nan row": (b, nan_x, None)}
    for name, (bias, xs, pick) in cases.items():
        layers = hidden + [(W, bias)]
        ref = ddqn_ref.qnet_ref(layers, xs)
        want = np.argmax(ref, axis=1)
        if name == "tie":
            assert np.all(ref[:, hi + 1] == ref[:, hi + 3]) and np.all(ref[:, hi + 1] == ref.max(1))
        if name == "nan row":
            assert np.isnan(ref[3]).all() and want[3] == 0 and not np.isnan(np.delete(ref, 3, 0)).any()
            assert np.all(np.delete(want, 3) == hi + 1)
        else:
            assert np.all(want == pick), (name, want)
        flat = torch.from_numpy(ddqn_ref.flat_params(layers)).cuda()
        q, a = _probe(flat.data_ptr(), list(dims), xs, (dims, name))
        assert np.array_equal(q, ref.astype(np.float32), equal_nan=True), (dims, name)
        assert np.array_equal(np.isnan(q), np.isnan(ref)) and U.same(a, want.astype(np.int64)), (dims, name, a)


def test_gpu_policy_select_edges():
    """exploit exactly where u < eps and enough: u just below, at and just above eps = 0.5, 0 and
    the largest double below 1; test mode with null u, rnd and eps is all greedy"""
    dims, nnz, seed = U.INTEGER_NETS[0]
    x, ref, flat, _ = _integer_net(dims, nnz, seed)
    n = 40
    greedy = np.argmax(ref[:n], axis=1)
    rnd = (greedy + 1 + np.arange(n) % 22) % 24  # never the greedy action
    u = np.resize([np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 0.0, 1 - 2.0 ** -53], n)
    assert u[4] < 1.0 and (rnd != greedy).all()
    for enough in (0, 1):
        q, a = _probe(flat.data_ptr(), list(dims), x[:n], ("select", enough), 0, enough, u, rnd, 0.5)
        exploit = (u < 0.5) & bool(enough)
        assert exploit.sum() == (16 if enough else 0)
        assert U.same(a, np.where(exploit, greedy, rnd).astype(np.int64)), enough
        assert U.same(q, ref[:n])
        _, a = _probe(flat.data_ptr(), list(dims), x[:n], ("test mode", enough), 1, enough)
        assert U.same(a, greedy.astype(np.int64))


def test_gpu_policy_probe_refuses_bad_arguments():
    dims, nnz, seed = U.INTEGER_NETS[0]
    x, _, flat, _ = _integer_net(dims, nnz, seed)
    L = _lib.load()
    xg = torch.from_numpy(x[:4].astype(np.float32)).cuda()
    q = torch.full((4, 24), -3.0, dtype=torch.float32, device="cuda")
    a = torch.full((4,), -3, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def rc(n=4, xp=xg.data_ptr(), pp=flat.data_ptr(), d=dims, test=1, qp=q.data_ptr(), ap=a.data_ptr()):
        arr = None if d is None else (ctypes.c_int32 * len(d))(*d)
        return L.mxa_policy_probe(st, n, xp, pp, 0 if d is None else len(d) - 1, arr, test, 1, None, None, None, qp, ap)

    assert rc() == 0
    for bad in (dict(n=0), dict(xp=None), dict(pp=None), dict(d=(256, 257, 24)), dict(d=(256, 0, 24)), dict(d=(256,)),
                dict(d=(2,) * 10), dict(d=None), dict(test=0), dict(qp=None, ap=None)):
        assert rc(**bad) == -1, bad  # MXA_EINVAL
    torch.cuda.synchronize()
