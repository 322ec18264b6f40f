"""include/mxa_ddqn.h mxa_qnet_* on the GPU: the hand-written Q-network forward and epsilon-greedy action
kernel (libmxa_ddqn.so, DDQNLearner(fused_act=True)) against an fp64 forward of the same weights,
over the whole 200 x 200 state space, and the learner paths built on it; then the kernel's edges
(odd widths, both staging paths, all of its LDS, every output of mxa_qnet_act, the select's and
the argmax's branches) with exact equality against oracle/ddqn_ref.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import ddqn_kernel_util as U
import ddqn_ref
from mxabides import ddqn

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-3   # test_gpu_qnet_matches_host's tolerance for the fp32 device net
TILE = 16                 # envs per workgroup (csrc/ddqn_qnet.hip kTile)
SEEDS = [123456789, 2024, 7, 123, 99991, 31337, 4242, 555, 1, 2, 3, 4, 5, 6, 8, 9]  # test_gpu_ddqn's
_CACHE = {}


def _states():
    g = torch.arange(200, dtype=torch.float32, device="cuda")
    return torch.cartesian_prod(g, g).contiguous()  # [40000, 2]


def _f64(net, x):
    net64 = copy.deepcopy(net).double().eval()
    with torch.no_grad():
        return net64(x.double())


def _ref(model):
    """per model, computed once and left unchanged: the seed-5 learner (test mode: greedy), the
    40,000 grid states, the fp64 reference, torch's fp32 forward and the kernel's q and actions"""
    if model not in _CACHE:
        L = ddqn.DDQNLearner(device="cuda", seed=5, model=model, fused_act=True, mode="test")
        x = _states()
        q64 = _f64(L.eval_model, x)
        L.eval_model.eval()
        with torch.no_grad():
            q32 = L.eval_model(x)
        q = L.q_values(x)
        a = L.choose_action(x)
        torch.cuda.synchronize()
        _CACHE[model] = (L, x, q64, q32, q, a)
    return _CACHE[model]


def _forward_raw(flat, dims, x, q_ptr, stream=None):
    d = (ctypes.c_int * len(dims))(*dims)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = ddqn.lib().mxa_qnet_forward(st, x.shape[0], x.data_ptr(), flat.data_ptr(), len(dims) - 1, d, q_ptr)
    assert rc == 0, rc


@pytest.mark.parametrize("model", ["NNModel_1", "NNModel_2"])
def test_gpu_qnet_q_values_whole_state_space(model):
    """measured on an MI355X, max |q - q64| over the 40,000 states: NNModel_1 fused 7.4e-6, torch's
    fp32 forward 8.3e-6 (max |q64| 14.8); NNModel_2 fused 5.9e-6, torch 6.6e-6 (max |q64| 9.0)"""
    L, x, q64, q32, q, _ = _ref(model)
    assert q.shape == (40000, 24) and q.dtype == torch.float32
    err_fused = (q.double() - q64).abs().max().item()
    err_torch = (q32.double() - q64).abs().max().item()
    print("%s: max |q - q64| fused %.3e, torch fp32 %.3e, max |q64| %.3f" % (model, err_fused, err_torch,
                                                                            q64.abs().max().item()))
    torch.testing.assert_close(q.double(), q64, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("model", ["NNModel_1", "NNModel_2"])
def test_gpu_qnet_greedy_action_every_row(model):
    L, x, q64, _, q, a = _ref(model)
    top2 = torch.topk(q64, 2, dim=1).values
    close = (top2[:, 0] - top2[:, 1]) < 1e-2
    print("%s: %d rows with an fp64 top-two gap below 1e-2" % (model, int(close.sum())))
    assert int(close.sum()) <= 0.02 * len(x)  # a condition on the inputs
    assert a.dtype == torch.int64 and a.shape == (len(x),)
    assert int(a.min()) >= 0 and int(a.max()) < 24
    picked = q64.gather(1, a[:, None])[:, 0]
    assert bool((picked >= top2[:, 0] - 2 * ATOL).all())  # every row, no exclusions
    assert torch.equal(a[~close], torch.argmax(q64, dim=1)[~close])
    assert torch.equal(a, torch.argmax(q, dim=1))  # the kernel's argmax of its own q


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4097])
def test_gpu_qnet_batch_invariance_and_guards(n):
    L, x, _, _, q, _ = _ref("NNModel_1")
    dims = list(L._qdims)
    side = torch.cuda.Stream()
    for off, stream in ((0, None), (7, None), (20001, side)):
        xs = x[off:off + n].clone()
        buf = torch.full((n + 4, 24), 12345.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _forward_raw(L.eflat, dims, xs, buf[2:].data_ptr(), None if stream is None else stream.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(buf[2:n + 2], q[off:off + n]), (n, off)
        assert bool((buf[:2] == 12345.0).all()) and bool((buf[n + 2:] == 12345.0).all()), (n, off)


def test_gpu_qnet_generic_shapes():
    gen = torch.Generator().manual_seed(11)
    dims = (3, 5, 256, 1, 7)
    lins = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    with torch.no_grad():
        for lin in lins:
            lin.weight.uniform_(-1, 1, generator=gen)
            lin.bias.uniform_(-1, 1, generator=gen)
    flat = torch.cat([p.detach().reshape(-1) for lin in lins for p in (lin.weight, lin.bias)]).cuda()
    x = (torch.rand((777, 3), generator=gen) * 4 - 2).cuda()
    h = x.double()
    for i, lin in enumerate(lins):
        h = h @ lin.weight.detach().double().cuda().T + lin.bias.detach().double().cuda()
        if i + 1 < len(lins):
            h = torch.relu(h)
    q = torch.empty((777, 7), dtype=torch.float32, device="cuda")
    _forward_raw(flat, dims, x, q.data_ptr())
    # the same parameters one float further on: no 16-byte alignment, the plain staging path
    shifted = torch.cat([torch.zeros(1, device="cuda"), flat])[1:]
    assert shifted.data_ptr() % 16 != 0
    q2 = torch.empty_like(q)
    _forward_raw(shifted, dims, x, q2.data_ptr())
    torch.cuda.synchronize()
    print("dims %s: max |q - q64| %.3e" % (dims, (q.double() - h).abs().max().item()))
    torch.testing.assert_close(q.double(), h, rtol=RTOL, atol=ATOL)
    assert torch.equal(q, q2)

    L = ddqn.DDQNLearner(device="cuda", seed=5, n_actions=5, fused_act=True)
    s = _states()[::7].contiguous()
    q5 = L.q_values(s)
    assert q5.shape == (len(s), 5)
    torch.testing.assert_close(q5.double(), _f64(L.eval_model, s), rtol=RTOL, atol=ATOL)
    # NNModel_1's own parameters, unaligned: same bits as the 16-byte staging path
    L2 = ddqn.DDQNLearner(device="cuda", seed=5, fused_act=True)
    sh = torch.cat([torch.zeros(1, device="cuda"), L2.eflat])[1:]
    out = torch.empty((len(s), 24), dtype=torch.float32, device="cuda")
    _forward_raw(sh, list(L2._qdims), s, out.data_ptr())
    assert torch.equal(out, L2.q_values(s))


def _clone_gen(g):
    c = torch.Generator(device="cuda")
    c.set_state(g.get_state())
    return c


def _fill(L, seed):
    rs = np.random.RandomState(seed)
    n = 64
    dv = lambda v: torch.from_numpy(v).to("cuda", torch.float32)
    L.memory.add(dv(rs.randint(0, 200, (n, 2)).astype(np.float64)), torch.from_numpy(rs.randint(0, 24, n)).cuda(),
                 dv(rs.randint(0, 200, (n, 2)).astype(np.float64)), dv(rs.normal(0, 50, n)),
                 torch.ones(n, dtype=torch.bool, device="cuda"))


def test_gpu_qnet_epsilon_greedy_matches_unfused():
    s = _states()[torch.randperm(40000, generator=torch.Generator().manual_seed(2))[:4096].cuda()].contiguous()
    Ls = {}
    for fused in (False, True):
        L = ddqn.DDQNLearner(device="cuda", seed=9, epsilon_increment=0.5, fused_act=fused)
        _fill(L, 1)
        assert L.learn() is not None
        assert L.epsilon == 0.5
        Ls[fused] = L
    g = _clone_gen(Ls[True].gen)
    u = torch.rand(4096, generator=g, device="cuda", dtype=torch.float64)
    rnd = torch.randint(0, 24, (4096,), generator=g, device="cuda")
    greedy = {f: torch.argmax(Ls[f].q_values(s), dim=1) for f in Ls}
    a = {f: Ls[f].choose_action(s) for f in Ls}
    torch.cuda.synchronize()
    explore = ~(u < 0.5)
    assert 1500 < int(explore.sum()) < 2600
    assert torch.equal(a[True], torch.where(explore, rnd, greedy[True]))
    # the two learners' weights differ in the last bits after the update (another summation order
    # in q_target's forwards), so a near-tie may fall the other way: compared where they agree,
    # and on every exploring row
    agree = greedy[True] == greedy[False]
    print("greedy actions agree on %d of 4096 rows" % int(agree.sum()))
    assert torch.equal(a[True][agree | explore], a[False][agree | explore])
    assert torch.equal(Ls[True].gen.get_state(), Ls[False].gen.get_state())

    # not enough experience: every action is the random one
    L = ddqn.DDQNLearner(device="cuda", seed=9, fused_act=True)
    g = _clone_gen(L.gen)
    torch.rand(4096, generator=g, device="cuda", dtype=torch.float64)
    rnd = torch.randint(0, 24, (4096,), generator=g, device="cuda")
    assert torch.equal(L.choose_action(s), rnd)
    # test mode: every action is greedy, and the exploration stream is not drawn from
    L = ddqn.DDQNLearner(device="cuda", seed=9, fused_act=True, mode="test")
    st = L.gen.get_state()
    assert torch.equal(L.choose_action(s), torch.argmax(L.q_values(s), dim=1))
    assert torch.equal(L.gen.get_state(), st)


def test_gpu_qnet_act_vectors_equal_execution_task():
    from mxabides.gym import OBS_SIZE
    task = ddqn.ExecutionTask(device="cuda")
    n = 1000
    gen = torch.Generator().manual_seed(6)
    obs = torch.rand((n, OBS_SIZE), generator=gen, dtype=torch.float64) * 1000
    obs[:, 0] = torch.randint(1, 4, (n,), generator=gen).double()  # a third of the rows on the last step
    obs[:, 1] = torch.randint(0, 100001, (n,), generator=gen).double()
    obs = obs.cuda()
    s = task.state(obs)
    for mode in ("train", "test"):
        L = ddqn.DDQNLearner(device="cuda", seed=5, fused_act=True, mode=mode)
        a, act = L.act(s, obs, task)
        torch.cuda.synchronize()
        assert 200 < int((obs[:, 0] == 1).sum()) < 500
        assert a.dtype == torch.int64 and act.dtype == torch.float64 and act.shape == (n, 3)
        assert torch.equal(act, task.actions(a, obs)), mode
        if mode == "test":
            assert torch.equal(a, torch.argmax(L.q_values(s), dim=1))
        else:
            assert len(set(a.tolist())) == 24  # no experience yet: the random actions


def _layers(net):
    return [(lin.weight.detach().cpu().numpy().T.astype(np.float64), lin.bias.detach().cpu().numpy().astype(np.float64))
            for lin in list(net.hidden) + [net.logits]]


def _batch(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 200, (n, 2)).astype(np.float64), rs.randint(0, 24, n), rs.randint(0, 200, (n, 2)).astype(np.float64),
            rs.normal(0, 50, n))


def test_gpu_qnet_q_target_matches_numpy_reference():
    import ddqn_ref
    L = ddqn.DDQNLearner(device="cuda", dropout=0.0, seed=3, batch_size=32, fused_act=True)
    dv = lambda v: torch.from_numpy(v).to("cuda", torch.float32)
    for it in range(6):
        s, a, s2, r = _batch(32, 100 + it)
        L.learn_on(dv(s), torch.from_numpy(a).cuda(), dv(s2), dv(r))
    assert L.learn_step_counter == 6
    s, a, s2, r = _batch(32, 200)
    got = L.q_target(dv(s), torch.from_numpy(a).cuda(), dv(s2), dv(r)).cpu().double().numpy()
    ref = ddqn_ref.q_target(_layers(L.eval_model), _layers(L.target_model), s, a, s2, r, L.reward_decay)
    print("q_target: max |fused - fp64| %.3e, max |ref| %.3f" % (np.abs(got - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-4)


def test_gpu_qnet_fused_episode_matches_oracle_replay():
    import pyoracle
    from mxabides.gym import VecABIDESEnv
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    base = SEEDS * 4  # 64 envs
    v = VecABIDESEnv(seeds=base)
    v.set_stream(stream.cuda_stream)
    learner = ddqn.DDQNLearner(device="cuda", seed=1, batch_size=32, fused_act=True)
    task = ddqn.ExecutionTask(device="cuda")
    oras = [None] * len(base)
    for ep in range(2):
        seeds = [s + 1000 * ep for s in base]
        rec = []
        res = ddqn.run_episode(v, learner, task, seeds=seeds, record=rec, fused=True)
        torch.cuda.synchronize()
        acts = torch.stack(rec).cpu().numpy()
        summ = v.summary()
        for e, seed in enumerate(seeds):
            if oras[e] is None:
                oras[e] = pyoracle.OracleGymEnv(seed=seed)
            else:
                oras[e].reset(seed=seed)
            o = oras[e]
            for i in range(len(acts)):
                _, done, rc = o.step(acts[i, e])
                if done or rc:
                    break
            assert summ["events"][e] == o.events and summ["hash"][e] == o.hash, (ep, e)
        assert res["stored"] > 0
        assert int(res["actions"].min()) >= 0 and int(res["actions"].max()) < 24
    assert learner.learn_step_counter > 0
    cost = learner.cost_hist
    assert cost and all(np.isfinite(float(c)) for c in cost)


# ---- the kernel's edges, through ctypes, against oracle/ddqn_ref.py's plain float64 forward with
# exact equality: nets whose fp32 fmaf chain is exact (ddqn_ref.integer_net), so any slip in the
# staging (16-byte and plain), the pass and tile bounds or the LDS strides shows as wrong bits

def _cdims(dims):
    return (ctypes.c_int * len(dims))(*dims)


def _fwd(flat, dims, x, what):
    """mxa_qnet_forward on x (numpy), q behind sentinels"""
    xg = U.Guarded(x.astype(np.float32))
    q = U.Guarded(np.full((len(x), dims[-1]), -3.0, dtype=np.float32))
    rc = ddqn.lib().mxa_qnet_forward(torch.cuda.current_stream().cuda_stream, len(x), xg.ptr, flat.data_ptr(),
                                          len(dims) - 1, _cdims(dims), q.ptr)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    return q.read(what)


def _act(flat, dims, x, test, enough, u, rnd, eps, obs, table, q0, what):
    """mxa_qnet_act with q, a (and, with obs, act) all requested, each behind sentinels"""
    n = len(x)
    xg = U.Guarded(x.astype(np.float32))
    ug = None if u is None else U.Guarded(np.asarray(u, dtype=np.float64))
    rg = None if rnd is None else U.Guarded(np.asarray(rnd, dtype=np.int64))
    eg = U.Guarded(np.array([eps], dtype=np.float64))
    og = None if obs is None else U.Guarded(obs)
    tg = None if obs is None else U.Guarded(table)
    q = U.Guarded(np.full((n, dims[-1]), -3.0, dtype=np.float32))
    a = U.Guarded(np.full(n, -3, dtype=np.int64))
    act = None if obs is None else U.Guarded(np.full((n, 3), -3.0))
    ptr = lambda g: None if g is None else g.ptr
    rc = ddqn.lib().mxa_qnet_act(torch.cuda.current_stream().cuda_stream, n, xg.ptr, flat.data_ptr(), len(dims) - 1,
                                      _cdims(dims), int(test), int(enough), ptr(ug), ptr(rg), eg.ptr,
                                      2 if obs is None else obs.shape[1], ptr(og), ptr(tg), q0, a.ptr, ptr(act), q.ptr)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    return a.read((what, "a")), None if act is None else act.read((what, "act")), q.read((what, "q"))


def _integer_net(dims, nnz, seed):
    key = ("int", dims)
    if key not in _CACHE:
        layers, x, _ = ddqn_ref.integer_net(dims, 100, seed, nnz)
        flat = torch.from_numpy(ddqn_ref.flat_params(layers)).cuda()
        shifted = torch.cat([torch.zeros(1, device="cuda"), flat])[1:]
        assert flat.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 != 0
        _CACHE[key] = (x, ddqn_ref.qnet_ref(layers, x).astype(np.float32), flat, shifted)
    return _CACHE[key]


@pytest.mark.parametrize("dims,nnz,seed", U.INTEGER_NETS)
def test_gpu_qnet_integer_nets_bit_for_bit(dims, nnz, seed):
    """widths that are no multiple of 4 (255, 65, 129, 63, 1) or of the 64-neuron pass, the weight
    strides of in = 4 and in = 12, a three-trip plain staging loop (in = 129, 255), 8 layers of 256
    (all of the 100,864 B of LDS); one env, a tile less one, a tile, a tile and one, two tiles and
    one, six tiles and four. The same bits from the parameters one float further on (no 16-byte
    alignment: the plain staging path for every layer)"""
    x, ref, flat, shifted = _integer_net(dims, nnz, seed)
    for n in (1, 15, 16, 17, 33, 100):
        for name, p in (("aligned", flat), ("shifted", shifted)):
            q = _fwd(p, dims, x[:n], (dims, n, name))
            assert U.same(q, ref[:n]), (dims, n, name, int((q != ref[:n]).sum()))


@pytest.mark.parametrize("dims,nnz,seed", U.INTEGER_NETS)
def test_gpu_qnet_act_q_a_and_act_behind_sentinels(dims, nnz, seed):
    """mxa_qnet_act with all three outputs: q has mxa_qnet_forward's (and so the reference's)
    bits, a is np.argmax of it where the env exploits and rnd elsewhere, act is actions_ref of a
    (rows of 2, 9 and 13 doubles, a fifth of them on the last step)"""
    x, ref, flat, _ = _integer_net(dims, nnz, seed)
    n_out = dims[-1]
    rs = np.random.RandomState(n_out)
    table = rs.rand(n_out, 3)
    for n, obs_w in ((1, 2), (17, 9), (100, 13), (33, 2)):
        u = rs.rand(n)
        rnd = rs.randint(0, n_out, n)
        obs = rs.rand(n, obs_w) * 100
        obs[:, 0] = np.resize([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nan, 2.0], n)
        obs[:, 1] = rs.randint(0, 100001, n)
        a, act, q = _act(flat, dims, x[:n], 0, 1, u, rnd, 0.5, obs, table, 1e5, (dims, n))
        assert U.same(q, ref[:n]) and U.same(q, _fwd(flat, dims, x[:n], (dims, n)))
        want = np.where(u < 0.5, np.argmax(ref[:n], axis=1), rnd)
        assert U.same(a, want.astype(np.int64)), (dims, n)
        assert U.same(act, ddqn_ref.actions_ref(obs, want, table, 1e5)), (dims, n)
        a2, none, q2 = _act(flat, dims, x[:n], 0, 1, u, rnd, 0.5, None, None, 1.0, (dims, n, "no act"))
        assert none is None and U.same(a2, a) and U.same(q2, q)


def test_gpu_qnet_epsilon_greedy_select_edges():
    """exploit exactly where u < eps and enough: u just below, at and just above eps = 0.5, 0
    and the largest double below 1; test mode with null u and rnd is all greedy"""
    dims, nnz, seed = U.INTEGER_NETS[0]
    x, ref, flat, _ = _integer_net(dims, nnz, seed)
    n = 40
    greedy = np.argmax(ref[:n], axis=1)
    rnd = (greedy + 1 + np.arange(n) % 22) % 24  # never the greedy action
    u = np.resize([np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 0.0, 1 - 2.0 ** -53], n)
    assert u[4] < 1.0 and (rnd != greedy).all()
    for enough in (0, 1):
        a, _, q = _act(flat, dims, x[:n], 0, enough, u, rnd, 0.5, None, None, 1.0, ("select", enough))
        exploit = (u < 0.5) & bool(enough)
        assert exploit.sum() == (16 if enough else 0)
        assert U.same(a, np.where(exploit, greedy, rnd).astype(np.int64)), enough
        assert U.same(q, ref[:n])
    for enough in (0, 1):
        a, _, _ = _act(flat, dims, x[:n], 1, enough, None, None, 0.5, None, None, 1.0, ("test mode", enough))
        assert U.same(a, greedy.astype(np.int64))


@pytest.mark.parametrize("dims", [(2, 6), (2, 4, 6)])
def test_gpu_qnet_crafted_maxima(dims):
    """the argmax's branches: an exact tie (the lower index wins), NaN (the first NaN wins, as
    np.argmax and torch.argmax), +inf, all -inf, and a NaN input row (action 0; the NaN passes
    through the ReLU). The expected action is np.argmax of the float64 reference"""
    rs = np.random.RandomState(len(dims))
    x = rs.randint(-4, 5, (20, 2)).astype(np.float64)
    hidden = [(rs.choice([-2.0, -1.0, 1.0, 2.0], (dims[i], dims[i + 1])), np.full(dims[i + 1], 10.0))
              for i in range(len(dims) - 2)]
    W = rs.choice([-2.0, -1.0, 1.0, 2.0], (dims[-2], 6))
    W[:, 3] = W[:, 1]
    b = np.array([-5000.0, 7.0, -4000.0, 7.0, -3000.0, -2000.0])
    nan_x = x.copy()
    nan_x[3] = [np.nan, 1.0]
    cases = {"tie": (b, x, 1), "nan": (np.array([0.0, 1.0, np.nan, 2.0, np.nan, 3.0]), x, 2),
             "inf": (np.array([0.0, np.inf, 1.0, 2.0, 3.0, 4.0]), x, 1), "all -inf": (np.full(6, -np.inf), x, 0),
             "nan row": (b, nan_x, None)}
    for name, (bias, xs, pick) in cases.items():
        layers = hidden + [(W, bias)]
        ref = ddqn_ref.qnet_ref(layers, xs)
        want = np.argmax(ref, axis=1)
        if name == "tie":
            assert np.all(ref[:, 1] == ref[:, 3]) and np.all(ref[:, 1] == ref.max(1))
        if name == "nan row":
            assert np.isnan(ref[3]).all() and want[3] == 0 and not np.isnan(np.delete(ref, 3, 0)).any()
            assert np.all(np.delete(want, 3) == 1)
        else:
            assert np.all(want == pick), (name, want)
        flat = torch.from_numpy(ddqn_ref.flat_params(layers)).cuda()
        a, _, q = _act(flat, dims, xs, 1, 0, None, None, 0.5, None, None, 1.0, (dims, name))
        assert np.array_equal(q, ref.astype(np.float32), equal_nan=True), (dims, name)
        assert np.array_equal(np.isnan(q), np.isnan(ref)) and U.same(a, want.astype(np.int64)), (dims, name, a)
