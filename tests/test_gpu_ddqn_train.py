"""include/mxa_ddqn_train.h on the GPU: the hand-written DDQN update (mxa_qnet_grad, mxa_qnet_update,
mxa_qnet_train; libmxa_ddqn.so, DDQNLearner(fused_learn=True)). Bit for bit against the float64
reference of oracle/ddqn_ref.py on nets and batches whose update is exact in fp32
(tests/ddqn_train_ref.exact_case) and against an unfused learner holding the same nets; the update's
edges against numpy float32 and learn_on's torch expressions; real nets against the float64
gradient with the autograd path's own error as the yardstick; then through the learner and one
episode. Every output of the raw calls sits behind sentinels."""
import ctypes

import numpy as np
import pytest
import torch

import ddqn_kernel_util as U
import ddqn_ref
import ddqn_train_ref as T
from mxabides import ddqn

pytestmark = pytest.mark.gpu
LR, RHO, RMS_EPS, ITER, EPS_MAX = 0.01, 0.9, 1e-7, 5, 0.9
SEEDS = [123456789, 2024, 7, 123, 99991, 31337, 4242, 555, 1, 2, 3, 4, 5, 6, 8, 9]  # test_gpu_ddqn's
_CACHE = {}


class Flat(U.Guarded):
    """a 1-D device buffer with `lead` sentinel elements before it and PAD after: lead 4 puts a
    float32 buffer on a 16-byte boundary, lead 5 one float past it"""

    def __init__(self, arr, lead=4):
        arr = np.ascontiguousarray(arr)
        assert arr.ndim == 1
        self.n, self.lead = len(arr), lead
        full = np.full(lead + self.n + U.PAD, U.SENTINEL[arr.dtype], dtype=arr.dtype)
        full[lead:lead + self.n] = arr
        self.full = torch.from_numpy(full).cuda()
        self.ptr = self.full[lead:].data_ptr()

    def read(self, what):
        full = self.full.cpu().numpy()
        s = U.SENTINEL[full.dtype]
        assert np.all(full[:self.lead] == s) and np.all(full[self.lead + self.n:] == s), "%s: sentinels overwritten" % (what,)
        return full[self.lead:self.lead + self.n]


def _case(dims, batch, rate, seed):
    key = (dims, batch, rate, seed)
    if key not in _CACHE:
        _CACHE[key] = T.exact_case(dims, batch, rate, seed)
    return _CACHE[key]


def _inputs(c, eflat=None, tflat=None):
    """the raw calls' inputs of an exact case (or of any dict with its keys)"""
    p = {k: c[k] for k in ("dims", "batch", "rate", "gamma", "s", "a", "s2", "r", "masks")}
    p["eflat"] = ddqn_ref.flat_params(c["eval"]) if eflat is None else eflat
    p["tflat"] = ddqn_ref.flat_params(c["target"]) if tflat is None else tflat
    return p


def _device(p, kind, rms=None, live=None, counter=0, eps=0.0, inc=None, lead=4, what=""):
    """one update through ctypes: kind "train" (mxa_qnet_train), "grad" (mxa_qnet_grad alone) or
    "grad+update" (mxa_qnet_grad, then mxa_qnet_update on its gradient). Every buffer the kernels
    write sits behind sentinels; the parameters start `lead` floats past a 256-byte boundary."""
    L = ddqn.lib()
    dims, B = p["dims"], p["batch"]
    n_layers, n_out, P = len(dims) - 1, dims[-1], len(p["eflat"])
    cd = (ctypes.c_int * len(dims))(*dims)
    st = torch.cuda.current_stream().cuda_stream
    ev, tg = Flat(p["eflat"], lead), Flat(p["tflat"], lead)
    assert ev.ptr % 16 == (0 if lead == 4 else 4)
    rm = Flat(np.zeros(P, dtype=np.float32) if rms is None else rms, lead)
    s, s2 = U.Guarded(p["s"].astype(np.float32)), U.Guarded(p["s2"].astype(np.float32))
    a, r = U.Guarded(p["a"].astype(np.int64)), U.Guarded(p["r"].astype(np.float32))
    masks = None
    keep = []
    if p["masks"] is not None:
        masks = (ctypes.c_void_p * max(1, n_layers - 1))()
        for h in range(1, n_layers - 1):
            keep.append(U.Guarded(p["masks"][h - 1]))
            masks[h] = keep[-1].ptr
    ws_bytes = L.mxa_qnet_train_workspace(B, n_layers, cd)
    assert ws_bytes > 0
    ws = Flat(np.zeros(ws_bytes // 4, dtype=np.float32))
    grad, loss = Flat(np.full(P, -3.0, dtype=np.float32)), U.Guarded(np.full(1, -3.0, dtype=np.float32))
    tgt = U.Guarded(np.full((B, n_out), -3.0, dtype=np.float32))
    lv = None if live is None else U.Guarded(np.array([live], dtype=np.bool_))
    cnt, ep = U.Guarded(np.array([counter], dtype=np.int64)), U.Guarded(np.array([eps], dtype=np.float64))
    batch = (B, s.ptr, a.ptr, s2.ptr, r.ptr, ev.ptr, tg.ptr, n_layers, cd, masks, p["rate"], p["gamma"], ws.ptr, grad.ptr,
             loss.ptr, tgt.ptr)
    upd = (cnt.ptr, ITER, ep.ptr, int(inc is not None), 0.0 if inc is None else inc, EPS_MAX, LR, RHO, RMS_EPS)
    lvp = None if lv is None else lv.ptr
    if kind == "train":
        rc = L.mxa_qnet_train(st, *batch, rm.ptr, lvp, *upd)
    else:
        rc = L.mxa_qnet_grad(st, *batch)
        if rc == 0 and kind == "grad+update":
            rc = L.mxa_qnet_update(st, P, grad.ptr, ev.ptr, tg.ptr, rm.ptr, lvp, *upd)
    assert rc == 0, (what, kind, rc)
    torch.cuda.synchronize()
    ws.read((what, "workspace"))
    for g in [s, s2, a, r] + keep:  # the inputs are left alone
        g.read((what, "input"))
    return {"grad": grad.read((what, "grad")), "loss": loss.read((what, "loss"))[0], "tgt": tgt.read((what, "tgt")),
            "eflat": ev.read((what, "eval")), "tflat": tg.read((what, "target")), "rms": rm.read((what, "rms")),
            "eps": float(ep.read((what, "eps"))[0]), "counter": int(cnt.read((what, "counter"))[0])}


STATE = ("eflat", "tflat", "rms", "eps", "counter")


def _same_state(got, want, what):
    for k in STATE:
        if k in ("eps", "counter"):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert U.same(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def _unfused_learner(c, inc):
    """an autograd learner holding the case's nets (its layer weights written into the nn.Linears
    through the flat buffers they are views of)"""
    dims = c["dims"]
    ddqn.QNet.WIDTHS["exact_case"] = tuple(dims[1:-1])
    try:
        L = ddqn.DDQNLearner(n_state=dims[0], n_actions=dims[-1], model="exact_case", dropout=c["rate"],
                             batch_size=c["batch"], reward_decay=c["gamma"], learning_rate=LR, epsilon_increment=inc,
                             epsilon_max=EPS_MAX, replace_target_iter=ITER, device="cuda", seed=1, fused_act=False,
                             fused_learn=False)
    finally:
        del ddqn.QNet.WIDTHS["exact_case"]
    assert [lin.in_features for lin in list(L.eval_model.hidden) + [L.eval_model.logits]] == list(dims[:-1])
    L.eflat.copy_(torch.from_numpy(ddqn_ref.flat_params(c["eval"])).cuda())
    L.tflat.copy_(torch.from_numpy(ddqn_ref.flat_params(c["target"])).cuda())
    W0 = L.eval_model.hidden[0].weight.detach().cpu().numpy()
    assert np.array_equal(W0.T.astype(np.float64), c["eval"][0][0])
    return L


def _learn_on(L, c):
    dv = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda()
    masks = None if c["masks"] is None else [torch.from_numpy(m).cuda() for m in c["masks"]]
    return L.learn_on(dv(c["s"]), torch.from_numpy(c["a"]).cuda(), dv(c["s2"]), dv(c["r"]), masks=masks)


@pytest.mark.parametrize("dims,batch,rate,seed", T.EXACT_CASES)
def test_gpu_train_exact_cases_bit_for_bit(dims, batch, rate, seed):
    """grad, loss and tgt_out equal oracle/ddqn_ref.py's float64 results exactly, with the
    parameters on a 16-byte boundary (16-byte staging) and one float past it (plain staging); the
    state after mxa_qnet_train equals an unfused learner's after learn_on on the same nets, bit
    for bit: every quantity of these cases is exact, so the summation order cannot matter"""
    c = _case(dims, batch, rate, seed)
    ref_g = T.flat_grads(c["grads"]).astype(np.float32)
    outs = []
    for lead in (4, 5):
        o = _device(_inputs(c), "train", inc=0.25, lead=lead, what=(dims, batch, lead))
        assert U.same(o["tgt"], c["tgt"].astype(np.float32)), (dims, batch, lead)
        assert U.same(o["grad"], ref_g), (dims, batch, lead, int((o["grad"] != ref_g).sum()))
        assert o["loss"] == np.float32(c["loss"]) and o["loss"].dtype == np.float32
        outs.append(o)
    _same_state(outs[1], outs[0], (dims, batch, "shifted"))
    if len(dims) > 2:  # QNet has at least one hidden layer
        L = _unfused_learner(c, 0.25)
        loss = _learn_on(L, c)
        got = {"eflat": L.eflat.cpu().numpy(), "tflat": L.tflat.cpu().numpy(), "rms": L.rms.cpu().numpy(),
               "eps": L.epsilon, "counter": L.learn_step_counter}
        _same_state(outs[0], got, (dims, batch, "unfused learn_on"))
        assert loss.dtype == torch.float32 and float(loss) == float(outs[0]["loss"])
    want = T.update_ref_f32(ddqn_ref.flat_params(c["eval"]), ddqn_ref.flat_params(c["target"]), ref_g,
                            np.zeros(len(ref_g), dtype=np.float32), True, 0, ITER, 0.0, 0.25, EPS_MAX, LR, RHO, RMS_EPS)
    _same_state(outs[0], dict(zip(STATE, want)), (dims, batch, "update_ref_f32"))


def _torch_update(p, g, rms, live, counter, eps, inc):
    """learn_on's own torch expressions on the device, on a given gradient"""
    dev = "cuda"
    eflat, tflat = torch.from_numpy(p["eflat"]).to(dev), torch.from_numpy(p["tflat"]).to(dev)
    g, rms0 = torch.from_numpy(g).to(dev), torch.from_numpy(rms).to(dev)
    live = torch.tensor(True if live is None else live, device=dev)
    cnt = torch.tensor(counter, dtype=torch.int64, device=dev)
    e = torch.tensor(eps, dtype=torch.float64, device=dev)
    do_copy = live & (cnt % ITER == 0)
    tflat = torch.where(do_copy, eflat, tflat)
    rms = RHO * rms0 + (1 - RHO) * g * g
    rms = torch.where(live, rms, rms0)
    step = LR * g / (torch.sqrt(rms) + RMS_EPS)
    eflat = eflat - torch.where(live, step, torch.zeros_like(step))
    if inc is not None:
        e2 = torch.where(e < EPS_MAX, e + inc, torch.full_like(e, EPS_MAX))
        e = torch.where(live, e2, e)
    cnt = cnt + live.to(torch.int64)
    return {"eflat": eflat.cpu().numpy(), "tflat": tflat.cpu().numpy(), "rms": rms.cpu().numpy(), "eps": float(e),
            "counter": int(cnt)}


def _glorot_inputs(model, batch, seed=5, fused_act=True):
    """a glorot-initialised learner's nets (rate 0.1, gamma 0.98) and a batch with its dropout masks"""
    L = ddqn.DDQNLearner(device="cuda", seed=seed, model=model, batch_size=batch, fused_act=fused_act)
    rs = np.random.RandomState(batch)
    s, s2 = rs.randint(0, 200, (batch, 2)).astype(np.float64), rs.randint(0, 200, (batch, 2)).astype(np.float64)
    a, r = rs.randint(0, 24, batch).astype(np.int64), rs.normal(0, 50, batch).astype(np.float32).astype(np.float64)
    masks = [m.cpu().numpy() for m in L.dropout_masks(batch)]
    p = {"dims": tuple(L._qdims), "batch": batch, "rate": 0.1, "gamma": 0.98, "s": s, "a": a, "s2": s2, "r": r,
         "masks": masks, "eflat": L.eflat.cpu().numpy(), "tflat": L.tflat.cpu().numpy()}
    return L, p


UNDER = float(np.nextafter(EPS_MAX, 0.0))
# (counter, eps, inc): no increment; an increment from 0; just under eps_max (overshoots), then the clamp
EDGES = [(0, EPS_MAX, None), (1, 0.0, 0.25), (4, UNDER, 0.5), (5, UNDER + 0.5, 0.5)]


@pytest.mark.parametrize("which", ["glorot", 1, 5])
def test_gpu_train_update_edges(which):
    """from a non-zero, non-dyadic rms: the state after mxa_qnet_train equals update_ref_f32 (numpy
    float32, op by op) applied to the kernel's own grad, and the torch expressions of learn_on run
    on the device on that grad; mxa_qnet_grad then mxa_qnet_update gives mxa_qnet_train's bits;
    counters 0 and 5 copy the eval parameters from before the step into the target, 1 and 4 leave
    it; the epsilon edges; live false touches none of the five buffers and still writes grad and
    loss; a second run gives the same bits"""
    if which == "glorot":
        p = _glorot_inputs("NNModel_1", 32)[1]
    else:
        p = _inputs(_case(*T.EXACT_CASES[which]))
    P = len(p["eflat"])
    rms0 = (np.random.RandomState(7).rand(P) * 0.01 + 1e-4).astype(np.float32)
    first = None
    for counter, eps, inc in (EDGES if which == "glorot" else EDGES[:2]):
        what = (which, counter)
        o = _device(p, "train", rms=rms0, counter=counter, eps=eps, inc=inc, what=what)
        if first is None:
            first = o
        assert U.same(o["grad"], first["grad"]) and o["loss"] == first["loss"] and U.same(o["tgt"], first["tgt"])
        want = dict(zip(STATE, T.update_ref_f32(p["eflat"], p["tflat"], o["grad"], rms0, True, counter, ITER, eps, inc,
                                                EPS_MAX, LR, RHO, RMS_EPS)))
        _same_state(o, want, (what, "update_ref_f32"))
        copied = counter % ITER == 0
        assert U.same(o["tflat"], p["eflat"] if copied else p["tflat"]), what
        assert not U.same(o["eflat"], p["eflat"]) and not U.same(p["eflat"], p["tflat"])
        assert o["counter"] == counter + 1
        assert o["eps"] == {0: EPS_MAX, 1: 0.25, 4: UNDER + 0.5, 5: EPS_MAX}[counter]
        # learn_on's expressions on the device; a difference is counted and the operation named
        t = _torch_update(p, o["grad"], rms0, None, counter, eps, inc)
        bad_rms, bad_e = int((t["rms"] != o["rms"]).sum()), int((t["eflat"] != o["eflat"]).sum())
        assert bad_rms == 0, "%s: rho * rms + (1 - rho) * g * g differs from torch's at %d of %d elements" % (what, bad_rms, P)
        assert bad_e == 0, "%s: lr * g / (sqrt(rms) + eps) or the subtraction differs from torch's at %d of %d elements" % (
            what, bad_e, P)
        _same_state(o, t, (what, "torch expressions"))
        split = _device(p, "grad+update", rms=rms0, counter=counter, eps=eps, inc=inc, what=(what, "split"))
        _same_state(split, o, (what, "grad then update"))
        assert U.same(split["grad"], o["grad"]) and split["loss"] == o["loss"] and U.same(split["tgt"], o["tgt"])
    again = _device(p, "train", rms=rms0, counter=EDGES[0][0], eps=EDGES[0][1], inc=EDGES[0][2], what=(which, "again"))
    _same_state(again, first, (which, "second run"))
    assert U.same(again["grad"], first["grad"]) and again["loss"] == first["loss"]
    for kind in ("train", "grad+update"):
        dead = _device(p, kind, rms=rms0, live=False, counter=5, eps=0.0, inc=0.25, what=(which, "dead", kind))
        _same_state(dead, {"eflat": p["eflat"], "tflat": p["tflat"], "rms": rms0, "eps": 0.0, "counter": 5}, (which, "dead"))
        assert U.same(dead["grad"], first["grad"]) and dead["loss"] == first["loss"]
    alive = _device(p, "train", rms=rms0, live=True, counter=EDGES[0][0], eps=EDGES[0][1], inc=EDGES[0][2], what=(which, "live"))
    _same_state(alive, first, (which, "live true"))


def _layers(net):
    return [(lin.weight.detach().cpu().numpy().T.astype(np.float64), lin.bias.detach().cpu().numpy().astype(np.float64))
            for lin in list(net.hidden) + [net.logits]]


@pytest.mark.parametrize("batch", [1, 31, 32, 33, 256])
@pytest.mark.parametrize("model", ["NNModel_1", "NNModel_2"])
def test_gpu_train_real_nets(model, batch):
    """glorot nets, rate 0.1, gamma 0.98: tgt_out has the bits of DDQNLearner(fused_act=True).q_target;
    grad against oracle/ddqn_ref.mse_grads in float64, at most 4x the autograd path's own maximum
    absolute error against that reference on the same batch (both are fp32 sums of the same terms
    in another order; the factor covers order luck over the ~38 k elements). Measured on an
    MI355X, max |g - g64| kernel / autograd (max |g64|), batch 1, 31, 32, 33, 256:
    NNModel_1 3.8e-5 / 2.7e-5 (54.1), 8.4e-6 / 1.0e-5 (15.1), 1.1e-5 / 6.7e-6 (13.8), 8.0e-6 / 6.4e-6
    (11.5), 6.7e-6 / 7.8e-6 (8.6); NNModel_2 1.4e-5 / 1.7e-5 (46.1), 5.8e-6 / 4.9e-6 (5.3), 5.7e-6 /
    6.2e-6 (6.8), 4.2e-6 / 6.4e-6 (4.1), 5.1e-6 / 4.3e-6 (3.9): the ratio spans 0.65 .. 1.72."""
    L, p = _glorot_inputs(model, batch)
    dv = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda()
    s, a, s2, r = dv(p["s"]), torch.from_numpy(p["a"]).cuda(), dv(p["s2"]), dv(p["r"])
    o = _device(p, "grad", what=(model, batch))
    assert U.same(o["tgt"], L.q_target(s, a, s2, r).cpu().numpy()), (model, batch)
    ev, tg = _layers(L.eval_model), _layers(L.target_model)
    tgt64 = ddqn_ref.q_target(ev, tg, p["s"], p["a"], p["s2"], p["r"], 0.98)
    loss64, grads = ddqn_ref.mse_grads(ev, p["s"], tgt64, p["masks"], 0.1)
    ref = T.flat_grads(grads)
    # the autograd path: learn_on's own lines on an unfused learner with the same nets
    Lu = ddqn.DDQNLearner(device="cuda", seed=5, model=model, batch_size=batch, fused_act=False, fused_learn=False)
    assert torch.equal(Lu.eflat, L.eflat) and torch.equal(Lu.tflat, L.tflat)
    tgt = Lu.q_target(s, a, s2, r)
    Lu.eval_model.train()
    loss = torch.mean((Lu.eval_model(s, [torch.from_numpy(m).cuda() for m in p["masks"]]) - tgt) ** 2)
    loss.backward()
    g_auto = torch.cat([q.grad.reshape(-1) for q in Lu.eval_model.parameters()]).cpu().double().numpy()
    err_auto = np.abs(g_auto - ref).max()
    err_kernel = np.abs(o["grad"].astype(np.float64) - ref).max()
    print("%s batch %d: max |g - g64| kernel %.3e, autograd %.3e, max |g64| %.3e; loss kernel %.6e, fp64 %.6e"
          % (model, batch, err_kernel, err_auto, np.abs(ref).max(), o["loss"], loss64))
    assert np.abs(ref).max() > 0 and err_auto > 0
    assert err_kernel <= 4 * err_auto, (model, batch, err_kernel, err_auto)
    assert abs(float(o["loss"]) - loss64) <= 2e-2 * max(1.0, loss64)


def _batch(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 200, (n, 2)).astype(np.float64), rs.randint(0, 24, n), rs.randint(0, 200, (n, 2)).astype(np.float64),
            rs.normal(0, 50, n))


def test_gpu_fused_learner_updates_match_numpy_reference():
    """the float32 row of test_gpu_learner_updates_match_numpy_reference with fused_learn=True: the
    same 18 updates against oracle/ddqn_ref.train_step, each from the learner's own current state,
    with that test's tolerances"""
    rtol, atol = 2e-3, 2e-4
    L = ddqn.DDQNLearner(device="cuda", dropout=0.0, seed=3, batch_size=32, fused_learn=True)
    assert L.fused_learn
    dv = lambda x: torch.from_numpy(x).to("cuda", torch.float32)
    counter = 0
    for it in range(18):
        s, a, s2, r = _batch(32, 100 + it)
        ev, tg = _layers(L.eval_model), _layers(L.target_model)
        rr = L.rms.detach().cpu().double().numpy()
        rms, off = [], 0
        for W, b in ev:
            rms.append((rr[off:off + W.size].reshape(W.shape[1], W.shape[0]).T.copy(),
                        rr[off + W.size:off + W.size + b.size].copy()))
            off += W.size + b.size
        ev, tg, rms, counter, loss = ddqn_ref.train_step(ev, tg, rms, counter, (s, a, s2, r))
        cost = L.learn_on(dv(s), torch.from_numpy(a).cuda(), dv(s2), dv(r))
        assert cost.dtype == torch.float32 and cost.dim() == 0
        assert abs(float(cost) - loss) <= rtol * max(1.0, loss) * 10, it
        for net, ref in ((L.eval_model, ev), (L.target_model, tg)):
            for (W, b), (W2, b2) in zip(_layers(net), ref):
                np.testing.assert_allclose(W, W2, rtol=rtol, atol=atol, err_msg="update %d" % it)
                np.testing.assert_allclose(b, b2, rtol=rtol, atol=atol, err_msg="update %d" % it)
    assert L.learn_step_counter == 18
    assert len(L.cost_hist) == 18


def _fill(L, seed):
    """as tests/test_gpu_qnet_fused.py's"""
    rs = np.random.RandomState(seed)
    n = 64
    dv = lambda v: torch.from_numpy(v).to("cuda", torch.float32)
    L.memory.add(dv(rs.randint(0, 200, (n, 2)).astype(np.float64)), torch.from_numpy(rs.randint(0, 24, n)).cuda(),
                 dv(rs.randint(0, 200, (n, 2)).astype(np.float64)), dv(rs.normal(0, 50, n)),
                 torch.ones(n, dtype=torch.bool, device="cuda"))


def test_gpu_fused_learn_through_the_learner():
    Ls = {}
    for fused in (False, True):
        L = ddqn.DDQNLearner(device="cuda", seed=9, epsilon_increment=0.25, fused_act=False, fused_learn=fused)
        assert L.fused_learn is fused
        assert L.learn() is None  # below the batch size
        _fill(L, 1)
        for _ in range(3):
            loss = L.learn()
            assert loss is not None and loss.dtype == torch.float32 and loss.dim() == 0
        Ls[fused] = L
    a, b = Ls[False], Ls[True]
    assert torch.equal(a.gen_sample.get_state(), b.gen_sample.get_state())
    assert torch.equal(a.gen_drop.get_state(), b.gen_drop.get_state())
    assert a.learn_step_counter == b.learn_step_counter == 3
    assert a.epsilon == b.epsilon == 0.75
    assert len(a.cost_hist) == len(b.cost_hist) == 3
    assert all(np.isfinite(c) for c in a.cost_hist + b.cost_hist)
    # the eval parameters are views of eflat and see the update
    assert b.eval_model.logits.bias.data_ptr() == b.eflat[-24:].data_ptr()
    assert not torch.equal(b.eflat, ddqn.DDQNLearner(device="cuda", seed=9).eflat)
    # a masked update through the learner is a no-op
    e0, t0, r0 = b.eflat.clone(), b.tflat.clone(), b.rms.clone()
    b.learn(live=torch.zeros((), dtype=torch.bool, device="cuda"))
    assert torch.equal(b.eflat, e0) and torch.equal(b.tflat, t0) and torch.equal(b.rms, r0)
    assert b.learn_step_counter == 3 and len(b.cost_hist) == 3
    # dimensions outside the kernels': refused with True
    with pytest.raises(RuntimeError):
        ddqn.DDQNLearner(device="cuda", seed=9, batch_size=257, fused_learn=True)


def test_gpu_fused_learn_episode():
    """one 64-env run_episode with fused_learn and fused_act: stored, env_steps and
    learn_step_counter equal the unfused run's on the same seeds; the costs are finite"""
    from mxabides.gym import VecABIDESEnv
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        base = SEEDS * 4  # 64 envs
        v = VecABIDESEnv(seeds=base)
        v.set_stream(stream.cuda_stream)
        task = ddqn.ExecutionTask(device="cuda")
        res = {}
        for fused in (False, True):
            learner = ddqn.DDQNLearner(device="cuda", seed=1, batch_size=32, fused_act=fused, fused_learn=fused)
            out = ddqn.run_episode(v, learner, task, seeds=base, fused=True)
            torch.cuda.synchronize()
            cost = learner.cost_hist
            assert cost and all(np.isfinite(c) for c in cost)
            res[fused] = (int(out["stored"]), out["env_steps"].cpu().numpy(), learner.learn_step_counter, len(cost))
        assert res[True][0] == res[False][0] > 0
        assert np.array_equal(res[True][1], res[False][1])
        assert res[True][2] == res[False][2] > 0
        assert res[True][3] == res[False][3]
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
