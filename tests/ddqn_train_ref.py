"""Shared by tests/test_ddqn_train_refs.py (CPU) and tests/test_gpu_ddqn_train.py (GPU): plain numpy
around oracle/ddqn_ref.py (q_target, mse_grads, train_step) for the training exports of
include/mxa_ddqn_train.h. `exact_case` builds nets and a batch whose whole update is exact in fp32
in any summation order, so the kernels must give the float64 reference's bits; `update_ref_f32` is
mxa_qnet_update in numpy float32, op by op. The expected values come from oracle/ddqn_ref.py and
from the expressions in the header, never from the code under test."""
import numpy as np

import ddqn_ref

GAMMA = 0.5
NNMODEL_1 = (2, 32, 64, 128, 128, 64, 32, 8)
NNMODEL_2 = (2, 32, 64, 128, 256, 128, 64, 32, 8)
# (dims, batch, rate, seed): the cases the GPU tests run. The seeds are the first of 3, 4, 5, ...
# for which exact_case's conditions (the magnitudes, and a nonzero gradient entry in every layer's
# weights and biases) hold; tests/test_ddqn_train_refs.py checks every one on the CPU
EXACT_CASES = [
    (NNMODEL_1, 1, 0.5, 17), (NNMODEL_1, 32, 0.5, 3), (NNMODEL_1, 64, 0.5, 3), (NNMODEL_1, 32, 0.0, 3),
    (NNMODEL_2, 32, 0.5, 3), ((3, 5, 255, 1, 65, 16), 16, 0.5, 3), ((7, 256, 256, 4), 8, 0.5, 3),
    ((2, 8), 4, 0.5, 3),                                   # a single layer: no hidden layer, no mask
    ((2, 16, 16, 16, 16, 16, 16, 16, 4), 16, 0.5, 6),      # eight layers
]


def _sparse_net(rs, dims):
    """weights from {-1, +1} with 2 nonzeros per neuron (1 where the layer has one input), biases in {0, 1}"""
    layers = []
    for i in range(len(dims) - 1):
        n_in, n_out = dims[i], dims[i + 1]
        W = np.zeros((n_in, n_out))
        for j in range(n_out):
            W[rs.choice(n_in, min(2, n_in), replace=False), j] = rs.choice([-1.0, 1.0], min(2, n_in))
        layers.append((W, rs.randint(0, 2, n_out).astype(np.float64)))
    return layers


def _forward_bound(layers, x, masks, rate):
    """the worst sum of magnitudes sum_k |a_k| |w_k| + |b| over every neuron and row"""
    acts = ddqn_ref.forward(layers, x, masks, rate)
    return max(float((np.abs(acts[i]) @ np.abs(W) + np.abs(b)).max()) for i, (W, b) in enumerate(layers))


def exact_case(dims, batch, rate, seed):
    """eval and target nets and a batch whose whole update is exact in fp32 in any summation
    order: inputs integers in [-2, 2], rewards integers in [-4, 4], gamma 0.5, rate in {0, 0.5}
    (the keep scale is 1 or 2), batch * n_out a power of two. Every forward value is an integer
    and the target a multiple of 1/2, so with q = 1 / (batch * n_out) every delta and every
    gradient term is a multiple of q. ASSERTS the condition on the inputs: the forward sums of
    magnitudes stay below 2^24, every backward sum of magnitudes (|d| @ |W^T| * scale,
    |acts|^T @ |d|, sum_b |d|) below 2^24 q, the summed squared error below 2^22; and that the
    reference gradient has a nonzero entry in every layer's weights and in every layer's biases.
    Returns a dict; `grads`, `loss` and `tgt` are oracle/ddqn_ref.py's float64 results."""
    dims = tuple(dims)
    assert rate in (0.0, 0.5)
    n_out, L = dims[-1], len(dims) - 1
    count = batch * n_out
    assert count & (count - 1) == 0, "batch * n_out must be a power of two"
    rs = np.random.RandomState(seed)
    ev, tg = _sparse_net(rs, dims), _sparse_net(rs, dims)
    s = rs.randint(-2, 3, (batch, dims[0])).astype(np.float64)
    s2 = rs.randint(-2, 3, (batch, dims[0])).astype(np.float64)
    a = rs.randint(0, n_out, batch).astype(np.int64)
    r = rs.randint(-4, 5, batch).astype(np.float64)
    masks = [rs.rand(batch, w) >= 0.5 for w in dims[2:-1]] if rate > 0 else None
    lim = 2.0 ** 24
    worst_f = max(_forward_bound(tg, s2, None, rate), _forward_bound(ev, s, None, rate),
                  _forward_bound(ev, s, masks, rate))
    assert worst_f < lim, (dims, batch, seed, worst_f)
    tgt = ddqn_ref.q_target(ev, tg, s, a, s2, r, GAMMA)
    loss, grads = ddqn_ref.mse_grads(ev, s, tgt, masks, rate)
    # the backward sums of magnitudes, in units of q
    acts = ddqn_ref.forward(ev, s, masks, rate)
    assert 4.0 * float(((acts[-1] - tgt) ** 2).sum()) < lim
    d = np.abs(2.0 * (acts[-1] - tgt))  # |d| / q
    worst_b = 0.0
    for i in range(L - 1, -1, -1):
        W, _ = ev[i]
        worst_b = max(worst_b, float((np.abs(acts[i]).T @ d).max()), float(d.sum(0).max()))
        if i:
            scale = 1.0 / (1.0 - rate) if (masks is not None and i - 1 >= 1) else 1.0
            back = (d @ np.abs(W).T) * scale
            worst_b = max(worst_b, float(back.max()))
            # the magnitudes that flow on are those of the true deltas' bound: |d| through |W|
            d = back * (acts[i] > 0)
    assert worst_b < lim, (dims, batch, seed, worst_b)
    for i, (gW, gb) in enumerate(grads):
        assert np.any(gW != 0) and np.any(gb != 0), "layer %d of %s batch %d seed %d has an all-zero gradient" % (
            i, dims, batch, seed)
    return {"dims": dims, "batch": batch, "rate": rate, "gamma": GAMMA, "eval": ev, "target": tg, "s": s, "a": a,
            "s2": s2, "r": r, "masks": masks, "tgt": tgt, "loss": loss, "grads": grads, "worst_forward": worst_f,
            "worst_backward": worst_b}


def flat_grads(grads):
    """the gradient in the flat parameter layout (float64)"""
    return np.concatenate([np.concatenate([gW.T.reshape(-1), gb]) for gW, gb in grads])


def _matmul_f32(x, W, reverse):
    """x @ W in float32, one sequential sum over the inner index, forwards or backwards"""
    acc = np.zeros((x.shape[0], W.shape[1]), dtype=np.float32)
    ks = range(x.shape[1] - 1, -1, -1) if reverse else range(x.shape[1])
    for k in ks:
        acc = acc + x[:, k, None] * W[None, k, :]
        assert acc.dtype == np.float32
    return acc


def eval_f32(c, reverse=False):
    """the case's target, loss and flat gradient with every operation in float32 and every sum
    sequential in index order, or in the reversed order: (tgt, loss, grad), float32"""
    f = lambda x: np.asarray(x, dtype=np.float32)

    def fwd(layers, x, masks):
        acts = [f(x)]
        for i, (W, b) in enumerate(layers):
            z = _matmul_f32(acts[-1], f(W), reverse) + f(b)
            if i + 1 < len(layers):
                z = np.maximum(z, np.float32(0))
                if masks is not None and i >= 1:
                    z = z * f(masks[i - 1]) * np.float32(1.0 / (1.0 - c["rate"]))
            acts.append(z)
        return acts

    q_next = fwd(c["target"], c["s2"], None)[-1]
    tgt = fwd(c["eval"], c["s"], None)[-1].copy()
    bi = np.arange(c["batch"])
    tgt[bi, c["a"]] = f(c["r"]) + np.float32(c["gamma"]) * q_next[bi, np.argmax(q_next, axis=1)]
    acts = fwd(c["eval"], c["s"], c["masks"])
    diff = acts[-1] - tgt
    sq = (diff * diff).reshape(-1)
    loss = np.float32(0)
    for v in (sq[::-1] if reverse else sq):
        loss = loss + v
    loss = loss / np.float32(sq.size)
    d = (np.float32(2) * diff) / np.float32(sq.size)
    out = [None] * len(c["eval"])
    for i in range(len(c["eval"]) - 1, -1, -1):
        W = f(c["eval"][i][0])
        gW = _matmul_f32(np.ascontiguousarray(acts[i].T), d, reverse)  # sum over the batch
        gb = _matmul_f32(np.ones((1, c["batch"]), dtype=np.float32), d, reverse)[0]
        out[i] = np.concatenate([gW.T.reshape(-1), gb])
        if i:
            scale = np.float32(1.0 / (1.0 - c["rate"]) if (c["masks"] is not None and i - 1 >= 1) else 1.0)
            d = _matmul_f32(d, np.ascontiguousarray(W.T), reverse) * scale * (acts[i] > 0)
    g = np.concatenate(out)
    assert tgt.dtype == loss.dtype == g.dtype == np.float32
    return tgt, loss, g


def update_ref_f32(params, target, g, rms, live, counter, replace_target_iter, eps, inc, eps_max, lr, rho=0.9,
                   rms_eps=1e-7):
    """mxa_qnet_update (include/mxa_ddqn_train.h) in numpy float32, op by op: the flat eval and
    target parameters, the gradient and rms are float32 arrays, eps a float (float64), inc None for
    no increment. Returns (eval', target', rms', eps', counter'); the inputs are left unchanged."""
    f = np.float32
    params, target, g, rms = (np.array(x, dtype=np.float32) for x in (params, target, g, rms))
    if not live:
        return params, target, rms, float(eps), int(counter)
    if int(counter) % int(replace_target_iter) == 0:
        target = params.copy()
    with np.errstate(all="ignore"):
        rms = f(rho) * rms + (f(1 - rho) * g) * g
        step = (f(lr) * g) / (np.sqrt(rms) + f(rms_eps))
        params = params - step
    assert rms.dtype == step.dtype == params.dtype == np.float32
    if inc is not None:
        eps = eps + inc if eps < eps_max else eps_max
    return params, target, rms, float(eps), int(counter) + 1


def unflatten(flat, dims):
    """a flat parameter-layout vector as [(W [in, out], b)] (float64)"""
    flat = np.asarray(flat, dtype=np.float64)
    out, off = [], 0
    for i in range(len(dims) - 1):
        n_in, n_out = dims[i], dims[i + 1]
        W = flat[off:off + n_in * n_out].reshape(n_out, n_in).T.copy()
        off += n_in * n_out
        out.append((W, flat[off:off + n_out].copy()))
        off += n_out
    return out
