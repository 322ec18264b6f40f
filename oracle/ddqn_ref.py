"""TEST INFRASTRUCTURE ONLY (the checker, never the product path): a float64 numpy restatement
of the reference DDQN learner's arithmetic, for the parity tests of mxabides.ddqn.

Follows agent/execution/qlearning/ddqlearning_execution_agent.py and util/model/QNets.py; the
Keras 2 (TensorFlow 2.1, requirements.txt:17) pieces are restated from their published
algorithm because TensorFlow is not installed here: Dense = x @ W + b with W
[in, out]; `mse` = mean over all elements; RMSprop optimizer_v2 with momentum 0, not centered:
rms = rho*rms + (1-rho)*g^2, w -= lr * g / (sqrt(rms) + eps). Parity with Keras itself is
therefore unpinned; what is pinned is the reference's own algorithm around it (the target of
train_neural_nets, the action table, the state discretization)."""
import numpy as np


def action_table(size_allocation, size_scale):
    """ddqlearning_execution_agent.py:27-37"""
    alloc = list(size_allocation.keys())
    alloc.append(0)
    alloc.sort()
    acts, k = {}, 0
    for i in range(len(alloc)):
        for j in range(len(size_scale)):
            acts[k] = (alloc[i], size_scale[j])
            k += 1
    return acts


def forward(layers, x, masks=None, rate=0.1):
    """layers: [(W [in,out], b)], ReLU on all but the last (QNets.py:19-27).  masks: the keep
    masks of the Dropout(rate) layers after hidden layers 2..n in training mode (QNets.py:22-26;
    Keras scales kept units by 1 / (1 - rate)); None = predict(), no dropout."""
    acts = [x]
    for i, (W, b) in enumerate(layers):
        z = acts[-1] @ W + b
        if i == len(layers) - 1:
            acts.append(z)
            continue
        h = np.maximum(z, 0.0)
        if masks is not None and i >= 1:
            h = h * masks[i - 1] / (1.0 - rate)
        acts.append(h)
    return acts


def q_target(eval_layers, target_layers, s, a, s2, r, gamma):
    """train_neural_nets, ddqlearning_execution_agent.py:475-490"""
    q_next = forward(target_layers, s2)[-1]
    q_eval4next = forward(target_layers, s2)[-1]
    q_eval = forward(eval_layers, s)[-1]
    tgt = q_eval.copy()
    bi = np.arange(len(s))
    tgt[bi, a.astype(int)] = r + gamma * q_next[bi, np.argmax(q_eval4next, axis=1)]
    return tgt


def mse_grads(layers, x, tgt, masks=None, rate=0.1):
    """loss = mean((f(x) - tgt)^2) and d loss / d (W, b) for every layer (train_on_batch: the
    dropout masks of training mode, if given)."""
    acts = forward(layers, x, masks, rate)
    out = acts[-1]
    loss = np.mean((out - tgt) ** 2)
    d = 2.0 * (out - tgt) / out.size
    grads = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        W, _ = layers[i]
        grads[i] = (acts[i].T @ d, d.sum(0))
        if i:
            # acts[i] = relu(z) (* mask / (1 - rate) after a dropout layer): > 0 exactly where
            # both the ReLU and the mask pass
            scale = 1.0 / (1.0 - rate) if (masks is not None and i - 1 >= 1) else 1.0
            d = (d @ W.T) * (acts[i] > 0) * scale
    return loss, grads


def rmsprop_step(layers, grads, rms, lr, rho=0.9, eps=1e-7):
    """Keras optimizer_v2 RMSprop, momentum 0, not centered (TF 2.1 rmsprop.py)."""
    new, new_rms = [], []
    for (W, b), (gW, gb), (rW, rb) in zip(layers, grads, rms):
        rW = rho * rW + (1 - rho) * gW * gW
        rb = rho * rb + (1 - rho) * gb * gb
        new.append((W - lr * gW / (np.sqrt(rW) + eps), b - lr * gb / (np.sqrt(rb) + eps)))
        new_rms.append((rW, rb))
    return new, new_rms


def step_reward(fills, arrival, q0):
    """compute_reward summed over fills [(qty, fill_price)] for a BUY (ddqlearning_execution_agent.py:425-432)"""
    return sum((1 - ((f - arrival) / arrival)) * q / q0 * 10000 for q, f in fills)


def train_step(eval_layers, target_layers, rms, counter, batch, lr=0.01, gamma=0.98, replace_target_iter=5, masks=None,
               rate=0.1):
    """One whole `train_neural_nets` update (ddqlearning_execution_agent.py:448-515) after the
    batch is sampled, in the reference's order:
      1. q_next, q_eval4next from the target net AS IT STANDS, q_eval from eval (:486-505);
      2. then, if learn_step_counter % replace_target_iter == 0, eval -> target (:508-510);
      3. then train_on_batch on the eval net (:513): MSE, one RMSprop step;
      4. epsilon, then learn_step_counter += 1 (:526-530).
    batch = (s, a, s2, r); masks: train_on_batch's dropout keep masks (None: dropout off).
    Returns (eval', target', rms', counter', loss)."""
    s, a, s2, r = batch
    tgt = q_target(eval_layers, target_layers, s, a, s2, r, gamma)
    if counter % replace_target_iter == 0:
        target_layers = [(W.copy(), b.copy()) for W, b in eval_layers]
    loss, grads = mse_grads(eval_layers, s, tgt, masks, rate)
    eval_layers, rms = rmsprop_step(eval_layers, grads, rms, lr)
    return eval_layers, target_layers, rms, counter + 1, loss


# ---- plain references of the device kernels (include/mxa_ddqn.h).  float64
# IEEE arithmetic, one rounding per operation, nothing taken from the code under test: the kernels'
# tests compare with exact equality.

def state_ref(obs, g0, g1, nh, q0):
    """ddqlearning_execution_agent.py:301-331 with agent/execution/util.py:25-40: the bin indices
    [n, 2] (int64) of 2 * remaining_time / len - 1 and 2 * remaining_qty / quantity - 1, true
    divisions, np.digitize (NaN and +inf -> len(bins), -inf -> 0)."""
    obs = np.asarray(obs, dtype=np.float64)
    out = np.zeros((len(obs), 2), dtype=np.int64)
    if len(obs):
        out[:, 0] = np.digitize(2 * (obs[:, 0] / float(nh)) - 1, np.asarray(g0, dtype=np.float64))
        out[:, 1] = np.digitize(2 * (obs[:, 1] / float(q0)) - 1, np.asarray(g1, dtype=np.float64))
    return out


def actions_ref(obs, a, table, q0):
    """take_action (:364-407) as the DummyRL action vector [n, 3]: the table's row of a, or on the
    last horizon step (obs[0] == 1) the whole remaining quantity at allocation (1, 0).  The
    quantity share is obs[1] * (1 / q0), the device's arithmetic: the engine places
    rint(q0 * x) shares, which is the quantity itself either way (rint_of_share_is_exact)."""
    out = np.zeros((len(a), 3), dtype=np.float64)
    inv = 1.0 / float(q0)
    for i in range(len(a)):
        if obs[i][0] == 1.0:
            out[i] = (obs[i][1] * inv, 1.0, 0.0)
        else:
            out[i] = table[int(a[i])]
    return out


def rint_of_share_is_exact(q0, q_max):
    """rint(q0 * (q * (1 / q0))) == q for every integer quantity 0..q_max"""
    q = np.arange(int(q_max) + 1, dtype=np.float64)
    return bool(np.all(np.rint(float(q0) * (q * (1.0 / float(q0)))) == q))


def period_ref(n, obs_w, st_w, train, obs, st, prev, arrival, flags, alive, s, a, env_steps, g0, n0, g1, n1, nh, q0,
               rscale, ring_s, ring_s2, ring_a, ring_r, cap, n_dev, stored):
    """One period of the learner loop (place_order, :275-299) for n envs, the arguments of
    mxa_ddqn_period as numpy arrays; the inputs are left unchanged and every output is returned.
    ok = alive & obs valid (flag bit 1) & no env error (bit 2); the reward is compute_reward summed
    over the step's fills (BUY): rscale * (2 dq + dcash / arrival) when dq > 0, else 0; the ok
    envs' rows (s, a, s2, float32(r)) are appended in env order at (n_dev + k) % cap."""
    obs = np.asarray(obs, dtype=np.float64).reshape(n, obs_w)
    st = np.asarray(st, dtype=np.float64).reshape(n, st_w)
    prev = np.asarray(prev, dtype=np.float64).reshape(n, st_w)
    s2 = state_ref(obs, g0[:n0], g1[:n1], nh, q0).astype(np.float32)
    alive_next = np.zeros(n, dtype=bool)
    r_row = np.zeros(n, dtype=np.float64)
    env_steps = np.array(env_steps, dtype=np.int64)
    ring_s, ring_s2 = np.array(ring_s, dtype=np.float32), np.array(ring_s2, dtype=np.float32)
    ring_a, ring_r = np.array(ring_a, dtype=np.int64), np.array(ring_r, dtype=np.float32)
    n_dev, stored = int(n_dev), int(stored)
    live = False
    k = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            f = int(flags[i])
            al = bool(alive[i])
            live = live or al
            ok = al and (f & 2) != 0 and (f & 4) == 0
            dq = st[i, 2] - prev[i, 2]
            dcash = st[i, 0] - prev[i, 0]
            r = np.float64(rscale) * (2.0 * dq + dcash / np.float64(arrival[i])) if dq > 0 else np.float64(0.0)
            env_steps[i] += 1 if al else 0
            r_row[i] = r if ok else 0.0
            alive_next[i] = ok and (f & 1) == 0
            if train and ok:
                pos = (n_dev + k) % int(cap)
                ring_s[pos] = s[i]
                ring_s2[pos] = s2[i]
                ring_a[pos] = a[i]
                ring_r[pos] = np.float32(r)
                k += 1
    return {"alive_next": alive_next, "live": live, "s2": s2, "r_row": r_row, "env_steps": env_steps,
            "ring_s": ring_s, "ring_s2": ring_s2, "ring_a": ring_a, "ring_r": ring_r,
            "n_dev": n_dev + k, "stored": stored + k}


def qnet_ref(layers, x):
    """Keras predict of a Dense stack (QNets.py:7-51) in float64: layers [(W [in, out], b)], ReLU
    on all but the last; a NaN passes through the ReLU."""
    h = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i, (W, b) in enumerate(layers):
            h = h @ np.asarray(W, dtype=np.float64) + np.asarray(b, dtype=np.float64)
            if i + 1 < len(layers):
                h = np.where(h < 0, 0.0, h)
    return h


def integer_net(dims, n_rows, seed, nnz=None):
    """A net and n_rows inputs whose float32 fmaf chain is exact in any summation order: inputs
    integers in [-4, 4], biases integers in [-3, 3], weights from {-2, -1, 1, 2} (with `nnz`, that
    many nonzeros per neuron at random inputs, else dense).  Asserts that sum_k |a_k| |w_k| + |b|
    < 2**24 for every neuron and every row (a condition on the inputs: every partial sum is then
    an integer that float32 holds), so the float32 result must equal qnet_ref bit for bit.
    Returns (layers [(W [in, out], b)], x [n_rows, dims[0]], the worst such sum)."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, (n_rows, dims[0])).astype(np.float64)
    layers, h, worst = [], x, 0.0
    for i in range(len(dims) - 1):
        n_in, n_out = dims[i], dims[i + 1]
        W = rs.choice([-2.0, -1.0, 1.0, 2.0], (n_in, n_out))
        if nnz is not None and nnz < n_in:
            keep = np.zeros((n_in, n_out), dtype=bool)
            for j in range(n_out):
                keep[rs.choice(n_in, nnz, replace=False), j] = True
            W = W * keep
        b = rs.randint(-3, 4, n_out).astype(np.float64)
        bound = np.abs(h) @ np.abs(W) + np.abs(b)
        worst = max(worst, float(bound.max()))
        assert bound.max() < 2 ** 24, (dims, i, float(bound.max()))
        layers.append((W, b))
        h = np.maximum(h @ W + b, 0.0)  # the next layer's inputs
    return layers, x, worst


def flat_params(layers):
    """the flat float32 parameter buffer of include/mxa_ddqn.h mxa_qnet_*: per layer weight[out][in]
    row-major, then bias[out]"""
    return np.concatenate([np.concatenate([W.T.reshape(-1), b]) for W, b in layers]).astype(np.float32)
