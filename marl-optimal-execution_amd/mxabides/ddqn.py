"""DDQN optimal-execution learner on PyTorch-ROCm, fed by the MI355X market step.

Restates the reference's DDQLearningExecutionAgent learner (agent/execution/qlearning/
ddqlearning_execution_agent.py, TensorFlow 2.1 / Keras, requirements.txt:17) for thousands of
parallel envs on one device:

* the 24-action table: SIZE_ALLOCATION x SIZE_SCALE (ddqlearning_execution_agent.py:21-37);
* the state: `discretize([time_remaining, qty_remaining, ...], grid)` on a 200 x 200 uniform grid
  over [0, 1]^2 (:129, :301-331; agent/execution/util.py:5-40). `discretize` zips the six
  features with the two grid axes, so the state is the two bin indices of time and quantity.
  Both features divide truly (remaining / total), on the CPU, in the PyTorch ops on the device
  and in libmxa_ddqn.so's kernels alike, so all three give np.digitize's bins of the reference's
  own expressions (oracle/ddqn_ref.state_ref; a multiply by 1/quantity would not). The four
  features the reference's zip drops ("add market variables to observation TBD") can be had:
  `ExecutionTask(features=[Feature(...), ...])` makes the state any 1..8 features of the
  observation row, each binned on its own split points or passed through, in the PyTorch ops, the
  per-period kernels and the policy inside the step kernel alike (include/mxa_state_spec.h);
* the Q-network NNModel_1 (util/model/QNets.py:7-27: Dense 32-64-128-128-64-32 ReLU, Dropout 0.1
  after layers 2-6, linear 24-way head; Keras defaults glorot_uniform / zero bias), EvalModel and
  TargetModel (QNets.py:54-60); NNModel_2 (:30-51) by name;
* epsilon-greedy `choose_action` (:333-362): exploit when U < epsilon and enough experience,
  else `randint(0, n_actions)`; epsilon = epsilon_max unless an increment is given (:100);
* `train_neural_nets` (:448-515): uniform sampling with replacement; q_next AND q_eval4next
  from the target net as it stands, THEN the eval -> target copy every `replace_target_iter`
  learn steps (:508-510), then the update; both from the TARGET net (so the "double" argmax is the target's own: kept as written), no terminal mask,
  one Keras `train_on_batch` (MSE, RMSprop lr 0.01, rho 0.9, eps 1e-7 outside the sqrt,
  TF 2.1 optimizer_v2), then the epsilon update that may overshoot epsilon_max by one step;
* `compute_reward` (:409-446): per fill (1 - (fill - arrival)/arrival) * qty/q0 * 1e4 (BUY).

The environment is the rmsc03 + DummyRL GymKernel composition on the device (BASELINE.json
configs[3]; libmxa MXA_RMSC03_RL), which is a build-defined composition: the reference runs the
DDQN agent only inside a Kernel config (config/execution/marketreplay/execution_marketreplay_ddqn.py)
and never under ABIDESEnv. What the composition changes, and why:

* actions go through DummyRL's action vector [x, level-1 share, level-2 share] (dummy_rl:138-158,
  q/q0 == 1 by the reference's own quirk): `x = qty/q0` places exactly `qty`; allocation 1 ->
  (1, 0), 2 -> (0.5, 0.5), 3 -> (0.34, 0.66) (levels 2-3 merged: order_level is 2); allocation 0
  (a MARKET order in the reference) has no DummyRL counterpart and posts at the level-1 bid.
  The last step (remaining_time == 1) places the whole remaining quantity (:388-390);
* the reward of a step is the SUM of `compute_reward` over the step's fills, from the agent's
  cash and executed-quantity change (sum_i q_i (2 - f_i/A) = 2 dq + dcash/A for a BUY); the
  reference overwrites the experience reward per message (acceptance 0, execution r), an
  artefact of message order that a per-step environment cannot see;
* one learner serves every env (shared replay, one policy); `batch_size`, `train_every` and
  `updates_per_train` default to the reference's 32, 5 and 1.

Across GPUs (bench.py --gpus N, BASELINE configs[3]) the learner is synchronous data-parallel:
with `group` (a torch.distributed process group over RCCL) the eval and target nets start from
rank 0's initialisation (broadcast), every update all-reduces the live-weighted gradient and the
count of live ranks in one message, and every rank applies the same RMSprop step, so ONE policy
serves the whole node. Each rank samples its batch from its own envs' replay; the update equals
one learner's on the union of the LIVE ranks' batches (a rank whose envs are done, or whose replay
is below the batch size, contributes nothing; tests/test_ddqn_multirank.py). Every rank runs the
same collectives on every learn() call, whatever its replay size. The market
results of a given action sequence are world-size invariant (envs shard by global index,
mxabides.shard); the policy trajectory depends on the world size through that batch union.

Random streams: `gen` draws choose_action's exploration, `gen_sample` the batch indices and
`gen_drop` the dropout masks (Keras Dropout 0.1 in train_on_batch). A masked update (learn with
live false) still draws its batch and masks, so those two streams advance on it; the exploration
stream does not.

Everything runs on the device stream the env steps on; the only host read is the stored-transition
count, when the replay ring's host-side bounds cannot decide the batch-size test.
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

# ddqlearning_execution_agent.py:21-37
SIZE_ALLOCATION = {1: [1, 0, 0, 0], 2: [0.5, 0.5, 0, 0], 3: [0.34, 0.33, 0.33, 0]}
SIZE_SCALE = [0.1] + [i * 0.5 for i in range(1, 6)]


def _action_table():
    alloc = sorted(list(SIZE_ALLOCATION.keys()) + [0])
    acts, k = {}, 0
    for a in alloc:
        for s in SIZE_SCALE:
            acts[k] = (a, s)
            k += 1
    return acts


ACTIONS = _action_table()
N_ACTIONS = len(ACTIONS)  # 24 (execution_marketreplay_ddqn.py:244)
GRID_BINS = (200, 200)    # create_uniform_grid(low=[0, 0], high=[1, 1], bins=(200, 200)), :129

# DummyRL level shares per allocation type (levels >= 2 merged: order_level 2); 0 = MARKET -> level 1
LEVEL_SHARES = {0: (1.0, 0.0), 1: (1.0, 0.0), 2: (0.5, 0.5), 3: (0.34, 0.66)}


def create_uniform_grid(low, high, bins=(10, 10)):
    """agent/execution/util.py:5-22: interior split points per dimension."""
    return [np.linspace(low[d], high[d], bins[d] + 1)[1:-1] for d in range(len(bins))]


def discretize(sample, grid):
    """agent/execution/util.py:25-40: np.digitize per dimension (zip truncates to the grid)."""
    return list(int(np.digitize(s, g)) for s, g in zip(sample, grid))


# the observation row's columns (dummy_rl:294-315 and ABIDESEnvMetrics; mxa_kernels.hip rl_observe)
(OBS_TIME_REMAINING, OBS_QTY_REMAINING, OBS_LOG_RETURN, OBS_SPREAD, OBS_VOLUME_IMBALANCE, OBS_SMART_PRICE,
 OBS_VOLATILITY, OBS_TRADE_DIRECTION, OBS_EFFECTIVE_SPREAD) = range(9)
OBS_COLUMNS = 9
MAX_FEATURES = 8  # include/mxa_state_spec.h MXA_STATE_MAX_FEATURES
MAX_SPLIT_POINTS = 1 << 20  # MXA_STATE_MAX_POINTS, all features together


class Feature:
    """One element of the learner's state (include/mxa_state_spec.h): x = mul * (obs[col] / div) + add
    with a true division, then its bin on the feature's split points (np.digitize), or x itself when
    it has none (a continuous input).  The split points are either a uniform grid, `bins` bins over
    [low, high] as create_uniform_grid makes them (bins - 1 interior points), or `splits`, given
    explicitly and strictly increasing.  Everything is checked here, on the host."""

    def __init__(self, col, low=None, high=None, bins=0, splits=None, mul=1.0, div=1.0, add=0.0):
        if int(col) != col or not 0 <= int(col) < OBS_COLUMNS:
            raise ValueError("Feature: col %r is not an observation column 0..%d" % (col, OBS_COLUMNS - 1))
        self.col = int(col)
        self.mul, self.div, self.add = float(mul), float(div), float(add)
        if not math.isfinite(self.div) or self.div == 0.0:
            raise ValueError("Feature: div must be finite and nonzero, not %r" % (div,))
        if not math.isfinite(self.mul) or not math.isfinite(self.add):
            raise ValueError("Feature: mul and add must be finite")
        if splits is not None:
            if bins or low is not None or high is not None:
                raise ValueError("Feature: either splits or a uniform grid (low, high, bins), not both")
            pts = np.array(splits, dtype=np.float64).reshape(-1)
            if not np.isfinite(pts).all() or not (np.diff(pts) > 0).all():
                raise ValueError("Feature: splits must be finite and strictly increasing")
        elif bins:
            if int(bins) != bins or bins < 1 or low is None or high is None or not float(low) < float(high) \
                    or not (math.isfinite(low) and math.isfinite(high)):
                raise ValueError("Feature: a uniform grid needs bins >= 1 and finite low < high")
            pts = create_uniform_grid([float(low)], [float(high)], (int(bins),))[0]
        else:
            if low is not None or high is not None:
                raise ValueError("Feature: low and high without bins")
            pts = np.zeros(0)
        self.splits = np.ascontiguousarray(pts, dtype=np.float64)

    def __repr__(self):
        return "Feature(col=%d, %d split points, mul=%r, div=%r, add=%r)" % (self.col, len(self.splits), self.mul,
                                                                            self.div, self.add)


def default_features(quantity=100000, n_horizon=27):
    """ExecutionTask's own two-element state as features: 2 * (time / n_horizon) - 1 and
    2 * (quantity left / quantity) - 1 on the 200-bin grids over [0, 1]; bit for bit the states of
    ExecutionTask() (x * 2 + (-1.0) and x * 2 - 1.0 are one IEEE operation)"""
    return [Feature(OBS_TIME_REMAINING, 0.0, 1.0, GRID_BINS[0], mul=2.0, div=float(int(n_horizon)), add=-1.0),
            Feature(OBS_QTY_REMAINING, 0.0, 1.0, GRID_BINS[1], mul=2.0, div=float(quantity), add=-1.0)]


class QNet(nn.Module):
    """NNModel_1 / NNModel_2 (util/model/QNets.py:7-51) with Keras Dense defaults."""

    WIDTHS = {"NNModel_1": (32, 64, 128, 128, 64, 32), "NNModel_2": (32, 64, 128, 256, 128, 64, 32)}

    def __init__(self, n_in=2, n_actions=N_ACTIONS, model="NNModel_1", dropout=0.1, generator=None):
        super().__init__()
        w = self.WIDTHS[model]
        dims = (n_in,) + w
        self.hidden = nn.ModuleList(nn.Linear(dims[i], dims[i + 1]) for i in range(len(w)))
        self.logits = nn.Linear(w[-1], n_actions)
        self.p = dropout
        with torch.no_grad():
            for lin in list(self.hidden) + [self.logits]:  # glorot_uniform kernel, zero bias
                lim = math.sqrt(6.0 / (lin.in_features + lin.out_features))
                lin.weight.uniform_(-lim, lim, generator=generator)
                lin.bias.zero_()

    def dropout_widths(self):
        """the widths of the Dropout layers (after hidden layers 2..n, QNets.py:22-26)"""
        return [lin.out_features for lin in list(self.hidden)[1:]]

    def forward(self, x, masks=None):
        """masks: the keep masks (0/1, [batch, width]) of the dropout layers in training mode;
        kept units are scaled by 1 / (1 - rate) as Keras' Dropout does (TF 2.1 nn.dropout)"""
        for i, lin in enumerate(self.hidden):
            x = torch.relu(lin(x))
            if i >= 1 and self.p > 0 and self.training:  # dropout after layers 2..n (QNets.py:22-26)
                if masks is None:
                    x = nn.functional.dropout(x, self.p, True)
                else:
                    x = x * masks[i - 1].to(x.dtype) / (1.0 - self.p)
        return self.logits(x)


class ReplayRing:
    """Device-resident experience (s, a, s', r) of every env (the reference keeps one
    OrderedDict per agent, :115-116). Valid rows are compacted with a prefix sum, no host loop.

    The row count lives on the device (`n_dev`); the host keeps bounds on it (`n_lb`, `n_ub`) and
    reads it only when a size test cannot be decided from them, so the per-step loop does not
    wait for the GPU (in practice one read per training run)."""

    def __init__(self, capacity, n_state, device):
        self.cap = int(capacity)
        # one extra row: masked-out rows of a batched append are written there
        self.s = torch.zeros((self.cap + 1, n_state), dtype=torch.float32, device=device)
        self.s2 = torch.zeros_like(self.s)
        self.a = torch.zeros(self.cap + 1, dtype=torch.int64, device=device)
        self.r = torch.zeros(self.cap + 1, dtype=torch.float32, device=device)
        self.n_dev = torch.zeros((), dtype=torch.int64, device=device)  # rows written so far
        self.n_lb = 0  # host bounds on n_dev
        self.n_ub = 0

    def add_device(self, s, a, s2, r, mask):
        """append rows where mask without a host read; returns the count as a device scalar"""
        m = mask.to(torch.int64)
        c = torch.cumsum(m, 0)
        pos = torch.where(mask, (self.n_dev + c - 1) % self.cap, torch.full_like(c, self.cap))
        self.s[pos] = s.float()
        self.s2[pos] = s2.float()
        self.a[pos] = a
        self.r[pos] = r.float()
        k = c[-1] if len(c) else torch.zeros((), dtype=torch.int64, device=m.device)
        self.n_dev += k
        self.n_ub += len(mask)
        return k

    def add(self, s, a, s2, r, mask):
        """append rows where mask; returns the number appended (one host read)."""
        k = int(self.add_device(s, a, s2, r, mask).item())
        self.n_lb = int(self.n_dev.item())
        return k

    @property
    def n(self):
        return int(self.n_dev.item())

    def more_than(self, x):
        """len(self) > x, reading the device count only when the host bounds cannot decide"""
        if min(self.n_lb, self.cap) > x:
            return True
        if min(self.n_ub, self.cap) <= x:
            return False
        self.n_lb = int(self.n_dev.item())
        self.n_ub = max(self.n_ub, self.n_lb)
        return min(self.n_lb, self.cap) > x

    def __len__(self):
        return min(self.n, self.cap)


class DDQNLearner:
    """DDQLearningExecutionAgent's learner (ddqlearning_execution_agent.py:40-131, 333-362, 448-515).

    Eval and target parameters each live in one flat device buffer (`eflat`, `tflat`; the
    modules' parameters are views of it), so the target copy and the RMSprop step are single
    elementwise passes and every update can be masked on the device: `learn(live=...)` with a
    device bool makes the whole update (target copy, RMSprop step and its state, epsilon,
    `learn_step_counter`) a no-op when it is false, without a host read. The counter and epsilon
    are device scalars for the same reason.

    `fused_act` (include/mxa_ddqn.h mxa_qnet_*): every forward without a gradient (q_values, and so
    choose_action and act; q_target's target(s2) and eval(s)) runs in libmxa_ddqn.so's kernel,
    and choose_action / act make the forward, the argmax and the epsilon-greedy select one launch.
    The exploration draws are the same two torch calls, so the stream `gen` and every exploring
    env's action are unchanged; Q-values differ from hipBLASLt's in the last bits (another
    summation order). True needs a CUDA device, dtype float32 and the library, else RuntimeError;
    None (the default) turns it on only where the environment has MXA_DDQN_FUSED_ACT=1 and those
    three hold.

    `fused_learn` (include/mxa_ddqn_train.h): one learn_on update (the Q-target, train_on_batch's
    training-mode forward with the dropout masks, MSE, the backward pass, the masked target copy,
    the RMSprop step, epsilon and the counter) is two launches of libmxa_ddqn.so's kernels
    (mxa_qnet_train) instead of about a hundred on autograd; with a process group the gradient alone
    (mxa_qnet_grad), the live-weighted all-reduce as before, then mxa_qnet_update. The batch and the
    masks are drawn by the same torch calls, so `gen_sample` and `gen_drop` are unchanged; the
    Q-target has fused_act's bits, the gradient is another fp32 summation order of the same terms
    (each element one sum over the batch in index order, the same bits on every run), and the update
    has the bits of learn_on's own expressions on that gradient. Independent of fused_act. True
    needs what fused_act=True needs, and a batch size and net the kernels support (batch <= 256, at
    most 8 layers of at most 256 units), else RuntimeError; None turns it on only where the
    environment has MXA_DDQN_FUSED_LEARN=1 and all of that holds. Without it train_on_batch's
    gradient pass stays on autograd."""

    def __init__(self, n_state=2, n_actions=N_ACTIONS, replace_target_iter=5, batch_size=32, learning_rate=0.01,
                 epsilon_increment=None, epsilon_max=0.9, reward_decay=0.98, mode="train", model="NNModel_1",
                 dropout=0.1, capacity=1 << 20, device="cuda", seed=0, dtype=torch.float32, group=None,
                 fused_act=None, fused_learn=None):
        self.device = torch.device(device)
        self.dtype = dtype
        can_fuse = self.device.type == "cuda" and dtype == torch.float32 and lib() is not None
        if fused_act and not can_fuse:
            raise RuntimeError("DDQNLearner(fused_act=True) needs a CUDA device, dtype float32 and libmxa_ddqn.so "
                               "(build_lib.build_ddqn)")
        if fused_act is None:
            fused_act = os.environ.get("MXA_DDQN_FUSED_ACT") == "1" and can_fuse
        self.fused_act = bool(fused_act)
        if fused_learn and not can_fuse:
            raise RuntimeError("DDQNLearner(fused_learn=True) needs a CUDA device, dtype float32 and libmxa_ddqn.so "
                               "(build_lib.build_ddqn)")
        self.gen = torch.Generator(device=self.device)  # choose_action's exploration
        self.gen.manual_seed(seed)
        self.gen_sample = torch.Generator(device=self.device)  # train_neural_nets' batch indices
        self.gen_sample.manual_seed(seed + (1 << 20))
        self.gen_drop = torch.Generator(device=self.device)  # train_on_batch's dropout masks
        self.gen_drop.manual_seed(seed + (2 << 20))
        cpu = torch.Generator()
        cpu.manual_seed(seed)
        # EvalModel and TargetModel are two separately initialised Keras models (QNets.py:54-60):
        # two draws from the same generator, not a copy
        self.eval_model, self.eflat = self._flat(QNet(n_state, n_actions, model, dropout, cpu))
        self.target_model, self.tflat = self._flat(QNet(n_state, n_actions, model, dropout, cpu))
        self.n_actions = n_actions
        self.n_state = int(n_state)
        # the layer widths, as mxa_qnet_* take them (a host array)
        widths = [n_state] + [lin.out_features for lin in self.eval_model.hidden] + [n_actions]
        self._qdims = (ctypes.c_int * len(widths))(*widths)
        self.replace_target_iter = replace_target_iter
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.epsilon_increment = epsilon_increment
        self.epsilon_max = epsilon_max
        eps0 = 0.0 if epsilon_increment is not None else epsilon_max  # :100
        self._eps = torch.tensor(eps0, dtype=torch.float64, device=self.device)
        self.reward_decay = reward_decay
        self.mode = mode
        self._counter = torch.zeros((), dtype=torch.int64, device=self.device)
        # per learn() call: the loss and whether the update ran (device buffers, grown on the host
        # side: the call count is known without reading the device)
        self._cost = torch.zeros(256, dtype=torch.float64, device=self.device)
        self._cost_live = torch.zeros(256, dtype=torch.bool, device=self.device)
        self._ncost = 0
        # Keras RMSprop (TF 2.1 optimizer_v2, momentum 0, not centered): rho 0.9, epsilon 1e-7
        self.rho, self.rms_eps = 0.9, 1e-7
        self.rms = torch.zeros_like(self.eflat)
        self.memory = ReplayRing(capacity, n_state, self.device)
        # synchronous data parallelism over the ranks of `group` (module docstring)
        import torch.distributed as dist
        self.group = group
        self.world = dist.get_world_size(group) if group is not None else 1
        if self.world > 1:
            src = dist.get_global_rank(group, 0) if group is not dist.group.WORLD else 0
            dist.broadcast(self.eflat, src, group=group)
            dist.broadcast(self.tflat, src, group=group)
        # fused_learn: the kernels' workspace and the host array of mask pointers, made once
        ws_bytes = lib().mxa_qnet_train_workspace(batch_size, len(widths) - 1, self._qdims) if can_fuse else -1
        if fused_learn and ws_bytes < 0:
            raise RuntimeError("DDQNLearner(fused_learn=True): batch size %d or widths %s outside what mxa_qnet_train "
                               "supports (include/mxa_ddqn_train.h)" % (batch_size, widths))
        if fused_learn is None:
            fused_learn = os.environ.get("MXA_DDQN_FUSED_LEARN") == "1" and can_fuse and ws_bytes >= 0
        self.fused_learn = bool(fused_learn)
        if self.fused_learn:
            self._ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=self.device)
            self._mask_ptrs = (ctypes.c_void_p * max(1, len(widths) - 2))()
            if self.world > 1:
                self._grad = torch.empty_like(self.eflat)

    def _flat(self, net):
        net = net.to(self.device, self.dtype)
        params = list(net.parameters())
        flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
        off = 0
        for p in params:
            k = p.numel()
            p.data = flat[off:off + k].view_as(p)
            off += k
        return net, flat

    @property
    def learn_step_counter(self):
        return int(self._counter.item())

    @property
    def epsilon(self):
        return float(self._eps.item())

    @property
    def cost_hist(self):
        """the losses of the updates that ran (one host read; not on the step path)"""
        n = self._ncost
        c, live = self._cost[:n].cpu(), self._cost_live[:n].cpu()
        return [float(x) for x, ok in zip(c.tolist(), live.tolist()) if ok]

    def _record_cost(self, loss, live):
        if self._ncost == len(self._cost):
            self._cost = torch.cat([self._cost, torch.zeros_like(self._cost)])
            self._cost_live = torch.cat([self._cost_live, torch.zeros_like(self._cost_live)])
        self._cost[self._ncost] = loss.to(torch.float64)
        self._cost_live[self._ncost] = live
        self._ncost += 1

    def dropout_masks(self, n):
        """train_on_batch's dropout keep masks for a batch of n (Keras: keep where U >= rate)"""
        p = self.eval_model.p
        if p <= 0:
            return None
        return [torch.rand((n, w), generator=self.gen_drop, device=self.device, dtype=torch.float64) >= p
                for w in self.eval_model.dropout_widths()]

    # ---- acting (choose_action, :333-362)
    def _predict(self, net, flat, s):
        """Keras predict (training=False: no dropout, no gradient) of eval_model / eflat or
        target_model / tflat; with fused_act in one launch (mxa_qnet_forward)"""
        if not self.fused_act:
            net.eval()
            with torch.no_grad():
                return net(s.to(self.dtype))
        x = s.detach().to(torch.float32).contiguous()
        q = torch.empty((x.shape[0], self.n_actions), dtype=torch.float32, device=self.device)
        _call("mxa_qnet_forward", x.shape[0], x.data_ptr(), flat.data_ptr(), len(self._qdims) - 1, self._qdims,
              q.data_ptr())
        return q

    def q_values(self, s):
        return self._predict(self.eval_model, self.eflat, s)

    def _explore(self, n):
        """choose_action's exploration draws from `gen`: U [n] float64, the random actions [n],
        and whether the replay holds enough experience to exploit (len + 1 > batch_size)"""
        u = torch.rand(n, generator=self.gen, device=self.device, dtype=torch.float64)
        rnd = torch.randint(0, self.n_actions, (n,), generator=self.gen, device=self.device)
        return u, rnd, self.memory.more_than(self.batch_size - 1)

    def act(self, s, obs=None, task=None, out_a=None, out_act=None):
        """fused_act only: choose_action(s) and, with `obs` and `task`, ExecutionTask.actions of
        it, in one launch (mxa_qnet_act). Fills out_a [n] int64 and out_act [n, 3] float64 (made
        here when None) and returns them; without obs only the actions are made."""
        if not self.fused_act:
            raise RuntimeError("DDQNLearner.act needs fused_act")
        x = s.detach().to(torch.float32).contiguous()
        n = x.shape[0]
        test = self.mode == "test"
        if out_a is None:
            out_a = torch.empty(n, dtype=torch.int64, device=self.device)
        obs_w, obs_p, tab_p, act_p, q0 = 2, None, None, None, 1.0
        if obs is not None:
            _check_width(self, task)
            if out_act is None:
                out_act = torch.empty((n, 3), dtype=torch.float64, device=self.device)
            table = task.table
            if obs.dtype != torch.float64 or obs.dim() != 2 or obs.shape[0] != n or obs.shape[1] < 2 \
                    or not obs.is_contiguous():
                raise ValueError("act: obs must be a contiguous float64 [n, w >= 2] tensor")
            if table.dtype != torch.float64 or table.dim() != 2 or table.shape[0] < self.n_actions \
                    or table.shape[1] != 3 or not table.is_contiguous():
                raise ValueError("act: task.table must be a contiguous float64 [>= n_actions, 3] tensor")
            if out_act.dtype != torch.float64 or tuple(out_act.shape) != (n, 3) or not out_act.is_contiguous():
                raise ValueError("act: out_act must be a contiguous float64 [n, 3] tensor")
            obs_w, obs_p, tab_p, act_p, q0 = obs.shape[1], obs.data_ptr(), table.data_ptr(), out_act.data_ptr(), task.q0
        if out_a.dtype != torch.int64 or tuple(out_a.shape) != (n,) or not out_a.is_contiguous():
            raise ValueError("act: out_a must be a contiguous int64 [n] tensor")
        u, rnd, enough = (None, None, False) if test else self._explore(n)  # the unfused choose_action's draws
        _call("mxa_qnet_act", n, x.data_ptr(), self.eflat.data_ptr(), len(self._qdims) - 1, self._qdims, int(test),
              int(enough), None if test else u.data_ptr(), None if test else rnd.data_ptr(), self._eps.data_ptr(),
              obs_w, obs_p, tab_p, q0, out_a.data_ptr(), act_p, None)
        return out_a, out_act

    def policy(self, task, test, enough, u, rnd):
        """the mxa_policy POD (include/mxa.h) of the eval net as it stands, for
        VecABIDESEnv.step_policy_device: the flat parameters and widths, `task`'s grid, action table,
        horizon and quantity, epsilon, and choose_action's draws u / rnd ([k, n] float64 / int64
        device tensors; None in test mode). The tensors it points to stay referenced by the returned
        object, which the caller keeps until the launch is enqueued.  For a task with features the
        grid fields stay null (mxa_step_policy_spec does not read them): the state is `task.spec`,
        which the caller passes to step_policy_device beside this object."""
        from . import _lib
        if not self.fused_act:
            raise RuntimeError("DDQNLearner.policy needs fused_act (the in-kernel Q-values carry its bits)")
        _check_width(self, task)
        table = task.table.contiguous()
        grids = () if task.spec is not None else tuple(g.contiguous() for g in task.grid)
        for name, t, dt in tuple(("grid", g, torch.float64) for g in grids) + (("table", table, torch.float64),):
            if t.dtype != dt or t.device != self.eflat.device:
                raise ValueError("policy: task.%s must be a %s tensor on the learner's device" % (name, dt))
        if table.dim() != 2 or table.shape[0] < self.n_actions or table.shape[1] != 3:
            raise ValueError("policy: task.table must be a float64 [>= n_actions, 3] tensor")
        if not test:
            if u is None or rnd is None or u.dtype != torch.float64 or rnd.dtype != torch.int64 \
                    or not u.is_contiguous() or not rnd.is_contiguous():
                raise ValueError("policy: u / rnd must be contiguous float64 / int64 device tensors in train mode")
        p = _lib.Policy()
        p.params, p.n_layers = self.eflat.data_ptr(), len(self._qdims) - 1
        for i, w in enumerate(self._qdims):
            p.dims[i] = w
        if grids:
            g0, g1 = grids
            p.grid0, p.n0, p.grid1, p.n1 = g0.data_ptr(), g0.numel(), g1.data_ptr(), g1.numel()
        p.nh, p.q0, p.table = float(task.nh), float(task.q0), table.data_ptr()
        p.test, p.enough = int(bool(test)), int(bool(enough))
        p.u = None if test else u.data_ptr()
        p.rnd = None if test else rnd.data_ptr()
        p.eps = self._eps.data_ptr()
        p.keep = (self.eflat, grids, task.spec, table, u, rnd, self._eps)
        return p

    def choose_action(self, s):
        """s [n, n_state] -> actions [n] int64 (epsilon-greedy per env in train mode)."""
        if self.fused_act:
            return self.act(s)[0]
        greedy = torch.argmax(self.q_values(s), dim=1)
        if self.mode == "test":
            return greedy
        u, rnd, enough = self._explore(s.shape[0])
        return torch.where((u < self._eps) & enough, greedy, rnd)

    # ---- learning (train_neural_nets, :448-515)
    def q_target(self, s, a, s2, r):
        """the reference's target: both q_next and q_eval4next from the target net (:486-505)."""
        with torch.no_grad():
            q_next = self._predict(self.target_model, self.tflat, s2)
            # the reference's second forward of the target net; the kernel's result is bitwise the
            # same in any batch, so with fused_act it is computed once
            q_eval4next = q_next if self.fused_act else self._predict(self.target_model, self.tflat, s2)
            tgt = self._predict(self.eval_model, self.eflat, s)
            if not self.fused_act:
                tgt = tgt.clone()  # q_eval.copy() (:490); the kernel's output is a buffer of its own already
            idx = torch.arange(s.shape[0], device=self.device)
            best = torch.argmax(q_eval4next, dim=1)
            tgt[idx, a] = r.to(self.dtype) + self.reward_decay * q_next[idx, best]
        return tgt

    def learn_on(self, s, a, s2, r, live=None, masks=None):
        """one train_neural_nets update on a given batch, in the reference's order: the target
        from the target net as it stands (:486-505), THEN the eval -> target copy when
        learn_step_counter % replace_target_iter == 0 (:508-510), then train_on_batch (:513).
        `live` (device bool, default true) masks the whole update; `masks` are the dropout keep
        masks (default: drawn from gen_drop). With a process group the update is one learner's on
        the union of the LIVE ranks' batches: each rank's gradient is weighted by its own live
        flag and the sum is divided by the number of live ranks (one all-reduce carries both), so a
        rank whose envs are all done adds nothing from its stale replay; the update runs when any
        rank is live. Every rank issues the same collectives on every call. Returns the (local)
        loss."""
        if live is None:
            live = torch.ones((), dtype=torch.bool, device=self.device)
        local_live = live
        if masks is None:
            masks = self.dropout_masks(s.shape[0])
        if self.fused_learn:
            return self._learn_fused(s, a, s2, r, live, masks)
        tgt = self.q_target(s, a, s2, r)
        self.eval_model.train()  # train_on_batch: training=True (dropout active)
        for p in self.eval_model.parameters():
            p.grad = None
        loss = torch.mean((self.eval_model(s.to(self.dtype), masks) - tgt) ** 2)
        loss.backward()
        with torch.no_grad():
            g = torch.cat([p.grad.reshape(-1) for p in self.eval_model.parameters()])
            if self.world > 1:  # one policy for the node: the mean gradient over the live ranks
                import torch.distributed as dist
                w = local_live.to(g.dtype).reshape(1)
                gl = torch.cat([g * w, w])
                dist.all_reduce(gl, group=self.group)
                n_live = gl[-1]
                live = n_live > 0
                g = gl[:-1] / torch.clamp(n_live, min=1)
            # the target copy comes after the target (:508-510), before the RMSprop step; the
            # gradient above is the eval net's and does not read the target parameters after
            # q_target, so the copy can follow the all-reduce
            do_copy = live & (self._counter % self.replace_target_iter == 0)
            self.tflat.copy_(torch.where(do_copy, self.eflat, self.tflat))
            rms = self.rho * self.rms + (1 - self.rho) * g * g
            self.rms.copy_(torch.where(live, rms, self.rms))
            step = self.learning_rate * g / (torch.sqrt(self.rms) + self.rms_eps)
            self.eflat.sub_(torch.where(live, step, torch.zeros_like(step)))
            if self.epsilon_increment is not None:  # :515, may overshoot epsilon_max by one step
                e = torch.where(self._eps < self.epsilon_max, self._eps + self.epsilon_increment,
                                torch.full_like(self._eps, self.epsilon_max))
                self._eps.copy_(torch.where(live, e, self._eps))
            self._counter += live.to(torch.int64)
        for p in self.eval_model.parameters():
            p.grad = None
        loss = loss.detach()
        self._record_cost(loss, live)
        return loss

    def _learn_fused(self, s, a, s2, r, live, masks):
        """learn_on's update in libmxa_ddqn.so's kernels (include/mxa_ddqn_train.h): one
        mxa_qnet_train call; with a process group mxa_qnet_grad, the live-weighted all-reduce of
        learn_on, then mxa_qnet_update on the averaged gradient"""
        n = s.shape[0]
        if n != self.batch_size:
            raise RuntimeError("fused_learn: a batch of %d rows, the workspace is for batch_size %d" % (n, self.batch_size))
        s = s.detach().to(torch.float32).contiguous()
        s2 = s2.detach().to(torch.float32).contiguous()
        r = r.detach().to(torch.float32).contiguous()
        a = a.to(torch.int64).contiguous()
        live = live.to(torch.bool)
        keep = []  # the masks the pointers refer to stay referenced until the call is enqueued
        for h in range(len(self._mask_ptrs)):
            m = None if masks is None or h == 0 else masks[h - 1].to(torch.bool).contiguous()
            keep.append(m)
            self._mask_ptrs[h] = None if m is None else m.data_ptr()
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        has_inc = self.epsilon_increment is not None
        net = (len(self._qdims) - 1, self._qdims, self._mask_ptrs, float(self.eval_model.p), float(self.reward_decay),
               self._ws.data_ptr())
        upd = (self._counter.data_ptr(), int(self.replace_target_iter), self._eps.data_ptr(), int(has_inc),
               float(self.epsilon_increment) if has_inc else 0.0, float(self.epsilon_max), float(self.learning_rate),
               float(self.rho), float(self.rms_eps))
        if self.world == 1:
            _call("mxa_qnet_train", n, s.data_ptr(), a.data_ptr(), s2.data_ptr(), r.data_ptr(), self.eflat.data_ptr(),
                  self.tflat.data_ptr(), *net, None, loss.data_ptr(), None, self.rms.data_ptr(), live.data_ptr(), *upd)
        else:
            import torch.distributed as dist
            g = self._grad
            _call("mxa_qnet_grad", n, s.data_ptr(), a.data_ptr(), s2.data_ptr(), r.data_ptr(), self.eflat.data_ptr(),
                  self.tflat.data_ptr(), *net, g.data_ptr(), loss.data_ptr(), None)
            w = live.to(g.dtype).reshape(1)
            gl = torch.cat([g * w, w])
            dist.all_reduce(gl, group=self.group)
            n_live = gl[-1]
            live = n_live > 0
            g = (gl[:-1] / torch.clamp(n_live, min=1)).contiguous()
            _call("mxa_qnet_update", g.numel(), g.data_ptr(), self.eflat.data_ptr(), self.tflat.data_ptr(),
                  self.rms.data_ptr(), live.data_ptr(), *upd)
        self._record_cost(loss, live)
        return loss

    def learn(self, live=None):
        """sample a batch with replacement (np.random.choice(current_size, batch)) and update."""
        m = self.memory
        if self.world > 1:
            # the size test is per rank (its own envs' outcomes fill its replay), but the
            # collectives of learn_on must pair up on every rank: a rank below the batch size
            # still takes part, with its own update masked off (an empty replay samples row 0)
            ok = torch.clamp(m.n_dev, max=m.cap) > self.batch_size
            live = ok if live is None else (live & ok)
        elif not m.more_than(self.batch_size):
            return None
        size = torch.clamp(m.n_dev, max=m.cap).to(torch.float64)  # the current size, on the device
        u = torch.rand(self.batch_size, generator=self.gen_sample, device=self.device, dtype=torch.float64)
        idx = torch.clamp((u * size).to(torch.int64), max=m.cap - 1)
        return self.learn_on(m.s[idx], m.a[idx], m.s2[idx], m.r[idx], live=live)


class ExecutionTask:
    """Maps the rmsc03 + DummyRL env (obs float64[9], agent state) to the DDQN's state, action
    and reward (ddqlearning_execution_agent.py:301-331, 364-407, 409-446).

    obs[0] = remaining horizon steps, obs[1] = remaining quantity (dummy_rl:294-315); the
    horizon has `n_horizon` points; the parent order is `quantity` shares BUY.

    features (a list of 1..8 Feature): the state is those features of the observation row instead,
    `n_state` wide, so the policy can see the market columns (OBS_SPREAD, OBS_VOLUME_IMBALANCE, ...).
    `spec` is then the task's mxa_state_spec (_lib.StateSpec, its split points on `device`), which
    the kernels take (include/mxa_ddqn_features.h, mxa_policy_features.h), and `state` the same in
    PyTorch ops: the CPU and fused=False path, bit for bit the kernels'.  None: today's two-element
    state on today's code path (`spec` is None, `n_state` 2); default_features() is that state as
    a feature list."""

    def __init__(self, quantity=100000, n_horizon=27, device="cuda", features=None):
        self.q0 = float(quantity)
        self.nh = int(n_horizon)
        self.child = int(self.q0 / (self.nh - 1))  # generate_schedule: int(quantity / (len - 1))
        g = create_uniform_grid([0, 0], [1.0, 1.0], GRID_BINS)
        self.grid = [torch.tensor(x, dtype=torch.float64, device=device) for x in g]
        tab = np.zeros((N_ACTIONS, 3))
        for k, (alloc, scale) in ACTIONS.items():
            tab[k] = (max(0, round(scale * self.child)) / self.q0,) + LEVEL_SHARES[alloc]
        self.table = torch.tensor(tab, dtype=torch.float64, device=device)
        # the state's divisors as 0-dim device tensors: a tensor / tensor division is a true
        # division on every device, where tensor / Python scalar on a CUDA device multiplies by
        # the scalar's reciprocal and lands one bin off np.digitize at 73 of the quantities 0..1e5
        self._nh = torch.tensor(float(self.nh), dtype=torch.float64, device=device)
        self._q0 = torch.tensor(self.q0, dtype=torch.float64, device=device)
        self.features, self.spec, self.n_state = None, None, 2
        if features is not None:
            self._set_features(list(features), device)

    def _set_features(self, features, device):
        from . import _lib
        if not 1 <= len(features) <= MAX_FEATURES or not all(isinstance(f, Feature) for f in features):
            raise ValueError("ExecutionTask: features must be a list of 1..%d Feature" % MAX_FEATURES)
        if sum(len(f.splits) for f in features) > MAX_SPLIT_POINTS:
            raise ValueError("ExecutionTask: more than %d split points in all" % MAX_SPLIT_POINTS)
        self.features, self.n_state = features, len(features)
        # every feature's split points in one device array (the spec's `grid`); a feature's own are a view of it
        self._points = torch.tensor(np.concatenate([f.splits for f in features]), dtype=torch.float64, device=device)
        sp = _lib.StateSpec()
        sp.n_feat, off = len(features), 0
        self._fgrid, self._fdiv = [], []
        for i, f in enumerate(features):
            sp.col[i], sp.mul[i], sp.div[i], sp.add[i] = f.col, f.mul, f.div, f.add
            sp.goff[i] = off
            self._fgrid.append(self._points[off:off + len(f.splits)] if len(f.splits) else None)
            # 0-dim device tensors, for the same reason as _nh and _q0: tensor / tensor divides truly
            self._fdiv.append(torch.tensor(f.div, dtype=torch.float64, device=device))
            off += len(f.splits)
        for i in range(len(features), len(sp.goff)):
            sp.goff[i] = off
        sp.grid = self._points.data_ptr() if off else None
        sp.keep = self._points  # the struct points into it
        self.spec = sp

    def state(self, obs):
        """discretize([2*rem_t/len - 1, 2*rem_q/q0 - 1]) -> float [n, 2] bin indices; true
        divisions, as the reference's numpy (:307-308; oracle/ddqn_ref.state_ref).  With features:
        float [n, n_state], per feature mul * (obs[:, col] / div) + add, binned or cast."""
        if self.features is not None:
            cols = []
            for f, g, d in zip(self.features, self._fgrid, self._fdiv):
                x = f.mul * (obs[:, f.col] / d) + f.add
                cols.append(x if g is None else torch.bucketize(x, g, right=True))
            return torch.stack([c.to(torch.float32) for c in cols], 1)
        tr = 2 * (obs[:, 0] / self._nh) - 1
        qr = 2 * (obs[:, 1] / self._q0) - 1
        # np.digitize(x, increasing bins) == torch.bucketize(x, bins, right=True)
        return torch.stack([torch.bucketize(tr, self.grid[0], right=True),
                            torch.bucketize(qr, self.grid[1], right=True)], 1).to(torch.float32)

    def actions(self, a, obs):
        """DDQN action index -> DummyRL action vector [n, 3] float64 (take_action, :364-407)."""
        act = self.table[a].clone()
        last = obs[:, 0] == 1  # remaining_time == 1: the whole remaining quantity, allocation 0
        # x = qty / q0 by a Python scalar (on a CUDA device: qty * (1 / q0)); the engine places
        # rint(q0 * x) shares, the quantity itself either way (oracle/ddqn_ref.rint_of_share_is_exact)
        act[:, 0] = torch.where(last, obs[:, 1] / self.q0, act[:, 0])
        act[:, 1] = torch.where(last, torch.ones_like(act[:, 1]), act[:, 1])
        act[:, 2] = torch.where(last, torch.zeros_like(act[:, 2]), act[:, 2])
        return act

    @staticmethod
    def reward(prev, cur, arrival, q0):
        """sum over the step's fills of compute_reward (BUY): 1e4/q0 * (2 dq + dcash / A);
        prev/cur are mxa_write_rl_state rows (CASH, holdings, executed, ...)."""
        dq = cur[:, 2] - prev[:, 2]
        dcash = cur[:, 0] - prev[:, 0]
        return torch.where(dq > 0, 1e4 / q0 * (2 * dq + dcash / arrival), torch.zeros_like(dq))


_LIB = None


def lib():
    """libmxa_ddqn.so (include/mxa_ddqn.h, mxa_ddqn_train.h) as a ctypes.CDLL with every export's
    argtypes set: the per-period kernels of run_episode, the Q-network forward and epsilon-greedy
    action kernel of DDQNLearner(fused_act=True) and the update kernels of
    DDQNLearner(fused_learn=True); None when it is not built"""
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "libmxa_ddqn.so")
        if not os.path.exists(path):
            return None
        L = ctypes.CDLL(path)
        P, I, I64, D, DIMS = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.POINTER(ctypes.c_int)
        L.mxa_ddqn_period.argtypes = [P, I, I, I, I] + [P] * 13 + [P, I, P, I, D, D, D, P, P, P, P, I64, P, P]
        L.mxa_ddqn_state.argtypes = [P, I, I, P, P, I, P, I, D, D, P]
        L.mxa_ddqn_actions.argtypes = [P, I, I, P, P, P, D, P]
        L.mxa_qnet_forward.argtypes = [P, I, P, P, I, DIMS, P]
        L.mxa_qnet_act.argtypes = [P, I, P, P, I, DIMS, I, I, P, P, P, I, P, P, D, P, P, P]
        # include/mxa_ddqn_train.h
        MASKS = ctypes.POINTER(ctypes.c_void_p)
        batch = [P, I, P, P, P, P, P, P, I, DIMS, MASKS, D, D, P, P, P, P]
        update = [P, I, P, I, D, D, D, D, D]  # counter, iter, eps, has_inc, inc, eps_max, lr, rho, rms_eps
        L.mxa_qnet_train_workspace.argtypes = [I, I, DIMS]
        L.mxa_qnet_train_workspace.restype = I64
        L.mxa_qnet_grad.argtypes = batch
        L.mxa_qnet_update.argtypes = [P, I64, P, P, P, P, P] + update
        L.mxa_qnet_train.argtypes = batch + [P, P] + update
        _LIB = L
    return _LIB


_FEATURES_LIB = None


def features_lib():
    """libmxa_ddqn_features.so (include/mxa_ddqn_features.h) as a ctypes.CDLL with its exports'
    argtypes set: the per-period kernels for a task with features (ExecutionTask(features=...)). A
    library beside libmxa_ddqn.so, built with it (build_lib.build_ddqn); None when it is not built"""
    global _FEATURES_LIB
    if _FEATURES_LIB is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "libmxa_ddqn_features.so")
        if not os.path.exists(path):
            return None
        from ._lib import StateSpec
        L = ctypes.CDLL(path)
        P, I, I64, D, SPEC = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.POINTER(StateSpec)
        L.mxa_ddqn_state_spec.argtypes = [P, I, I, P, SPEC, P]
        L.mxa_ddqn_period_spec.argtypes = [P, I, I, I, I] + [P] * 13 + [SPEC, D, D, P, P, P, P, I64, P, P]
        _FEATURES_LIB = L
    return _FEATURES_LIB


period_lib = lib  # the name bench.py asks by
qnet_lib = lib  # the Q-network exports' loader by its earlier name, for callers that predate lib()


def _call(name, *args):
    """the export `name` of lib(), or of features_lib() for the *_spec kernels, on the current torch
    stream; a hipError_t raises, and so does a features library that is not built (no fall-back)"""
    L = lib()
    if name.endswith("_spec"):
        L = features_lib()
        if L is None:
            raise RuntimeError("%s: libmxa_ddqn_features.so is not built (build_lib.build_ddqn)" % name)
    rc = getattr(L, name)(torch.cuda.current_stream().cuda_stream, *args)
    if rc:
        raise RuntimeError("%s: hip error %d" % (name, rc))


def _check_width(learner, task):
    """a learner whose network is not as wide as the task's state is refused before any launch"""
    if learner.n_state != task.n_state:
        raise ValueError("DDQNLearner(n_state=%d) does not match the task's state of %d element(s)"
                         % (learner.n_state, task.n_state))


def _state_device(task, obs, out):
    if task.spec is not None:
        _call("mxa_ddqn_state_spec", obs.shape[0], obs.shape[1], obs.data_ptr(), ctypes.byref(task.spec), out.data_ptr())
        return out
    _call("mxa_ddqn_state", obs.shape[0], obs.shape[1], obs.data_ptr(), task.grid[0].data_ptr(), task.grid[0].numel(),
          task.grid[1].data_ptr(), task.grid[1].numel(), float(task.nh), task.q0, out.data_ptr())
    return out


def _act(learner, task, s, obs, out):
    """the period's actions a [n] and their action vectors [n, 3] (ExecutionTask.actions). `out` is
    the kernels' action-vector buffer; None: PyTorch ops, which make a new one"""
    if out is not None and learner.fused_act:  # forward, epsilon-greedy select and action vector in one launch
        return learner.act(s, obs, task, out_act=out)
    a = learner.choose_action(s)
    if out is None:
        return a, task.actions(a, obs)
    a = a.contiguous()
    _call("mxa_ddqn_actions", obs.shape[0], obs.shape[1], obs.data_ptr(), a.data_ptr(),
          task.table.contiguous().data_ptr(), task.q0, out.data_ptr())
    return a, out


def period_torch(task, m, train, obs, st, prev, arrival, flags, alive, s, a, env_steps, stored, r_row, spare=None):
    """One period's bookkeeping after the env step, as PyTorch ops: ok = alive & obs valid & no env
    error; the reward of the step's fills from the agent states `prev` and `st`; the next state
    s2; env_steps += alive; with `train` the ok envs' transitions (s, a, s2, r) appended to the
    replay ring `m` and counted in `stored`; r_row = where(ok, r, 0). Returns s2, the next alive
    mask and any(alive), the learner's update mask (the reference's agents stop training with their
    episode), all left on the device. `spare` is unused: period_kernel's output buffers."""
    ok = alive & ((flags & 2) != 0) & ((flags & 4) == 0)
    r = task.reward(prev, st, arrival, task.q0)
    s2 = task.state(obs)
    env_steps += alive.to(torch.int64)
    if train:
        stored += m.add_device(s, a, s2, r, ok)
    torch.where(ok, r, torch.zeros_like(r), out=r_row)
    return s2, ok & ((flags & 1) == 0), alive.any()


def period_kernel(task, m, train, obs, st, prev, arrival, flags, alive, s, a, env_steps, stored, r_row, spare):
    """period_torch in one launch (include/mxa_ddqn.h mxa_ddqn_period), bitwise the same; s2, the
    next alive mask and the update mask are written into the three buffers of `spare` and returned.
    The kernel refuses a training batch of more envs than the replay capacity."""
    s2, alive_next, live = spare
    n = obs.shape[0]
    if task.spec is not None:  # include/mxa_ddqn_features.h: the rows of s, s2 and the ring are n_state wide
        _call("mxa_ddqn_period_spec", n, obs.shape[1], st.shape[1], int(train), obs.data_ptr(), st.data_ptr(),
              prev.data_ptr(), arrival.data_ptr(), flags.data_ptr(), alive.data_ptr(), alive_next.data_ptr(),
              live.data_ptr(), s.data_ptr(), a.data_ptr(), s2.data_ptr(), r_row.data_ptr(), env_steps.data_ptr(),
              ctypes.byref(task.spec), task.q0, 1e4 / task.q0, m.s.data_ptr(), m.s2.data_ptr(), m.a.data_ptr(),
              m.r.data_ptr(), m.cap, m.n_dev.data_ptr(), stored.data_ptr())
        if train:
            m.n_ub += n
        return spare
    g0, g1 = task.grid
    _call("mxa_ddqn_period", n, obs.shape[1], st.shape[1], int(train), obs.data_ptr(), st.data_ptr(), prev.data_ptr(),
          arrival.data_ptr(), flags.data_ptr(), alive.data_ptr(), alive_next.data_ptr(), live.data_ptr(), s.data_ptr(),
          a.data_ptr(), s2.data_ptr(), r_row.data_ptr(), env_steps.data_ptr(), g0.data_ptr(), g0.numel(), g1.data_ptr(),
          g1.numel(), float(task.nh), task.q0, 1e4 / task.q0, m.s.data_ptr(), m.s2.data_ptr(), m.a.data_ptr(),
          m.r.data_ptr(), m.cap, m.n_dev.data_ptr(), stored.data_ptr())
    if train:
        m.n_ub += n
    return spare


def rollout_chunks(nh=27, train_every=5, train=True):
    """The launches of one closed-loop episode (run_episode(rollout=True)) as (first_zero, n_steps)
    pairs: the episode is the zero step and the periods t = 0 .. nh-1, nh + 1 steps in all. When
    training, a launch ends after every period t with t % train_every == 0, where the learner
    updates the net the next period acts with; otherwise the episode is one launch. Only the first
    launch holds the zero step."""
    if not train:
        return [(True, nh + 1)]
    chunks, n = [], 1
    for t in range(nh):
        n += 1
        if t % train_every == 0:
            chunks.append((not chunks, n))
            n = 0
    if n:
        chunks.append((not chunks, n))
    return chunks


def _run_rollout(env, learner, task, train_every, updates_per_train, record, timing):
    """run_episode's loop with the policy inside the step kernel (include/mxa.h mxa_step_policy):
    per launch the exploration draws of its periods, the launch, then period_kernel per period on
    the recorded rows and the learner's update where run_episode's loop has it"""
    from .gym import OBS_SIZE, RL_STATE_WORDS
    dev, n, nh = learner.device, env.n_envs, task.nh
    train, test = learner.mode == "train", learner.mode == "test"
    K = nh + 1  # row 0: the zero step; row t + 1: period t
    obs = torch.zeros((K, n, OBS_SIZE), dtype=torch.float64, device=dev)
    flags = torch.zeros((K, n), dtype=torch.int32, device=dev)
    st = torch.zeros((K, n, RL_STATE_WORDS), dtype=torch.float64, device=dev)
    a_idx = torch.zeros((K, n), dtype=torch.int64, device=dev)
    act = torch.zeros((K, n, 3), dtype=torch.float64, device=dev)
    u = rnd = None
    if not test:
        u = torch.zeros((K, n), dtype=torch.float64, device=dev)
        rnd = torch.zeros((K, n), dtype=torch.int64, device=dev)
    rw = torch.zeros((nh, n), dtype=torch.float64, device=dev)
    stored = torch.zeros((), dtype=torch.int64, device=dev)
    ctx = {}

    def launch(r0, k, first_zero, enough):
        for r in range(r0 + (1 if first_zero else 0), r0 + k):  # _explore's draws, in its order
            if not test:
                u[r] = torch.rand(n, generator=learner.gen, device=dev, dtype=torch.float64)
                rnd[r] = torch.randint(0, learner.n_actions, (n,), generator=learner.gen, device=dev)
        pol = learner.policy(task, test, enough, None if test else u[r0:], None if test else rnd[r0:])
        if timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        env.step_policy_device(k, pol, obs[r0].data_ptr(), flags[r0].data_ptr(), a_idx[r0].data_ptr(),
                               act[r0].data_ptr(), st[r0].data_ptr(), first_zero=first_zero, spec=task.spec)
        if timing is not None:
            e1.record()
            timing.append((e0, e1))
        if record is not None:
            record.extend(act[r].clone() for r in range(r0, r0 + k))
        for r in range(r0, r0 + k):
            if r == 0:  # after the zero step, as run_episode
                ctx["alive"] = ((flags[0] & 2) != 0) & ((flags[0] & 5) == 0)
                lob_ok = (st[0][:, 7] == 3)
                ctx["arrival"] = torch.where(lob_ok, (st[0][:, 3] + st[0][:, 4]) / 2,
                                             torch.ones_like(st[0][:, 3])).contiguous()
                ctx["env_steps"] = ctx["alive"].to(torch.int64)
                ctx["s"] = _state_device(task, obs[0], torch.empty((n, task.n_state), dtype=torch.float32, device=dev))
                ctx["spare"] = (torch.empty_like(ctx["s"]), torch.zeros_like(ctx["alive"]),
                                torch.zeros((), dtype=torch.bool, device=dev))
                continue
            t = r - 1
            s2, alive_next, live = period_kernel(task, learner.memory, train, obs[r], st[r], st[r - 1], ctx["arrival"],
                                                 flags[r], ctx["alive"], ctx["s"], a_idx[r], ctx["env_steps"], stored,
                                                 rw[t], ctx["spare"])
            if train and t % train_every == 0:
                for _ in range(updates_per_train):
                    learner.learn(live=live)
            ctx["s"], ctx["alive"], ctx["spare"] = s2, alive_next, (ctx["s"], ctx["alive"], live)

    def enough_now():
        return test or learner.memory.more_than(learner.batch_size - 1)

    r0 = 0
    for first_zero, k in rollout_chunks(nh, train_every, train):
        end = r0 + k
        # `enough` is one value per launch: until the replay holds a batch (it only grows), one
        # step per launch, each period with choose_action's own test before it
        while r0 < end:
            enough = enough_now()
            kk = end - r0 if enough else 1
            launch(r0, kk, first_zero and r0 == 0, enough)
            r0 += kk
    return {"rewards": rw if nh else None, "actions": a_idx[1:].clone() if nh else None, "returns": rw.sum(0),
            "flags": flags[K - 1], "arrival": ctx["arrival"], "stored": stored, "env_steps": ctx["env_steps"],
            "steps": nh + 1}


def run_episode(env, learner, task, seeds=None, train_every=5, updates_per_train=1, record=None, timing=None,
                fused=None, rollout=None):
    """One episode of every env of a VecABIDESEnv (rmsc03 + DummyRL) driven by the learner, all on
    the current torch stream (the env must step on it: env.set_stream). Mirrors the agent's
    per-period loop (place_order, :275-299): observe, choose, act, then store the completed
    transition and train every `train_every` periods (train_step_counter % 5 == 0, :286-293).
    Every horizon step is enqueued without waiting for the GPU: envs that are done stay done in the
    step kernel, their rows are masked out, and an update once every env is done is a masked no-op.

    fused (default: a learner on the GPU with libmxa_ddqn.so built): the action vectors and the
    bookkeeping after each step in one kernel each (period_kernel), bitwise the same as the PyTorch
    ops that fused=False runs (period_torch; tests/test_gpu_ddqn.py; 59.9 -> 55.8 ms per
    rmsc03_ddqn x4096 episode on one box); both equal the plain float64 references of
    oracle/ddqn_ref.py (tests/test_gpu_ddqn_kernels.py, tests/test_ddqn_episode.py).

    Returns a dict of device tensors (rewards [steps, n], actions [steps, n], flags) and the
    number of stored transitions. `record` (a list) receives the per-step action vectors;
    `timing` (a list) receives a (start, end) torch.cuda.Event pair around every step launch.

    rollout: the policy inside the step kernel (include/mxa.h mxa_step_policy): the launches of
    rollout_chunks, each running its periods of every env with the epsilon-greedy Q-network policy
    evaluated in place, so an env does not wait for the slowest env of every step; the exploration
    draws, period_kernel and the learner's updates are the same calls in the same order, and the
    returned dict, the replay ring, the learner and the env blocks are bitwise those of
    rollout=False. True needs the kernel path (fused not False), a CUDA learner with fused_act (the
    in-kernel Q-values carry fused_act's bits) and both libraries, else RuntimeError; None (the
    default) turns it on only where the environment has MXA_DDQN_ROLLOUT=1 and all of that holds.
    Until the replay holds a batch (choose_action's `enough`), a launch runs one period."""
    from .gym import OBS_SIZE, RL_STATE_WORDS
    _check_width(learner, task)
    kernel = fused is not False and learner.device.type == "cuda" and lib() is not None
    if fused and not kernel:
        raise RuntimeError("run_episode(fused=True): libmxa_ddqn.so is not built (build_lib.build_ddqn)")
    can_roll = kernel and learner.fused_act and hasattr(env.L, "mxa_step_policy" if task.spec is None
                                                        else "mxa_step_policy_spec")
    if rollout and not can_roll:
        raise RuntimeError("run_episode(rollout=True) needs the kernel path (fused not False), a CUDA learner with "
                           "fused_act, libmxa_ddqn.so and a libmxa.so with mxa_step_policy")
    if rollout is None:
        rollout = os.environ.get("MXA_DDQN_ROLLOUT") == "1" and can_roll
    if rollout:
        env.reset(seeds=seeds)
        return _run_rollout(env, learner, task, train_every, updates_per_train, record, timing)
    period = period_kernel if kernel else period_torch
    dev, n, nh = learner.device, env.n_envs, task.nh
    env.reset(seeds=seeds)
    obs = torch.zeros((n, OBS_SIZE), dtype=torch.float64, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.zeros((n, RL_STATE_WORDS), dtype=torch.float64, device=dev)
    prev = torch.zeros_like(st)
    act0 = torch.zeros((n, 3), dtype=torch.float64, device=dev)  # first step: no cached LOB, nothing placed
    env.step_device(act0.data_ptr(), obs.data_ptr(), flags.data_ptr())
    env.write_rl_state(st.data_ptr())
    if record is not None:
        record.append(act0.clone())
    alive = ((flags & 2) != 0) & ((flags & 5) == 0)
    lob_ok = (st[:, 7] == 3)
    arrival = torch.where(lob_ok, (st[:, 3] + st[:, 4]) / 2, torch.ones_like(st[:, 3])).contiguous()  # mid at start_time
    rw = torch.zeros((nh, n), dtype=torch.float64, device=dev)
    actions = []
    stored = torch.zeros((), dtype=torch.int64, device=dev)
    env_steps = alive.to(torch.int64)  # per env: ABIDESEnv.step calls taken while alive (the first one included)
    if kernel:  # the kernels fill preallocated buffers: the action vectors, and (s2, alive_next, live)
        s = _state_device(task, obs, torch.empty((n, task.n_state), dtype=torch.float32, device=dev))
        out = torch.empty((n, 3), dtype=torch.float64, device=dev)
        spare = (torch.empty_like(s), torch.zeros_like(alive), torch.zeros((), dtype=torch.bool, device=dev))
    else:
        s, out, spare = task.state(obs), None, None
    train = learner.mode == "train"
    for t in range(nh):
        a, act = _act(learner, task, s, obs, out)
        if record is not None:
            record.append(act.clone())
        st, prev = prev, st  # write_rl_state fills the other buffer: prev keeps the state before the step
        if timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        env.step_device(act.data_ptr(), obs.data_ptr(), flags.data_ptr())
        if timing is not None:
            e1.record()
            timing.append((e0, e1))
        env.write_rl_state(st.data_ptr())
        s2, alive_next, live = period(task, learner.memory, train, obs, st, prev, arrival, flags, alive, s, a,
                                      env_steps, stored, rw[t], spare)
        if train and t % train_every == 0:
            for _ in range(updates_per_train):
                learner.learn(live=live)
        actions.append(a)
        s, alive, spare = s2, alive_next, (s, alive, live)  # the buffers of the period before are free again
    return {"rewards": rw if nh else None, "actions": torch.stack(actions) if actions else None,
            "returns": rw.sum(0), "flags": flags, "arrival": arrival, "stored": stored, "env_steps": env_steps,
            "steps": nh + 1}
