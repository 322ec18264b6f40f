"""Shared by tests/test_ddqn_kernel_refs.py (CPU) and tests/test_gpu_ddqn_kernels.py (GPU): seeded
synthetic inputs of one learner period (include/mxa_ddqn.h mxa_ddqn_period), and the same period
as this project's PyTorch ops (ExecutionTask.state / .reward, ReplayRing.add_device, alive.any())
on any device; the sentinel-guarded device buffers of the GPU tests. The expected values come from
oracle/ddqn_ref.py, never from here."""
import numpy as np
import torch

from mxabides import ddqn

OK_PATTERNS = ("all", "none", "half", "lane63", "lane0", "env1024", "last")
DEFAULT_GRID = ddqn.create_uniform_grid([0, 0], [1.0, 1.0], ddqn.GRID_BINS)
# an irregular grid of 7 split points with a repeated one, for the time axis
IRREGULAR_G0 = np.array([-0.9, -0.5, -0.5, -0.1, 0.0, 0.3, 0.99])
# the nets of the Q-net kernel's exact tests: (widths, nonzero weights per neuron or None for
# dense, seed). Seed 3, but 4 for the net with the 1-wide layer: with 3 that unit is 0 for every
# input and all rows come out equal
INTEGER_NETS = [((256, 256, 24), None, 3), ((255, 256, 65, 24), None, 3),
                ((4, 12, 65, 129, 256, 256, 255, 64, 1), 16, 3), ((256,) * 9, 16, 3), ((1, 63, 64, 1, 256, 7), 16, 4)]

PAD = 3  # sentinel rows before and after every buffer
SENTINEL = {np.dtype(np.float64): -77777.25, np.dtype(np.float32): -77777.25, np.dtype(np.int64): -7777777,
            np.dtype(np.int32): -7777777, np.dtype(np.uint8): 0xA5}


class Guarded:
    """a device buffer holding `arr` between PAD sentinel rows"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.bool_:
            arr = arr.astype(np.uint8)
        if arr.ndim == 0:
            arr = arr.reshape(1)
        self.n = len(arr)
        full = np.full((self.n + 2 * PAD,) + arr.shape[1:], SENTINEL[arr.dtype], dtype=arr.dtype)
        full[PAD:PAD + self.n] = arr
        self.full = torch.from_numpy(full).cuda()
        self.ptr = self.full[PAD:].data_ptr()

    def read(self, what):
        """the rows, after checking the sentinels around them"""
        full = self.full.cpu().numpy()
        s = SENTINEL[full.dtype]
        assert np.all(full[:PAD] == s) and np.all(full[PAD + self.n:] == s), "%s: sentinel rows overwritten" % (what,)
        return full[PAD:PAD + self.n]


def same(a, b):
    """exact equality: dtype, shape and every bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ok_mask(pattern, n, rs):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "half":
        return rs.rand(n) < 0.5
    if pattern == "lane63":
        return i % 64 == 63
    if pattern == "lane0":
        return i % 64 == 0
    if pattern == "env1024":
        return i == 1024
    if pattern == "last":
        return i == n - 1
    raise ValueError(pattern)


def make_case(n, seed, ok="half", obs_w=9, st_w=8, cap=2200, n_dev=0, stored=1000, g0=None, g1=None, nh=27, q0=1e5,
              q0_reward=None, train=1):
    """numpy inputs of one mxa_ddqn_period call. Envs that are to be ok are alive with flag bit 1
    set and bit 2 clear; every other env is, at random, dead (NaN in st, prev and arrival, any flag
    bits) or alive with one of the six combinations of bits 0..2 that are not ok. Flag bits 3..31
    are junk (so some flags are negative), bit 0 (done) is random. The reward inputs cover dq > 0,
    dq <= 0, dq NaN and an arrival of 0 with dq > 0. rscale is 1e4 / q0_reward (default q0), as ExecutionTask.reward."""
    rs = np.random.RandomState(seed)
    want = ok_mask(ok, n, rs)
    alive = want | (rs.rand(n) < 0.6)
    f = np.where(want, rs.choice([2, 3], n), np.where(alive, rs.choice([0, 1, 4, 5, 6, 7], n), rs.randint(0, 8, n)))
    f |= rs.randint(0, 1 << 29, n) << 3
    flags = (f & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    obs = rs.rand(n, obs_w) * 1000 - 500
    obs[:, 0] = rs.randint(0, int(nh) + 1, n)
    obs[:, 1] = rs.randint(0, int(q0) + 1, n)
    prev = rs.rand(n, st_w) * 1e6 - 5e5
    st = rs.rand(n, st_w) * 1e6 - 5e5
    prev[:, 2] = rs.randint(0, 50000, n)
    prev[:, 0] = -rs.randint(0, 10 ** 9, n).astype(np.float64)
    dq = rs.randint(-3, 4000, n).astype(np.float64)
    dq[rs.rand(n) < 0.2] = 0.0
    st[:, 2] = prev[:, 2] + dq
    st[:, 0] = prev[:, 0] - dq * rs.randint(99000, 101000, n)
    arrival = 100000.0 + rs.randint(-2000, 2000, n) / 2.0
    nan_dq = rs.rand(n) < 0.05
    st[nan_dq, 2] = np.nan
    arrival[(rs.rand(n) < 0.05) & (dq > 0)] = 0.0
    dead = ~alive
    st[dead], prev[dead], arrival[dead] = np.nan, np.nan, np.nan
    g0 = DEFAULT_GRID[0] if g0 is None else np.asarray(g0, dtype=np.float64)
    g1 = DEFAULT_GRID[1] if g1 is None else np.asarray(g1, dtype=np.float64)
    return {
        "n": n, "obs_w": obs_w, "st_w": st_w, "train": train, "obs": obs, "st": st, "prev": prev, "arrival": arrival,
        "flags": flags, "alive": alive, "s": rs.randint(0, 200, (n, 2)).astype(np.float32),
        "a": rs.randint(-5, 1 << 40, n).astype(np.int64), "env_steps": rs.randint(0, 28, n).astype(np.int64),
        "g0": g0, "n0": len(g0), "g1": g1, "n1": len(g1), "nh": float(nh), "q0": float(q0),
        "q0_reward": float(q0 if q0_reward is None else q0_reward),
        "rscale": 1e4 / float(q0 if q0_reward is None else q0_reward),
        "ring_s": rs.randint(0, 200, (cap + 1, 2)).astype(np.float32),
        "ring_s2": rs.randint(0, 200, (cap + 1, 2)).astype(np.float32),
        "ring_a": rs.randint(0, 24, cap + 1).astype(np.int64), "ring_r": rs.normal(0, 50, cap + 1).astype(np.float32),
        "cap": cap, "n_dev": int(n_dev), "stored": int(stored), "want_ok": want,
    }


REF_ARGS = ("n", "obs_w", "st_w", "train", "obs", "st", "prev", "arrival", "flags", "alive", "s", "a", "env_steps", "g0",
            "n0", "g1", "n1", "nh", "q0", "rscale", "ring_s", "ring_s2", "ring_a", "ring_r", "cap", "n_dev", "stored")
OUTPUTS = ("alive_next", "live", "s2", "r_row", "env_steps", "ring_s", "ring_s2", "ring_a", "ring_r", "n_dev", "stored")


def reference(c):
    import ddqn_ref
    return ddqn_ref.period_ref(*[c[k] for k in REF_ARGS])


def chain(c, out, seed):
    """the next period's inputs after `out`: its ring, counts, alive mask and state carried over,
    fresh observations, agent states and flags"""
    nxt = make_case(c["n"], seed, "half", c["obs_w"], c["st_w"], c["cap"], out["n_dev"], out["stored"], c["g0"], c["g1"],
                    c["nh"], c["q0"], c["q0_reward"], c["train"])
    for k in ("ring_s", "ring_s2", "ring_a", "ring_r", "env_steps"):
        nxt[k] = np.array(out[k])
    nxt["s"] = np.array(out["s2"])
    nxt["alive"] = np.array(out["alive_next"])
    return nxt


def make_task(c, device):
    """an ExecutionTask with the case's grid, horizon and quantity"""
    task = ddqn.ExecutionTask(quantity=c["q0"], n_horizon=int(c["nh"]), device=device)
    task.grid = [torch.tensor(c["g0"], dtype=torch.float64, device=device),
                 torch.tensor(c["g1"], dtype=torch.float64, device=device)]
    return task


def torch_period(c, device):
    """the period as run_episode's PyTorch ops (mxabides.ddqn.period_torch) on `device`; returns
    the outputs as numpy. The ring's spare row `cap` takes the masked-out rows of
    ReplayRing.add_device here, so it is returned but not comparable with the kernel's."""
    dv = lambda k: torch.from_numpy(np.ascontiguousarray(c[k])).to(device)
    task = make_task(c, device)
    task.q0 = c["q0_reward"]  # the reward's scale alone: the state divides by the tensor task._q0
    assert float(task._q0) == c["q0"], "ExecutionTask.state no longer has a quantity of its own"
    obs, st, prev, arrival, flags, alive = (dv(k).reshape(np.shape(c[k])) for k in
                                            ("obs", "st", "prev", "arrival", "flags", "alive"))
    s, a, env_steps = dv("s"), dv("a"), dv("env_steps").clone()
    m = ddqn.ReplayRing(c["cap"], 2, device)
    m.s, m.s2, m.a, m.r = dv("ring_s").clone(), dv("ring_s2").clone(), dv("ring_a").clone(), dv("ring_r").clone()
    m.n_dev = torch.tensor(c["n_dev"], dtype=torch.int64, device=device)
    stored = torch.tensor(c["stored"], dtype=torch.int64, device=device)
    r_row = torch.empty(c["n"], dtype=torch.float64, device=device)
    s2, alive_next, live = ddqn.period_torch(task, m, c["train"], obs, st, prev, arrival, flags, alive, s, a, env_steps,
                                             stored, r_row)
    out = {"alive_next": alive_next, "live": live, "s2": s2, "r_row": r_row, "env_steps": env_steps, "ring_s": m.s,
           "ring_s2": m.s2, "ring_a": m.a, "ring_r": m.r, "n_dev": m.n_dev, "stored": stored}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("live", "n_dev", "stored"):
        out[k] = out[k].item()
    return out


def assert_outputs_equal(got, ref, what, ring_rows=None):
    """every output exactly; ring_rows limits the ring arrays to their first rows (torch_period)"""
    for k in OUTPUTS:
        g, r = got[k], ref[k]
        if k in ("live", "n_dev", "stored"):
            assert int(g) == int(r), (what, k, g, r)
            continue
        if k.startswith("ring_") and ring_rows is not None:
            g, r = g[:ring_rows], r[:ring_rows]
        if not same(g, r):
            bad = np.flatnonzero((np.asarray(g).reshape(len(g), -1) != np.asarray(r).reshape(len(r), -1)).any(1))
            raise AssertionError("%s: %s differs at %d rows, first %s: %s != %s"
                                 % (what, k, len(bad), bad[:5], np.asarray(g)[bad[:3]], np.asarray(r)[bad[:3]]))
