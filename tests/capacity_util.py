"""The tight compositions tests/golden/cap_*.json (gen_capacity_fixtures.py) and their seed pools,
classified by the oracle: shared by test_capacity_edges.py (CPU) and test_gpu_capacity_edges.py."""
import functools
import json
import os

import numpy as np

import pyoracle
from golden_util import GOLDEN

# name -> (pool size, the resources whose capacity the pool's peaks straddle: "q" pending events,
# "b" resting orders)
POOLS = {"cap_zi95_q": (2048, "q"), "cap_zi95_b": (2048, "b"), "cap_zi95_qb": (2048, "qb"),
         "cap_zi384_q": (512, "q"), "cap_zi767_q": (512, "q"), "cap_rmsc03_q": (2048, "q")}
# the oracle's fail() codes of ora_set_capacities / ora_set_open_capacity -> the device's
# ERR_QUEUE_FULL / ERR_BOOK_FULL / ERR_OPEN_FULL
ORACLE_TO_DEVICE = {pyoracle.ERR_QUEUE_FULL: 1, pyoracle.ERR_BOOK_FULL: 2, pyoracle.ERR_OPEN_FULL: 3}
THREADS = min(16, os.cpu_count() or 1)


def pool(n):
    return ((np.arange(n, dtype=np.int64) * 7919 + 3) & 0xFFFFFFFF).astype(np.uint32)


def load(name):
    """the fixture's composition as an oracle config (the bytes of mxabides' MarketConfig)"""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        d = json.load(f)["composition"]
    c = pyoracle.OraConfig()
    for k, _ in pyoracle.OraConfig._fields_:
        v = d[k]
        if k == "mm":
            for n, _ in c.mm._fields_:
                setattr(c.mm, n, v[n])
        elif k in ("zi_count", "zi_r_min", "zi_r_max", "zi_eta"):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


class Pool:
    """one composition's pool under the oracle: `peak` [n][2] (pending, resting) of the run without
    capacities, (events, hash) of that run, and (events, hash, err) of the run with the capacities
    `cap` = (q, b).  margin[i]: how far seed i's peak lies over the capacity, the larger of the
    tight resources' (0: ends exactly full, 1: needs one slot more)."""

    def __init__(self, name, cap):
        n, tight = POOLS[name]
        self.name, self.cap, self.tight = name, cap, tight
        self.cfg = load(name)
        self.seeds = pool(n)
        self.ev, self.hs, er, _, st = pyoracle.run_batch_config(self.cfg, self.seeds, THREADS, stats=True)
        assert (er == 0).all()
        self.peak = st[:, :2]
        self.cev, self.chs, self.cer, _ = pyoracle.run_batch_config(self.cfg, self.seeds, THREADS, capacities=cap)
        over = [self.peak[:, i] - cap[i] for i, r in enumerate("qb") if r in tight]
        self.margin = np.max(over, axis=0)

    def index(self, seeds):
        pos = {int(s): i for i, s in enumerate(self.seeds)}
        return np.array([pos[int(s)] for s in seeds], dtype=np.int64)

    def batch(self):
        """the mixed batch: every seed whose peak lies within capacity - 1 .. capacity + 2 (at most
        64 per class), 32 well below and 32 well above where the pool has them, interleaved in pool
        order so that overflowing envs sit next to passing ones"""
        take = []
        for k in (-1, 0, 1, 2):
            take += np.nonzero(self.margin == k)[0][:64].tolist()
        take += np.nonzero(self.margin < -1)[0][:32].tolist()
        take += np.nonzero(self.margin > 2)[0][:32].tolist()
        return np.array(sorted(take), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def classified(name, cap):
    return Pool(name, cap)
