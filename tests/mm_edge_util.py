"""The option edges of config/rmsc03.py's POV market maker on the per-env options engine
(include/mxa.h mxa_create_params): the case table, the mixed batch and its oracle runs, shared by
test_mm_option_edges.py (CPU) and test_gpu_mm_option_edges.py.

Every row is a set of --mm-* options at a branch boundary of mm_requote / mm_place_ladder
(csrc/mxa_kernels.hip): the ladder is placed in batched passes of 64 up to 128 orders (63 ticks)
and order by order beyond, or when the order size is 0; the open-order list holds 256 entries, so
two 128-order ladders (the old one still being cancelled) fill it exactly."""
import functools
import os

import numpy as np

import pyoracle
from mxabides.configs import MM_DEFAULTS, mm_params

# the device's capacities of MXA_RMSC03_MM (include/mxa.h): pending events, resting orders, open
# orders per agent
CAP = (320, 192, 256)
SEEDS = [30, 31, 32, 33, 1000, 1001, 1002, 1003]
THREADS = min(16, os.cpu_count() or 1)
PRIME_NS = 999_999_937  # a wake-up period that divides nothing
WRAP_WINDOW = 2 ** 31 - 1 - 50000  # mid (about 100,000 cents) + window is beyond int32

# name -> the options that differ from the script's defaults (pov 0.05, min 20, window 5, 20 ticks, "1S")
CASES = {
    "ticks0": dict(num_ticks=0),             # a ladder of 2
    "ticks31": dict(num_ticks=31),           # 64 orders: exactly one pass
    "ticks32": dict(num_ticks=32),           # 66: a second pass with 2 live lanes
    "ticks62": dict(num_ticks=62),           # 126: a second pass two lanes short
    "ticks63": dict(num_ticks=63),           # 128: two full passes, the open-order list exactly full
    "window0": dict(window_size=0),          # the lowest ask at the mid: ladder orders execute on arrival
    "size0": dict(pov=0.0, min_order_size=0),  # order size 0: ids consumed, nothing sent (the serial loop)
    "min0": dict(min_order_size=0),          # size 0 whenever pov x volume rounds to 0, batched otherwise
    "pov0.5": dict(pov=0.5, min_order_size=1),   # py_round ties: k + 0.5 for every odd volume
    "pov0.25": dict(pov=0.25, min_order_size=1),
    "wake7h": dict(wake_up_freq=7 * 3600 * 10 ** 9),   # longer than the session: no second wake-up
    "wakeprime": dict(wake_up_freq=PRIME_NS),
    "wake100ms": dict(wake_up_freq=10 ** 8),           # sub-second: about 1.56 M events per env
    "combo": dict(pov=0.5, min_order_size=1, window_size=0, num_ticks=63),
}
# reference runs (tests/golden/gen_fixtures.py "rmsc03%POV,MIN,WIN,TICKS,FREQ" SEED): fixture name ->
# (options, seed, the device can hold it)
FIXTURES = {
    "rmsc03_mm_0_0_5_20_1S_30": (dict(pov=0.0, min_order_size=0), 30, True),
    "rmsc03_mm_0.5_1_0_63_1S_30": (dict(pov=0.5, min_order_size=1, window_size=0, num_ticks=63), 30, True),
    "rmsc03_mm_0.05_20_5_32_1S_31": (dict(num_ticks=32), 31, True),
    "rmsc03_mm_0.05_20_0_0_1S_33": (dict(window_size=0, num_ticks=0), 33, True),
    "rmsc03_mm_0.05_20_5_20_7H_30": (dict(wake_up_freq=7 * 3600 * 10 ** 9), 30, True),
    "rmsc03_mm_0.05_20_5_20_500ms_31": (dict(wake_up_freq=5 * 10 ** 8), 31, True),
    "rmsc03_mm_0.05_20_5_64_1S_31": (dict(num_ticks=64), 31, False),  # 130 orders: twice that is beyond the list
}


def row(n=1, **opts):
    """[n] option records: the defaults with `opts` (wake-ups in ns)"""
    o = dict(MM_DEFAULTS, wake_up_freq=10 ** 9)
    o.update(opts)
    return mm_params(n, **o)


def rows(names, seeds=SEEDS):
    """the mixed batch of `names`: regimes interleaved env by env (env i runs row i % len(names) on
    seed i // len(names)), so a serial-path env sits between batched ones.  -> (seeds, options,
    row index of each env)"""
    k = len(names)
    idx = np.arange(k * len(seeds)) % k
    sd = np.repeat(np.asarray(seeds, dtype=np.uint32), k)
    p = np.concatenate([row(**CASES[names[j]]) for j in idx])
    return sd, p, idx


class Expected:
    """the oracle on (seeds, options): `ev`, `hs`, `peak` [n][3] (queue, book, open) of the run
    without capacities (64-bit prices), and `cev`, `chs`, `cer` of the run with the device's
    capacities and 32-bit price words, the device's expected stop; `status`, `err` as the device
    reports them"""

    def __init__(self, seeds, p):
        from capacity_util import ORACLE_TO_DEVICE
        self.seeds, self.p = np.asarray(seeds, dtype=np.uint32), p
        self.ev, self.hs, self.er, _, st = pyoracle.run_batch_mm(self.seeds, p, THREADS, stats=True)
        self.peak = st[:, :3]
        self.cev, self.chs, self.cer, _ = pyoracle.run_batch_mm(self.seeds, p, THREADS, capacities=CAP, price_words=True)
        to_dev = dict(ORACLE_TO_DEVICE)
        to_dev[pyoracle.ERR_ORDER_PRICE] = 31
        self.status = np.where(self.cer == 0, 1, 2)
        self.err = np.array([to_dev[int(e)] if e else 0 for e in self.cer])

    def take(self, sel):
        e = object.__new__(Expected)
        for k, v in self.__dict__.items():
            setattr(e, k, v[sel])
        return e


@functools.lru_cache(maxsize=None)
def mixed():
    """the shared batch of every case row x SEEDS and its oracle runs, computed once"""
    names = tuple(CASES)
    sd, p, idx = rows(names)
    return names, sd, p, idx, Expected(sd, p)


@functools.lru_cache(maxsize=None)
def defaults():
    """SEEDS under the script's default options"""
    return Expected(SEEDS, row(len(SEEDS)))


def quoting():
    """the base seeds whose maker quotes at least twice: under the default options its 42-order
    ladder is placed while the previous one is still open (seeds 32 and 1000 end after about 5 k
    events, before the market maker's first quote, whatever its options)"""
    return defaults().peak[:, 2] == 84


def mismatches(s, x):
    """[n] bool: the envs of a device summary whose status, err, events or hash is not Expected's"""
    return (s["status"] != x.status) | (s["err"] != x.err) | (s["events"] != x.cev) | (s["hash"] != x.chs)


def assert_equals_oracle(s, x, what=""):
    """a device summary against Expected, env by env and exactly: status, err, events and hash of
    the capacity-aware oracle; passing envs also against the run without capacities, with the
    high-water marks against the oracle's peaks; no env ever beyond a capacity"""
    bad = np.nonzero(mismatches(s, x))[0]
    assert len(bad) == 0, "%s: envs %s differ; the first: status %d err %d events %d hash %016x, want %d %d %d %016x" % (
        what, bad.tolist(), s["status"][bad[0]], s["err"][bad[0]], s["events"][bad[0]], s["hash"][bad[0]],
        x.status[bad[0]], x.err[bad[0]], x.cev[bad[0]], x.chs[bad[0]])
    ok = x.status == 1
    assert (s["events"][ok] == x.ev[ok]).all() and (s["hash"][ok] == x.hs[ok]).all(), what
    assert (s["max_queue"][ok] == x.peak[ok, 0]).all(), (what, s["max_queue"][ok], x.peak[ok, 0])
    assert (s["max_book"][ok] == x.peak[ok, 1]).all(), (what, s["max_book"][ok], x.peak[ok, 1])
    assert (s["max_queue"] <= CAP[0]).all() and (s["max_book"] <= CAP[1]).all(), what
