"""Runtime compositions at their price and parameter edges (include/mxa.h MXA_PRICE_MAX): the
compositions, the seed pool and the oracle's runs, shared by test_composition_edges.py (CPU) and
test_gpu_composition_edges.py.

The compositions are those of tests/golden/gen_config_fixtures.py's edge entries, read from their
reference fixtures: rmsc03 with 20 noise, 10 value and 2 momentum agents over five minutes.

  rmsc03_shocks   a megashock every 0.1 s: several per observation, prices well inside the range
  rmsc03_low      r_bar 50: the fundamental is clamped at 0, estimates and ladders reach prices <= 0
  rmsc03_high     r_bar just under 2^31: every first order is above the range
  rmsc03_top      every order at exactly MXA_PRICE_MAX (no maker, constant fundamental): finishes
  rmsc03_over     ... at MXA_PRICE_MAX + 1: stops at its first value order
  rmsc03_bottom   ... at 1: finishes
  rmsc03_zero     ... at 0: stops at its first value order
  rmsc03_top_mm   value orders up to MXA_PRICE_MAX - 3 pass, the maker's first ladder is above the range
"""
import functools

import numpy as np

import pyoracle
from golden_util import load_composition

PRICE_MAX = 2 ** 30 - 1
# (name, seed) of the reference fixtures cfg_<name>_<seed>.*
EDGE_FIXTURES = [("rmsc03_shocks", 1), ("rmsc03_shocks", 2), ("rmsc03_low", 15), ("rmsc03_high", 26), ("rmsc03_top", 7),
                 ("rmsc03_over", 7), ("rmsc03_bottom", 7), ("rmsc03_zero", 7), ("rmsc03_top_mm", 1)]
FINISH = ("rmsc03_top", "rmsc03_bottom")       # every env finishes
STOP_FIRST = ("rmsc03_over", "rmsc03_zero")    # every env stops at its first value order
EDGES = ("rmsc03_low", "rmsc03_high") + FINISH + STOP_FIRST + ("rmsc03_top_mm",)
SEEDS = np.arange(1, 33, dtype=np.uint32)
BOOK_LOG = 1 << 18  # records per env: the longest env writes 147 k with the exchange log on, so no log fills
BL_FUNDAMENTAL = -2 ** 31
K_LIMIT = 11  # trace record word 3 (oracle/abides_oracle.c)
ERR_DEVICE = {0: 0, pyoracle.ERR_ORDER_PRICE: 31}


def composition(name):
    """the composition's every field, from its (first) reference fixture"""
    from mxabides import composition as C
    seed = next(s for n, s in EDGE_FIXTURES if n == name)
    return C.from_dict(load_composition(name, seed)[0]["composition"])


class Run:
    """one oracle env under the device's price range: what the device's summary and records must equal"""

    def __init__(self, cfg, seed, exchange_log, price_words=True):
        o = pyoracle.OracleEnv(cfg, int(seed))
        o.set_book_log()
        if exchange_log:
            o.set_exchange_log()
        if price_words:
            o.set_price_words()
        o.run()
        self.err, self.msg = o.error
        self.events, self.hash = o.events, o.hash
        self.current_time, self.order_counter, self.last_trade = o.current_time, o.order_counter, o.last_trade
        self.records = o.book_records()
        self.status = 1 if self.err == 0 else 2

    @property
    def f_log(self):
        return self.records[self.records[:, 1] == BL_FUNDAMENTAL]


@functools.lru_cache(maxsize=None)
def runs(name, exchange_log=False, seeds=None):
    """[Run] of `name` over SEEDS (or a tuple of seeds), computed once"""
    cfg = composition(name)
    return [Run(cfg, s, exchange_log) for s in (SEEDS if seeds is None else seeds)]


def column(rs, key):
    return np.array([getattr(r, key) for r in rs], dtype=np.uint64 if key == "hash" else np.int64)


def first_value_order(cfg, seed):
    """the number of the pop in which the unbounded oracle's first ValueAgent handles the spread
    reply that makes it place its first order (that order's LIMIT_ORDER is pushed by that pop)"""
    o = pyoracle.OracleEnv(cfg, int(seed), trace_cap=4096)
    o.run(4096)
    t = o.trace()
    lo, hi = 1 + cfg.n_noise, 1 + cfg.n_noise + cfg.n_value
    lim = np.nonzero((t[:, 3] == K_LIMIT) & (t[:, 5] >= lo) & (t[:, 5] < hi))[0]
    first = t[lim[0]]
    before = np.nonzero(t[:lim[0], 1] == first[5])[0]  # the pop that pushed it: that agent's latest before it
    return int(before[-1]) + 1, first


def agent_class_of(cfg, agent):
    """the class of agent id `agent` in an rmsc03 composition (config/rmsc03.py's order)"""
    bounds = [("ExchangeAgent", 1), ("NoiseAgent", cfg.n_noise), ("ValueAgent", cfg.n_value), ("POVMarketMakerAgent", cfg.n_mm),
              ("MomentumAgent", cfg.n_momentum)]
    for cls, n in bounds:
        if agent < n:
            return cls
        agent -= n
    raise ValueError("no such agent")


def expected_stop(cfg, seed):
    """where the price range must stop the env, from the UNBOUNDED oracle's trace alone: (events
    at the stop, class of the agent) of the earliest pop that pushes a LIMIT_ORDER (quantity > 0: a
    zero quantity sends none) at a price outside 1 .. PRICE_MAX, or None if the run holds none.
    The bounded run is the unbounded one up to that pop.  The pop that pushed an order is its
    agent's latest pop before the order's own; the market maker's ladder is one pop's, and as its
    bids and asks are two runs of consecutive prices, it holds a price outside the range exactly
    when its lowest bid or its highest ask is outside, which is the test made before it cancels"""
    u = pyoracle.OracleEnv(cfg, int(seed), trace_cap=1 << 17)
    u.run()
    t = u.trace()
    assert len(t) == u.events
    out = np.nonzero((t[:, 3] == K_LIMIT) & (t[:, 7] > 0) & ((t[:, 8] < 1) | (t[:, 8] > PRICE_MAX)))[0]
    best = None
    for j in out:
        if best is not None and j > best[0] + 4096:  # (an order pops within its pusher's time step)
            break
        a = int(t[j, 5])
        k = int(np.nonzero(t[:j, 1] == a)[0][-1]) + 1
        if best is None or k < best[0]:
            best = (k, agent_class_of(cfg, a))
    return best
