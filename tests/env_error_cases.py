"""The env stop codes (csrc/mxa_layout.h ERR_*): the census of every code, the inputs that reach the
ones a caller can reach through the C-ABI, and the oracle's runs of those inputs, shared by
test_env_errors.py (CPU) and test_gpu_env_errors.py.

An env that stops has status 2 and one of these codes (INTEGRATION.md "Errors"): never silently
truncated, the reference's own behaviour where it has one, in the pop the reference would die in,
with the state before the failing action.  Whole-episode parity almost never goes there: no seed of
the built-in configurations' bench batches reaches a code but 28, so every other code needs an input
made for it.

CENSUS has one row per code:
  sites    the functions of csrc/mxa_kernels.hip whose fail() raises it, one entry per site
           (test_env_errors.py parses the source: a new site or code needs its row)
  oracle   the oracle's fail() code of the same stop (oracle/abides_oracle.c), None where the
           oracle has no such stop; the oracle numbers a stop by its cause, so -3 and -18 each
           stand for two device codes apart by the handle kind
  pin      "case:NAME" (a case below), "test:MODULE::FUNCTION" (the test that already pins it), or
           UNREACHED
  note     for UNREACHED: why no input reaches it and how it was searched

UNREACHED is of two kinds.  SEED_ONLY: the code lives in a configuration that takes nothing but a
seed, or behind a capacity that is no field of any input, and no seed searched reaches it.
NO_DRIVER: every input that would reach the site is refused by the host or excluded by how the
handle is built; the note gives the argument and names the test of the refusal where there is one.
"""
import functools
import json
import os

import numpy as np

import pyoracle
import synth_tapes as S
from golden_util import GOLDEN
from mxabides.tape import Tape

UNREACHED = "UNREACHED"
TRACE_CAP = 4096  # more than the longest env of any case (1,873 events)

# the bench batches (batch 0 of shard.env_seeds) and the seed ranges searched with the oracle on the
# CPU, every env to its end; none ends in a code but rmsc03_sbmm_poll's -18 (device 28)
SEARCHED = ("oracle, every env to its end, no stop but -18: the bench batches rmsc03 / rmsc02 / obi_rmsc02 / rmsc01 x4096, "
            "value_noise / sparse_zi_100 / rmsc03_sbmm / rmsc03_sbmm_poll x2048, random_fund_value / random_fund_diverse "
            "x1024; seeds 0.. of value_noise 32,768, sparse_zi_100 16,384, obi_rmsc02 16,384, rmsc02 12,288, rmsc03 12,288, "
            "rmsc03_sbmm 8,192, random_fund_diverse 3,072; rmsc01 seeds 0..6,143; rmsc02, obi_rmsc02 and rmsc03_sbmm "
            "seeds 100,000..108,191")

# (code, name, sites, oracle code, pin, note)
CENSUS = [
    (1, "ERR_QUEUE_FULL", ("q_push", "q_push_lanes"), -20, "test:test_gpu_capacity_edges::test_gpu_zi_overflow_is_exact", ""),
    (2, "ERR_BOOK_FULL", ("b_enter",), -21, "test:test_gpu_capacity_edges::test_gpu_zi_overflow_is_exact", ""),
    (3, "ERR_OPEN_FULL", ("place_limit_oid",), -22,
     "test:test_gpu_mm_option_edges::test_gpu_open_list_exactly_full_then_one_over", ""),
    (4, "ERR_TX_FULL", ("tx_add",), None, UNREACHED,
     "SEED_ONLY: the transaction ring's size (tx_cap) is no composition field; " + SEARCHED),
    (5, "ERR_PANDAS_NO_TX", ("ex_receive",), -5, "case:pandas_no_tx", ""),
    (6, "ERR_WAKEUP_PAST", ("wakeup_at", "kcancel_at"), -3, "case:late_start", ""),
    (7, "ERR_THETA_INDEX", ("zi_update_estimates",), -6, "case:theta_index", ""),
    (8, "ERR_BAD_CONFIG", ("RPCHK",), None, UNREACHED,
     "SEED_ONLY: the replay book's own consistency checks (RPCHK), true of every state the book can reach; " + SEARCHED),
    (9, "ERR_RNG_OVERRUN", ("rng_maint",), None, UNREACHED,
     "SEED_ONLY: the draw window's size is no composition field; " + SEARCHED),
    (10, "ERR_RP_PRICE", ("ex_spread_reply", "lvl_index", "rp_enter_pf"), None, UNREACHED,
     "NO_DRIVER: the ladder spans every price of the tape (create_replay: pmin .. pmax over all records), an "
     "execution agent's orders go to prices it was quoted from that ladder, and a price outside 0 .. 2^20 - 1 is "
     "refused by the host (test_api_args::test_create_replay; both ends inside: test_gpu_synth_tapes' ladder_ends); "
     "lvl_index has no caller; ex_spread_reply's site needs a level-2 price outside 0 .. 2^20 - 1 on rmsc03_rl, "
     "which takes a seed only"),
    (11, "ERR_RP_POOL", ("rp_enter_pf",), None, UNREACHED,
     "NO_DRIVER: the pool holds records + 4,096 entries (create_replay: C = n_rec + rl_ids); a record adds at "
     "most one entry (a modify replaces the head), and the execution agent's orders are cancelled every 30 s, two "
     "a step (test_env_errors::test_replay_books_stay_below_the_entry_pool)"),
    (12, "ERR_RP_IDS", ("agent_dense",), None, "test:test_gpu_synth_tapes::test_gpu_gym_skip_over_ends_in_err_rp_ids", ""),
    (13, "ERR_RP_KEYERROR", ("mr_wakeup",), -7, UNREACHED,
     "NO_DRIVER: the replay agent wakes at the kernel's start (hours unknown: it returns before the lookup) and at "
     "times it took from the tape's own groups; a wake-up is delayed only by a computation delay, and the replay "
     "configurations' is 0 with no input to set it.  A first tape time before the kernel's start is "
     "ERR_WAKEUP_PAST (case tape_before_start)"),
    (14, "ERR_RP_OBS", ("rl_observe", "rl_observe", "rl_observe", "rl_kernel_cancel"), -8,
     "test:test_gpu_rl::test_gpu_rl_matches_reference_and_oracle", ""),
    (15, "ERR_RP_STOPPING", ("rp_terminate",), -8, UNREACHED,
     "NO_DRIVER: the episode ends when the queue runs dry or past the stop time; the execution agent's wake-ups "
     "chain to the last horizon time, where it ends its trade itself, both horizons end before the market closes, "
     "and a GymKernel handle refuses mxa_set_stop_time (test_gpu_env_errors::test_gpu_gym_handle_stop_is_sticky). "
     "The oracle tells the two -8 apart by message; rmsc03_rl's bench batch holds get_observation's only "
     "(test_gpu_bench_sizes::test_gpu_rmsc03_rl_bench_size_equals_oracle)"),
    (16, "ERR_RP_MODIFY", ("rp_modify", "mr_place_record_as"), None,
     "test:test_gpu_synth_tapes::test_gpu_refused_modify_stops_the_env_at_that_pop", ""),
    (17, "ERR_HBL_WINDOW", ("hbl_place", "hbl_place", "hbl_place"), -11, UNREACHED, "SEED_ONLY: rmsc01 / rmsc02; " + SEARCHED),
    (18, "ERR_HBL_RANGE", ("hbl_place",), None, UNREACHED, "SEED_ONLY: rmsc01 / rmsc02; " + SEARCHED),
    (19, "ERR_FLOAT_PRICE", ("mk_receive",), -13, UNREACHED, "SEED_ONLY: rmsc02's MarketMakerAgent; " + SEARCHED),
    (20, "ERR_BOOK_LOG_FULL", ("bl_put", "bl_put_lanes"), None,
     "test:test_gpu_booklog::test_gpu_book_log_overflow_is_an_env_error", ""),
    (21, "ERR_MD_NO_UPDATE", ("md_publish",), -14, UNREACHED, "SEED_ONLY: the subscribing agents of rmsc02 / obi_rmsc02 / rmsc03_sbmm; " + SEARCHED),
    (22, "ERR_MD_SUBS", ("md_subscribe", "md_publish"), -15, UNREACHED,
     "SEED_ONLY: the subscribing agents of rmsc02 / obi_rmsc02 / rmsc03_sbmm; " + SEARCHED),
    (23, "ERR_MD_KEYERROR", ("md_subscribe",), -16, UNREACHED,
     "SEED_ONLY: the subscribing agents of rmsc02 / obi_rmsc02 / rmsc03_sbmm; " + SEARCHED),
    (24, "ERR_MD_SLOT", ("mk_market_data", "obi_receive"), None, UNREACHED,
     "SEED_ONLY: the subscribing agents of rmsc02 / obi_rmsc02; " + SEARCHED),
    (25, "ERR_TWAP_SCHEDULE", ("tw_receive",), -17, "test:test_gpu_replay_runner::test_gpu_twap_execution_matches_reference", ""),
    (26, "ERR_TWAP_QUOTE", ("tw_receive",), -18, "case:twap_quote_bid_only", ""),
    (27, "ERR_TWAP_MARKET", ("tw_receive",), -19, UNREACHED,
     "SEED_ONLY: placeMarketOrder at horizon[-2]; every trading TWAP env stops at its first horizon time (25 or 26), "
     "120 horizon times earlier, and nothing restarts it"),
    (28, "ERR_SB_MID", ("sb_receive",), -18, "test:test_gpu_bench_sizes::test_gpu_bench_batches_equal_oracle", ""),
    (29, "ERR_ORDER_SIZE", ("mm_note",), None, "test:test_gpu_rmsc03_mm::test_gpu_mm_order_size_beyond_int32_is_an_env_error", ""),
    (30, "ERR_RP_QUOTE_SIZE", ("rp_spread",), None,
     "test:test_gpu_synth_tapes::test_gpu_gym_fills_big_level_quote_is_an_env_error", ""),
    (31, "ERR_ORDER_PRICE", ("o_compute", "place_limit_oid", "mm_requote", "mm_requote"), -23,
     "test:test_gpu_composition_edges::test_gpu_edge_equals_oracle", ""),
]
# the codes that may stay without a pin for want of a seed
SEED_ONLY_ALLOWED = (4, 8, 9, 17, 18, 19, 21, 22, 23, 24, 27)

# ---- composition cases: the reference fixtures cfg_<fixture>_<seed> of tests/golden/gen_config_fixtures.py.
# code / oracle: the stop; seeds: the batch (stopping and clean envs interleaved by seed where the
# composition has both); stops: seed -> events at the stop of the seeds with a reference fixture;
# clean: the fixture seeds that run to the end; neighbours: compositions one step inside, (fixture, seed)
COMPOSITION_CASES = {
    # config/rmsc03.py's market maker beside one value agent: the maker's first
    # QUERY_TRANSACTED_VOLUME finds a history without a transaction.  Every seed stops.
    "pandas_no_tx": dict(code=5, oracle=-5, fixture="rmsc03_mm_value1", seeds=tuple(range(1, 17)), stops={1: 19}, clean=(),
                         neighbours=(("rmsc03_mm_only", 1), ("rmsc03_mm_noise2", 1)),
                         stop_error="AttributeError: 'Series' object has no attribute 'columns'"),
    # the kernel starts 2 ns after the market opens: a first wake-up drawn below mkt_open + 2
    "late_start": dict(code=6, oracle=-3, fixture="rmsc03_late_start", seeds=(1, 27, 2, 3, 13, 4, 5, 6) + tuple(range(28, 36)),
                       stops={27: 6, 13: 11}, clean=(1,), neighbours=(),
                       stop_error="ValueError: ('setWakeup() called with requested time not in future'"),
    # q_max 1 and latencies up to 10 s: a cancel in flight while the next order fills, q = 2
    "theta_index": dict(code=7, oracle=-6, fixture="sparse_zi_q1", seeds=tuple(range(1, 17)), stops={2: 574, 6: 406},
                        clean=(1,), neighbours=(), stop_error="IndexError: list index out of range"),
}


# one seed of each composition's reference fixtures
FIXTURE_SEED = {"rmsc03_mm_value1": 1, "rmsc03_mm_only": 1, "rmsc03_mm_noise2": 1, "rmsc03_late_start": 27, "sparse_zi_q1": 2}


def fixture(name, seed):
    """(fixture dict, trace) of cfg_<name>_<seed>"""
    with open(os.path.join(GOLDEN, "cfg_%s_%d.json" % (name, seed))) as f:
        d = json.load(f)
    return d, np.load(os.path.join(GOLDEN, "cfg_%s_%d.npz" % (name, seed)))["trace"]


def composition(name):
    """the MarketConfig of a fixture's composition (every fixture of a name carries the same one)"""
    from mxabides import composition as C
    return C.from_dict(fixture(name, FIXTURE_SEED[name])[0]["composition"])


class Stop:
    """one oracle env run to its end or its stop: what the device's summary, trace, books and agents
    must equal.  The oracle leaves fail() at once, so its state is the one before the failing action"""

    def __init__(self, o, run=True):
        if run:
            o.run()
        self.err, self.msg = o.error
        self.events, self.hash, self.current_time = o.events, o.hash, o.current_time
        self.order_counter, self.last_trade = o.order_counter, o.last_trade
        self.trace = np.array(o.trace())
        self.bids, self.asks = o.book(0), o.book(1)
        self.agents = [tuple(a) for a in o.agents()]
        self.status = 1 if self.err == 0 else 2


@functools.lru_cache(maxsize=None)
def composition_runs(fixture_name, seeds):
    """[Stop] of a composition over a tuple of seeds, under the device's price range, computed once"""
    cfg = composition(fixture_name)
    out = []
    for s in seeds:
        o = pyoracle.OracleEnv(cfg, int(s), trace_cap=TRACE_CAP)
        o.set_price_words()
        out.append(Stop(o))
    return out


# ---- crafted tapes (synth_tapes.py builders).  name -> (builder, handle kind, device code, oracle code)
def _twap(sides, ticker):
    """a book with the given sides resting from 09:30:01 on, untouched at 10:00, the trading TWAP
    agent's first horizon time; the closing record after 10:01 bounds the tape"""
    b = S._Builder(ticker)
    x = 10_000
    if "b" in sides:
        b.place(x - 5, 7, S.BUY)
    if "a" in sides:
        b.place(x + 5, 7, S.SELL)
    b.t = S.OPEN_NS + 31 * 60 * 1000 * S.NS_MS
    return b.tape(x)


def twap_quote_bid_only():
    return _twap("b", "TWQB")


def twap_quote_ask_only():
    return _twap("a", "TWQA")


def twap_two_sided():
    return _twap("ba", "TWQ2")


def _first_time(t0, ticker):
    t = np.array([t0, S.OPEN_NS + 10 ** 9, S.OPEN_NS + 2 * 10 ** 9], dtype=np.int64)
    i = S.first_id()
    return Tape(t, [i, i + 1, i + 2], [100, 101, 100], [1, 1, 1], [1, 0, 1], symbol=ticker, date=S.DATE)


def tape_before_start():
    """the first record 1 ns before midnight, the kernel's start: the replay agent's first wake-up
    (mkt_open + getWakeFrequency() = the first tape time) lies in the past when it learns the hours"""
    return _first_time(-1, "TNEG")


def tape_at_start():
    return _first_time(0, "TZER")


# kind: the handle (VecMarket config); twap: OracleReplayRunner's
TAPE_CASES = {
    "twap_quote_bid_only": dict(tape=twap_quote_bid_only, kind="marketreplay_twap_e", twap=True, code=26, oracle=-18, events=20),
    "twap_quote_ask_only": dict(tape=twap_quote_ask_only, kind="marketreplay_twap_e", twap=True, code=26, oracle=-18, events=20),
    "twap_two_sided": dict(tape=twap_two_sided, kind="marketreplay_twap_e", twap=True, code=25, oracle=-17, events=23),
    "twap_quote_bid_only_passive": dict(tape=twap_quote_bid_only, kind="marketreplay_twap", twap=False, code=0, oracle=0, events=19),
    "tape_before_start": dict(tape=tape_before_start, kind="marketreplay_runner", twap=None, code=6, oracle=-3, events=6),
    "tape_at_start": dict(tape=tape_at_start, kind="marketreplay_runner", twap=None, code=0, oracle=0, events=16),
}


@functools.lru_cache(maxsize=None)
def tape_run(name):
    c = TAPE_CASES[name]
    tp = c["tape"]()
    return tp, Stop(pyoracle.OracleReplayRunner(tp, symbol=tp.symbol, trace_cap=TRACE_CAP, twap=c["twap"]))


# ---- the GymKernel handle of the stickiness checks: rmsc03 + DummyRL on these seeds under zero
# actions; the oracle says which envs stop (get_observation on an empty book side, -8 / device 14)
GYM_SEEDS = (123456789, 123456798, 7, 1008, 123456790, 123456791, 123456792, 123456793)
GYM_STEPS = 8


@functools.lru_cache(maxsize=None)
def gym_runs():
    """per env of GYM_SEEDS: (oracle, [(events, done, rc, obs or None) after each of GYM_STEPS steps; a
    stopped env's list ends with its stop])"""
    out = []
    for s in GYM_SEEDS:
        o = pyoracle.OracleGymEnv(seed=s)
        steps = []
        for _ in range(GYM_STEPS):
            obs, done, rc = o.step(np.zeros(3))
            steps.append((o.events, done, rc, None if obs is None else obs.copy()))
            if rc or done:
                break
        out.append((o, steps))
    return out
