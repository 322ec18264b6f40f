"""The POV market maker's option edges on the per-env options engine (mxa_create_params,
MXA_RMSC03_MM): every branch boundary of mm_requote / mm_place_ladder (csrc/mxa_kernels.hip) that
the option grid of test_gpu_rmsc03_mm.py leaves out.  The cases and their reasons are the table of
mm_edge_util.py; the conditions on the seed pool are asserted on the CPU (test_mm_option_edges.py).

Every comparison is exact: events, hash, status and err per env against the C oracle with the
device's capacities (320 pending events, 192 resting orders, 256 open orders per agent) and its
32-bit price words; passing envs also against the oracle without either, with the high-water
marks against its peaks.  The oracle itself is pinned to reference runs at these edges
(tests/golden/rmsc03_mm_*)."""
import numpy as np
import pytest

import mm_edge_util as U
import pyoracle
from golden_util import first_mismatch, load_named

pytestmark = pytest.mark.gpu
MM_ID = 61  # rmsc03's market maker (config/rmsc03.py)
KEYS = ("events", "hash", "status", "err", "max_queue", "max_book", "current_time", "order_counter", "last_trade")


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


_ONE = {}


def _mixed_in_one_launch(mx):
    if not _ONE:
        names, sd, p, idx, x = U.mixed()
        m = mx.VecMarket("rmsc03", sd, mm_params=p)
        _ONE["launches"] = m.run()
        _ONE["s"] = m.summary()
        m.close()
    return _ONE["s"]


def test_gpu_mixed_batch_equals_oracle(mx):
    """every case row x 8 seeds as one handle, the regimes interleaved env by env: an env on the
    serial place_limit loop (size 0) sits between envs on one and two batched passes"""
    names, sd, p, idx, x = U.mixed()
    s = _mixed_in_one_launch(mx)
    for j, name in enumerate(names):
        m = idx == j
        print("%-10s %d of %d envs differ, status %s events %s" % (
            name, U.mismatches(s, x)[m].sum(), m.sum(), s["status"][m].tolist(), s["events"][m].tolist()))
    U.assert_equals_oracle(s, x, "mixed batch")
    assert (s["status"] == 1).all()


def test_gpu_mixed_batch_in_997_pop_launches(mx):
    """the same batch through launches of 997 pops, which save and reload queue, book and the
    open-order list between launches: every result word of the one-launch run"""
    names, sd, p, idx, x = U.mixed()
    one = _mixed_in_one_launch(mx)
    m = mx.VecMarket("rmsc03", sd, mm_params=p)
    n = m.run(chunk=997)
    s = m.summary()
    m.close()
    assert n > 1000
    U.assert_equals_oracle(s, x, "997-pop launches")
    for k in KEYS:
        assert (s[k] == one[k]).all(), k


@pytest.mark.parametrize("name", sorted(n for n, f in U.FIXTURES.items() if f[2]))
def test_gpu_edge_matches_reference(mx, name):
    """the reference's own run at the edge, as a single-env handle: every trace record kept, books,
    report lines and the summary log"""
    opts, seed, _ = U.FIXTURES[name]
    d, ref, summ = load_named(name)
    m = mx.VecMarket("rmsc03", [seed], trace_cap=len(ref), mm_params=U.row(**opts))
    m.run()
    s = m.summary()
    assert s["status"][0] == 1, "env error %d" % s["err"][0]
    assert first_mismatch(m.trace(0), ref) == -1
    assert int(s["events"][0]) == d["events"] and "%016x" % int(s["hash"][0]) == d["hash"]
    assert m.book(0, 0) == d["bids"] and m.book(0, 1) == d["asks"]
    holdings, means = m.report(0)
    assert holdings == d["final_holdings_lines"] and means == d["mean_lines"]
    got = m.summary_log(0)
    assert len(got) == len(summ)
    for a, b in zip(got, summ):
        assert a == b and type(a["Event"]) is type(b["Event"]), (a, b)
    m.close()


def test_gpu_open_list_exactly_full_then_one_over(mx):
    """63 ticks beside 64, 65, 80 and 127 in one handle.  Two 128-order ladders fill the open-order
    list exactly and pass with the uncapped hash; from 64 ticks on the env stops (status 2) in the
    pop the capped oracle stops in, and its 63-tick neighbours never notice.  64, 65 and 80 ticks
    stop with ERR_OPEN_FULL (3) at the second quote, at the first order over 256.  127 ticks never
    gets that far: its first ladder of 256 orders is more than the 192 resting orders the book
    holds, so the capped oracle, and the device, stop with ERR_BOOK_FULL (2) while the exchange
    takes it in.  Envs whose maker never quotes (seeds 32, 1000) pass whatever their ticks."""
    ticks = np.array([63, 64, 63, 65, 63, 80, 63, 127] * len(U.SEEDS))
    sd = np.repeat(np.asarray(U.SEEDS, dtype=np.uint32), 8)
    q = np.repeat(U.quoting(), 8)
    p = np.concatenate([U.row(num_ticks=int(t)) for t in ticks])
    x = U.Expected(sd, p)
    m = mx.VecMarket("rmsc03", sd, mm_params=p)
    m.run()
    s = m.summary()
    n_open = np.array([m.agents(i)[MM_ID]["n_open"] for i in range(m.n_envs)])
    most = np.array([max(a["n_open"] for a in m.agents(i)) for i in range(m.n_envs)])
    m.close()
    print("status", s["status"].tolist(), "err", s["err"].tolist(), "maker open", n_open.tolist())
    U.assert_equals_oracle(s, x, "full then one over")
    full = ticks == 63
    assert (s["status"][full] == 1).all() and (x.peak[full & q, 2] == 256).all() and (full & q).sum() == 24
    assert (s["status"][~q] == 1).all()
    over = ~full & q
    assert (s["status"][over] == 2).all()
    assert (s["err"][over & (ticks != 127)] == 3).all() and (n_open[over & (ticks != 127)] == 256).all()
    assert (s["err"][over & (ticks == 127)] == 2).all() and (s["max_book"][over & (ticks == 127)] == U.CAP[1]).all()
    assert (most <= U.CAP[2]).all() and (n_open == most)[q].all()


def test_gpu_ladder_prices_beyond_int32_stop_the_env(mx):
    """--mm-window-size 2^31 - 1 - 50000 at 20 ticks: mid + window is beyond the 32-bit price
    words.  The 64-bit oracle quotes those asks; the device cannot, and an env that ended with
    status 1 and another hash would have quoted wrapped prices.  Either mxa_create_params refuses
    the options, or each env is the oracle's with 32-bit price words bit for bit: stopped with
    error 31 (ERR_ORDER_PRICE) at the maker's first requote, before it cancels or places."""
    p = U.row(len(U.SEEDS), window_size=U.WRAP_WINDOW)
    x = U.Expected(U.SEEDS, p)
    q = U.quoting()
    assert (x.er == 0).all() and (x.cer[q] == pyoracle.ERR_ORDER_PRICE).all() and (x.cer[~q] == 0).all()
    try:
        m = mx.VecMarket("rmsc03", U.SEEDS, mm_params=p)
    except mx.MxaError:
        return
    m.run()
    s = m.summary()
    m.close()
    print("status", s["status"].tolist(), "err", s["err"].tolist(), "events", s["events"].tolist())
    quiet = (s["status"] == 1) & (s["hash"] != x.hs)
    assert not quiet.any(), "wrapped ladder prices in envs %s" % np.nonzero(quiet)[0].tolist()
    U.assert_equals_oracle(s, x, "price words")
    assert (s["status"][q] == 2).all() and (s["err"][q] == 31).all()


REGIMES = ["ticks63", "size0", "window0", "ticks32", "pov0.5", "min0", "ticks0", "combo"]


def test_gpu_masked_reset_takes_the_new_options(mx):
    """16 envs of mixed rows run to 20,000 pops; mxa_set_mm_params swaps every env's row for
    another regime; reset(odd envs).  The odd envs run the new rows from the start, the even envs
    finish under the options they began with (the maker's record keeps them); after a whole reset
    every env runs the new rows."""
    n = 16
    sd = np.asarray([U.SEEDS[i % 8] for i in range(n)], dtype=np.uint32)
    old = np.concatenate([U.row(**U.CASES[REGIMES[i % 8]]) for i in range(n)])
    new = np.concatenate([U.row(**U.CASES[REGIMES[(i + 3) % 8]]) for i in range(n)])
    xo, xn = U.Expected(sd, old), U.Expected(sd, new)
    assert ((xo.hs != xn.hs) | ~np.tile(U.quoting(), 2)).all()
    m = mx.VecMarket("rmsc03", sd, mm_params=old)
    assert m.run(chunk=5000, max_launches=4) == 4
    st = m.summary()["status"]
    odd = (np.arange(n) % 2).astype(np.uint8)
    assert (st[odd == 1] == 0).any() and (st[odd == 0] == 0).any(), st
    m.set_mm_params(new)
    m.reset(odd)
    ev = m.summary()["events"]
    assert (ev[odd == 1] == 0).all() and (ev[odd == 0] > 0).all()
    m.run()
    s = m.summary()
    sel = odd == 1
    U.assert_equals_oracle({k: v[sel] for k, v in s.items()}, xn.take(sel), "odd envs, new rows")
    U.assert_equals_oracle({k: v[~sel] for k, v in s.items()}, xo.take(~sel), "even envs, old rows")
    m.reset()
    m.run()
    U.assert_equals_oracle(m.summary(), xn, "whole reset, new rows")
    m.close()


def test_gpu_snapshot_fork_carries_the_options(mx):
    """env 0 at 63 ticks / pov 0.5 / min 1, envs 1-3 at the defaults, cut at 20,000 pops; env 0 is
    saved and restored into all four.  The options travel in the maker's record, so every env
    ends as the oracle of env 0's seed and env 0's options; the handle's option table is untouched,
    so after reset() envs 1-3 run their own seeds and rows again."""
    sd = np.asarray([30, 31, 33, 1001], dtype=np.uint32)
    p = np.concatenate([U.row(pov=0.5, min_order_size=1, num_ticks=63), U.row(3)])
    x = U.Expected(sd, p)
    assert (x.cer == 0).all() and x.peak[0, 2] == 256 and len(set(x.hs.tolist())) == 4
    m = mx.VecMarket("rmsc03", sd, mm_params=p)
    assert m.run(chunk=5000, max_launches=4) == 4
    assert (m.summary()["status"] == 0).all()
    snap = m.snapshot(1)
    snap.save({0: 0})
    snap.restore({i: 0 for i in range(4)})
    snap.close()
    m.run()
    s = m.summary()
    U.assert_equals_oracle(s, x.take(np.zeros(4, dtype=np.int64)), "forks of env 0")
    m.reset()
    m.run()
    U.assert_equals_oracle(m.summary(), x, "after reset")
    m.close()


def _oracle_stream(seed, mm):
    o = pyoracle.OracleEnv("rmsc03", seed, mm=mm)
    o.set_book_log()
    o.set_exchange_log()
    o.run()
    assert o.error[0] == 0
    return o.book_records()


def test_gpu_book_update_log_of_a_128_order_ladder(mx):
    """the book-update log with the exchange log on, record for record the oracle's: 63 ticks (a
    LIMIT run of 128 orders, the longest the log has seen), size 0 (ids consumed, nothing logged)
    and 63 ticks at window 0 with py_round ties (ladder orders that execute inside the run)"""
    sd = [30, 31, 33]
    p = np.concatenate([U.row(**U.CASES[k]) for k in ("ticks63", "size0", "combo")])
    want = [_oracle_stream(s, p[i]) for i, s in enumerate(sd)]
    m = mx.VecMarket("rmsc03", sd, mm_params=p, book_log=max(len(a) for a in want) + 64, exchange_log=True)
    m.run()
    s = m.summary()
    assert (s["status"] == 1).all(), s["err"]
    for i, a in enumerate(want):
        d = m.book_log_records(i)
        print("env %d: %d records" % (i, len(d)))
        assert len(d) == len(a), (i, len(d), len(a))
        assert (d["t"] == a[:, 0]).all() and (d["price"] == a[:, 1]).all() and (d["qty"] == a[:, 2]).all(), i
    assert len(want[0]) > 100 * len(want[1])
    m.close()
