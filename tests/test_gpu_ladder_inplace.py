"""The market maker's cancel and ladder runs taken in its wakeup's pop (Eng::mm_ladder_cycle,
DESIGN.md §3): the CANCEL_ORDER and LIMIT_ORDER runs at the exchange and the ORDER_CANCELLED and
ORDER_ACCEPTED runs at the market maker, handled without a queue trip, must leave every observable
of the queued sequence.  Integer parity against the C oracle and byte equality of whole env blocks
at the edges of the all-or-nothing decision: launch budgets around every boundary of the 89- and
173-pop groups, stopTime at a full-ladder wake, a cycle after a ladder order was filled (41
cancels), the instant the momentum agents share, the close, and the parity hash on and off."""
import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process

import pyoracle

pytestmark = pytest.mark.gpu

NS = 10 ** 9
OPEN = (9 * 3600 + 30 * 60) * NS
SEEDS = [123456789, 1008, 7, 11, 2, 3, 5, 13]  # 1008, 13: a market maker that stalls on a one-sided book
STALLED = (1008, 13)
MM = 61  # rmsc03's market maker (config/rmsc03.py)
MT_MESSAGE, MT_WAKEUP, MK_CANCEL = 1, 2, 12
NL = 42  # its ladder: 2 * (num_ticks + 1) orders


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


_ORACLE = {}


def oracle(stop):
    """per-env oracle records of rmsc03 run to stopTime `stop` (None: the config's), computed once"""
    if stop not in _ORACLE:
        out = []
        for sd in SEEDS:
            o = pyoracle.OracleEnv("rmsc03", sd)
            if stop is not None:
                o.set_stop(stop)
            o.run()
            assert o.error[0] == 0, o.error
            out.append((o.events, o.hash, o.order_counter, o.last_trade, o.agents()[1:]))
        _ORACLE[stop] = out
    return _ORACLE[stop]


_GROUPS = {}


def mm_groups(stop):
    """per seed, from the oracle's trace: (second after the open, pops at the wake's instant from the
    wakeup on, CANCEL_ORDERs among them) of every market-maker wake up to `stop`; computed once"""
    if stop not in _GROUPS:
        out = []
        for sd in SEEDS:
            o = pyoracle.OracleEnv("rmsc03", sd, trace_cap=1 << 18)
            if stop is not None:
                o.set_stop(stop)
            o.run()
            tr = np.asarray(o.trace())
            assert len(tr) == o.events  # the whole run fits the trace
            g = []
            for i in np.nonzero((tr[:, 2] == MT_WAKEUP) & (tr[:, 1] == MM))[0]:
                same = tr[i:, 0] == tr[i, 0]
                n = len(same) if same.all() else int(np.argmin(same))
                grp = tr[i:i + n]
                nc = int(((grp[:, 2] == MT_MESSAGE) & (grp[:, 1] == 0) & (grp[:, 3] == MK_CANCEL)).sum())
                g.append((int((tr[i, 0] - OPEN) // NS), n, nc))
            out.append(g)
        _GROUPS[stop] = out
    return _GROUPS[stop]


def records(m):
    """per-env (events, hash, order counter, last trade, every trading agent's cash / holdings / open orders)"""
    s = m.summary()
    assert (s["status"] != 2).all(), s["err"]
    return [(int(s["events"][i]), int(s["hash"][i]), int(s["order_counter"][i]), int(s["last_trade"][i]),
             [(a["cash"], a["shares"], a["n_open"]) for a in m.agents(i)[1:]]) for i in range(m.n_envs)]


def run_to(mx, stop, chunk=None, hash_on=True):
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(hash_on)
    if stop is not None:
        m.set_stop_time(stop)
    if chunk is None:
        m.run()
    else:
        m.run(chunk=chunk)
    return m


def assert_oracle(m, stop, hash_on=True):
    for i, (got, ref) in enumerate(zip(records(m), oracle(stop))):
        if not hash_on:  # the hash was not computed
            got, ref = got[:1] + got[2:], ref[:1] + ref[2:]
        assert got[:-1] == ref[:-1], (i, got[:-1], ref[:-1])
        assert got[-1] == ref[-1], (i, [k for k, (a, b) in enumerate(zip(got[-1], ref[-1])) if a != b])


# EnvHdr words that record how the launches went, not the market: the RNG streams' LDS windows of
# the last launch (rs_w0, rs_wn) and the path counters kc[25..27] (busy requeues, record round
# trips, pops handled as run members: a launch budget cuts runs into single pops)
HDR_LAUNCH_LOCAL = [(248, 280), (368 + 4 * 25, 368 + 4 * 28)]
HDR_HASH = [(16, 24), (368, 368 + 4 * 28)]  # EnvHdr.hash and the event-class counters only instrumented runs keep


def raw_state(m, skip=()):
    """every env's whole block (header, agent records, open orders, RNG streams, saved queue and
    book, transaction ring) with the launch-local header words (and `skip`) zeroed"""
    out = []
    for i in range(m.n_envs):
        b = m.raw(i, 0, m.env_bytes).copy()
        for lo, hi in HDR_LAUNCH_LOCAL + list(skip):
            b[lo:hi] = 0
        out.append(b)
    return out


def assert_same_blocks(a, b, what):
    for e, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, e, np.nonzero(x != y)[0][:16].tolist())


@pytest.mark.parametrize("hash_on", [True, False])
def test_gpu_launch_budgets_cut_the_long_group(mx, hash_on):
    """open + 3 s: the first ladder (an 89-pop group: 1 + 4 + 42 + 42) and two full cycles (173
    pops: 1 + 4 + 4 x 42, or 171 after a fill) under launch budgets on both sides of every
    boundary of the group.  A budget that cuts the group takes the queued path for all of it; seqs,
    the queue's high-water mark, the pending wakeup's slot and the open-order list end as the
    one-launch run's, byte for byte"""
    stop = OPEN + 3 * NS
    full = 0
    for sd, g in zip(SEEDS, mm_groups(stop)):
        if sd in STALLED:
            continue
        g = [x for x in g if x[0] <= 3]  # (the runner's last pop may be the wake behind stopTime)
        assert [x[0] for x in g] == [0, 1, 2, 3], (sd, g)
        assert g[1][1:] == (2 * NL + 5, 0), (sd, g)
        for x in g[2:]:
            assert x[1:] in ((4 * NL + 5, NL), (4 * NL + 3, NL - 1)), (sd, g)
        full += g[2][1:] == g[3][1:] == (4 * NL + 5, NL)
    assert full >= 4, full
    one = run_to(mx, stop, hash_on=hash_on)
    assert_oracle(one, stop, hash_on)
    want, raw = records(one), raw_state(one)
    for c in (5, 6, 46, 47, 48, 88, 89, 90, 130, 131, 132, 172, 173, 174, 175, 400):
        m = run_to(mx, stop, chunk=c, hash_on=hash_on)
        assert records(m) == want, c
        assert (m.summary()["max_queue"] == one.summary()["max_queue"]).all(), c
        assert_same_blocks(raw_state(m), raw, c)


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_gpu_stop_time_at_a_full_ladder_wake(mx, off):
    stop = OPEN + 3 * NS + off
    assert_oracle(run_to(mx, stop), stop)
    assert_oracle(run_to(mx, stop, chunk=100), stop)


def test_gpu_cycle_after_a_filled_ladder_order(mx):
    """the first wake of each seed that cancels fewer than 42 orders (a ladder order was filled
    since the last wake), read off the oracle's trace: the 41-member runs in place"""
    first = []
    for sd, g in zip(SEEDS, mm_groups(None)):
        short = [x[0] for x in g if x[1] > 2 * NL + 5 and x[2] < NL]
        if sd not in STALLED and short:
            first.append(short[0])
    assert len(first) >= 4, first
    stop = OPEN + (max(first) + 1) * NS
    one = run_to(mx, stop)
    assert_oracle(one, stop)
    m = run_to(mx, stop, chunk=100)
    assert_oracle(m, stop)
    assert_same_blocks(raw_state(m), raw_state(one), "chunk=100")


def test_gpu_shared_instant(mx):
    """open + 20 s: the momentum agents wake on the market maker's nanosecond (the queued path)"""
    stop = OPEN + 21 * NS
    one = run_to(mx, stop)
    assert_oracle(one, stop)
    assert_same_blocks(raw_state(run_to(mx, stop, chunk=100)), raw_state(one), "chunk=100")


def test_gpu_whole_episode_hash_off_equals_hash_on(mx):
    """the whole episode, the close included: the plain kernel (no message is built for an elided
    pop) leaves the instrumented kernel's env blocks apart from the hash and the class counters"""
    on = run_to(mx, None)
    assert_oracle(on, None)
    off = run_to(mx, None, hash_on=False)
    assert_oracle(off, None, hash_on=False)
    assert_same_blocks(raw_state(off, HDR_HASH), raw_state(on, HDR_HASH), "hash off")
