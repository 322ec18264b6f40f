"""The tighter nothing-else-pending test of the in-place groups (Eng::none_before, DESIGN.md §3
"The bound"): a group of agent a's at t is taken in its wakeup's pop when no pending key is below
(t, a + 1), so the market maker (61) takes its whole group at the instants it shares with the
momentum agents (62, 63).  test_gpu_shared_instants_are_taken_in_place asserts the path through
mxa_read_inplace; the stopTime and budget tests pin the shared instants' edges against the oracle.

The other tests are a guard for in-place work on the pops around a value, noise or momentum
agent's order (queued now; DESIGN.md Appendix R.9 has the builds that were measured and taken out):
windows with orders that rest, fill outright, fill and rest, against one maker and several.  They
hold for any path those pops take.  Everywhere the yardstick is the queued sequence: integer parity
against the C oracle (events, per-pop hash, order counter, last trade, every agent's cash /
holdings / open orders) and byte equality of whole env blocks between one launch and launches cut
by budgets.  Each test first asserts from the oracle's trace that its window holds the case it names.

Own next wakeup: a value agent's next wakeup lands on t itself only if its exponential draw rounds
to 0 ns (mean 1 / 7e-11 ns = 14.3 s).  No value wake of the eight seeds' whole episodes has one
(checked on the oracle's traces), and none is constructed here; so a bound one recipient too low,
(t, a), passes this file, while one too high, (t, a + 2), fails the in-place count below.

mxa_read_counters' run-member and record-round-trip counters do not tell the paths apart: the
in-place paths count what the queued pops count (test_gpu_sync_query.py pins that against the
queued build's counters).  mxa_read_inplace does."""
import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process

import pyoracle

pytestmark = pytest.mark.gpu

NS = 10 ** 9
OPEN = (9 * 3600 + 30 * 60) * NS
SEEDS = [123456789, 1008, 7, 11, 2, 3, 5, 13]  # 1008, 13: a market maker that stalls on a one-sided book
STALLED = (1008, 13)
NOISE, VALUE, MM, MOM = range(1, 51), range(51, 61), 61, range(62, 64)  # rmsc03's agent ids (config/rmsc03.py)
MT_MESSAGE, MT_WAKEUP = 1, 2
MK_SPREAD_REQ, MK_LIMIT, MK_ACCEPTED, MK_EXECUTED = 5, 11, 14, 15
WINDOW = OPEN + 60 * NS
KINDS = ("rest", "fill1", "fillN", "fill+rest1", "fill+restN")


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


_TRACE = []


def traces():
    """the oracle's trace of every seed up to WINDOW, computed once"""
    if not _TRACE:
        for sd in SEEDS:
            o = pyoracle.OracleEnv("rmsc03", sd, trace_cap=1 << 16)
            o.set_stop(WINDOW)
            o.run()
            tr = np.asarray(o.trace())
            assert len(tr) == o.events  # the whole window fits the trace
            _TRACE.append(tr)
    return _TRACE


_ORDERS = []


def orders():
    """per seed, every single LIMIT_ORDER the exchange pops in the window (the market maker's ladder
    apart): (t, sender, kind), kind by the replies that follow it: "rest" (ORDER_ACCEPTED alone),
    "fill1" / "fillN" (executed outright against one maker / several), "fill+rest1" / "fill+restN"
    (executed, then the remainder accepted)"""
    if not _ORDERS:
        for tr in traces():
            out = []
            for i in np.nonzero((tr[:, 2] == MT_MESSAGE) & (tr[:, 1] == 0) & (tr[:, 3] == MK_LIMIT) & (tr[:, 5] != MM))[0]:
                ag, oid = int(tr[i, 5]), tr[i, 4]
                nxt = tr[i + 1:i + 64]
                nxt = nxt[(nxt[:, 0] == tr[i, 0]) & (nxt[:, 1] == ag) & (nxt[:, 4] == oid)]
                ex = int((nxt[:, 3] == MK_EXECUTED).sum())
                acc = bool((nxt[:, 3] == MK_ACCEPTED).any())
                assert ex or acc, (ag, oid)
                kind = "rest" if not ex else ("fill+rest" if acc else "fill") + ("1" if ex == 1 else "N")
                out.append((int(tr[i, 0]), ag, kind))
            _ORDERS.append(out)
    return _ORDERS


def first_order(agents, kind, after=OPEN + NS):
    """(t, seed index) of the earliest order of `kind` by one of `agents` behind `after`, over the seeds"""
    hits = [(t, e) for e, out in enumerate(orders()) for t, ag, k in out if ag in agents and k == kind and t > after]
    assert hits, (kind, "not in the window")
    return min(hits)


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


def polls(tr, agents, lo, hi):
    """wakeups of `agents` in (lo, hi] that are followed at once by their QUERY_SPREAD at the exchange"""
    w = (tr[:-1, 2] == MT_WAKEUP) & np.isin(tr[:-1, 1], list(agents)) & (tr[:-1, 0] > lo) & (tr[:-1, 0] <= hi)
    q = (tr[1:, 2] == MT_MESSAGE) & (tr[1:, 1] == 0) & (tr[1:, 3] == MK_SPREAD_REQ) & (tr[1:, 0] == tr[:-1, 0]) & (tr[1:, 4] == tr[:-1, 1])
    return int((w & q).sum())


@pytest.mark.parametrize("hash_on", [True, False])
def test_gpu_launch_budgets_cut_the_value_and_poll_groups(mx, hash_on):
    """open + 21 s under launch budgets of 1-9 and 64 pops.  The value agents' groups (wakeup,
    CANCEL_ORDER, QUERY_SPREAD, ORDER_CANCELLED, spread reply, then the LIMIT_ORDER and its
    ORDER_ACCEPTED or executions) and the noise and momentum agents' polls (wakeup, QUERY_SPREAD,
    reply, LIMIT_ORDER, replies) start at every phase of the budgets, so each is cut at every
    position, both sides of the LIMIT_ORDER and ORDER_ACCEPTED pops included; the market maker's
    group at the shared instant open + 20 s likewise.  A budget that cuts an in-place group takes the
    queued path for it; seqs, the queue's high-water mark and the saved queue end as the one-launch
    run's, byte for byte"""
    stop = OPEN + 21 * NS
    for sd, tr, out in zip(SEEDS, traces(), orders()):
        kinds = {(ag in VALUE, k) for t, ag, k in out if t <= stop}
        assert (True, "rest") in kinds and any(v and k != "rest" for v, k in kinds), (sd, kinds)  # value orders that rest, that cross
        assert any(not v for v, k in kinds), (sd, kinds)  # noise orders
        assert polls(tr, NOISE, OPEN, stop) >= 5 and polls(tr, VALUE, OPEN, stop) >= 5, sd
        if sd not in STALLED:
            assert polls(tr, MOM, OPEN + NS, stop) == 2, sd  # the momentum agents' poll at open + 20 s
    one = run_to(mx, stop, hash_on=hash_on)
    assert_oracle(one, stop, hash_on)
    want, raw = records(one), raw_state(one)
    for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64):
        m = run_to(mx, stop, chunk=c, hash_on=hash_on)
        assert records(m) == want, c
        assert (m.summary()["max_queue"] == one.summary()["max_queue"]).all(), c
        assert_same_blocks(raw_state(m), raw, c)


def stop_cases():
    """stopTime cases: a value wake whose order rests, one whose order crosses, a shared instant"""
    return {"rests": first_order(VALUE, "rest")[0],
            "crosses": min(first_order(VALUE, k) for k in KINDS[1:] if any(x[2] == k and x[1] in VALUE for o in orders() for x in o))[0],
            "shared": OPEN + 20 * NS}


@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("case", ["rests", "crosses", "shared"])
def test_gpu_stop_time_at_a_group(mx, case, off):
    """stopTime at, 1 ns before and 1 ns after a value wake whose order rests, one whose order crosses,
    and an instant the market maker shares with the momentum agents"""
    t = stop_cases()[case]
    if case == "shared":
        for sd, tr in zip(SEEDS, traces()):
            if sd not in STALLED:
                w = tr[(tr[:, 2] == MT_WAKEUP) & (tr[:, 0] == t)][:, 1].tolist()
                assert w[0] == MM and set(w[1:]) == set(MOM), (sd, w)
    stop = t + off
    assert_oracle(run_to(mx, stop), stop)
    assert_oracle(run_to(mx, stop, chunk=3), stop)


@pytest.mark.parametrize("who,kind", [("value", k) for k in KINDS] + [("noise", k) for k in KINDS[1:]])
def test_gpu_kinds_of_order(mx, who, kind):
    """a window that ends at the instant of the first order of each kind: a value order that rests, that
    fills outright against one maker and against several, that fills and rests its remainder against
    one maker and against several; a noise order of every kind (they always cross).  Every agent's
    cash, holdings and open orders right after it equal the oracle's"""
    t, e = first_order(VALUE, kind) if who == "value" else first_order(NOISE, kind, after=OPEN - 1)
    one = run_to(mx, t)
    assert_oracle(one, t)
    assert_same_blocks(raw_state(run_to(mx, t, chunk=4)), raw_state(one), "chunk=4")


def test_gpu_shared_instants_are_taken_in_place(mx):
    """open + 20 s: the market maker wakes first (agent 61) with the momentum agents' wakeups (62, 63)
    pending at the same nanosecond, behind the bound.  Between open + 19.5 s and open + 20 s the only
    market-maker wake is that one, so the in-place counts of a run to open + 20 s exceed those of a
    run to open + 19.5 s by one query group per env whose market maker is not stalled, each with its
    cancel / ladder group (a market maker that waits for both replies re-quotes on the second; the
    ladder group's own fallbacks need a ladder order filled down to one live entry of a list chunk,
    a full queue or a crossing ladder, none of which a 20-tick ladder around the mid meets)"""
    live = 0
    for sd, tr in zip(SEEDS, traces()):
        w = tr[(tr[:, 2] == MT_WAKEUP) & (tr[:, 0] == OPEN + 20 * NS)][:, 1].tolist()
        between = tr[(tr[:, 2] == MT_WAKEUP) & (tr[:, 1] == MM) & (tr[:, 0] > OPEN + 19 * NS + NS // 2) & (tr[:, 0] < OPEN + 20 * NS)]
        assert len(between) == 0, sd
        if sd in STALLED:
            assert MM not in w, (sd, w)
        else:
            assert w[0] == MM and set(w[1:]) == set(MOM), (sd, w)
            live += 1
    assert live == 6
    counts = []
    for stop in (OPEN + 19 * NS + NS // 2, OPEN + 20 * NS):
        m = mx.VecMarket("rmsc03", SEEDS)
        m.set_parity_hash(True)
        m.set_stop_time(stop)
        m.inplace_groups()  # clear what earlier runs of this process left
        m.run()
        assert_oracle(m, stop)
        counts.append(m.inplace_groups().astype(np.int64))
    d = counts[1] - counts[0]
    assert d[0] == live and d[2] == live, (counts, live)
    assert d[1] >= 0 and counts[0][1] > 0 and d[3] == 0, counts  # (value wakes in place in both runs)


def test_gpu_shared_instants_momentum_and_market_maker(mx):
    """open + 20, 40 and 60 s: the market maker wakes first (agent 61), the momentum agents' wakeups
    (62, 63) are pending at the same nanosecond behind the bound, and each then polls in turn.  The
    run equals the oracle, and its counters (per-kind pops, requeues, record round trips, run
    members) equal those of a run whose 4-pop budgets force every group onto the queued path"""
    n = 0
    for sd, tr in zip(SEEDS, traces()):
        if sd in STALLED:
            continue
        for s in (20, 40, 60):
            w = tr[(tr[:, 2] == MT_WAKEUP) & (tr[:, 0] == OPEN + s * NS)][:, 1].tolist()
            assert w[0] == MM and set(w[1:]) == set(MOM), (sd, s, w)
            n += 1
    assert n >= 3 * 6
    one = run_to(mx, WINDOW)
    assert_oracle(one, WINDOW)
    cut = run_to(mx, WINDOW, chunk=4)
    assert_oracle(cut, WINDOW)
    a, b = one.counters(), cut.counters()
    assert (a[:, :31] == b[:, :31]).all()  # (31, 32: record round trips and run members, launch-local)
    assert_same_blocks(raw_state(cut), raw_state(one), "chunk=4")


def test_gpu_step_kernel(mx):
    """rmsc03 + DummyRL over the same window (3 steps: to 09:31:00, :30, 09:32:00): k steps in one
    launch equal one-step launches and the oracle"""
    from mxabides.gym import ACTION_SIZE, OBS_SIZE, VecABIDESEnv
    n, k = len(SEEDS), 3
    acts = np.random.RandomState(31).uniform(0, 1, (k, n, ACTION_SIZE))
    acts[:, :, 0] *= 0.05
    r = pyoracle.gym_batch(acts, 8, seeds=np.array(SEEDS, dtype=np.uint32))
    act = torch.tensor(acts, dtype=torch.float64, device="cuda")
    obs_a = torch.zeros((k, n, OBS_SIZE), dtype=torch.float64, device="cuda")
    flg_a = torch.zeros((k, n), dtype=torch.int32, device="cuda")
    obs_b, flg_b = torch.zeros_like(obs_a), torch.zeros_like(flg_a)
    a, b = VecABIDESEnv(seeds=SEEDS), VecABIDESEnv(seeds=SEEDS)
    for v in (a, b):
        v.set_parity_hash(True)
        v.reset()
    torch.cuda.synchronize()  # the handles run on streams of their own
    for i in range(k):
        a.step_device(act[i].data_ptr(), obs_a[i].data_ptr(), flg_a[i].data_ptr())
    b.step_many_device(k, act.data_ptr(), obs_b.data_ptr(), flg_b.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(flg_a, flg_b)
    assert torch.equal(obs_a.view(torch.int64), obs_b.view(torch.int64))  # bit for bit
    sa, sb = a.summary(), b.summary()
    for key in ("events", "hash", "status", "err", "current_time", "order_counter"):
        assert (sa[key] == sb[key]).all(), key
    assert (sb["events"] == r["events"]).all() and (sb["hash"] == r["hash"]).all(), (sb["events"], r["events"])


def test_gpu_outside_the_masks_runtime_market_maker_options(mx):
    """rmsc03 with per-env market-maker options (scripts/rmsc03.sh: a 102-order ladder every 10 s) is
    outside every in-place mask: the queued path, unchanged"""
    from mxabides.configs import mm_params
    seeds = np.array(SEEDS, dtype=np.uint32)
    p = mm_params(len(seeds), pov=0.05, min_order_size=25, window_size=5, num_ticks=50, wake_up_freq="10S")
    m = mx.VecMarket("rmsc03", seeds, mm_params=p)
    m.set_parity_hash(True)
    m.run()
    s = m.summary()
    ev, hs, er, _ = pyoracle.run_batch_mm(seeds, p, 8)
    assert (er == 0).all() and (s["status"] == 1).all()
    assert (s["events"] == ev).all() and (s["hash"] == hs).all()


def test_gpu_whole_episode_hash_off_equals_hash_on(mx):
    """the whole episode, the close included: the plain kernel (no message is built for an elided
    pop) leaves the instrumented kernel's env blocks apart from the hash and the class counters"""
    on = run_to(mx, None)
    assert_oracle(on, None)
    off = run_to(mx, None, hash_on=False)
    assert_oracle(off, None, hash_on=False)
    assert_same_blocks(raw_state(off, HDR_HASH), raw_state(on, HDR_HASH), "hash off")
