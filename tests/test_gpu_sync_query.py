"""Exchange queries answered in place (Eng::mm_cycle): the POV market maker's
QUERY_SPREAD / QUERY_TRANSACTED_VOLUME round trip handled inside its wakeup's pop must leave every
observable of the queued sequence.  Integer parity against the C oracle (events, per-pop hash,
order counter, last trade, every agent's cash / holdings / open orders) at the edges of the
in-place path: a launch budget that cuts the group at every position, stopTime at, before and
after a market-maker wake, an instant the momentum agents share with the market maker (the
queued fallback), a value agent waking with an open order, the step kernel, and a configuration
outside MXA_INPLACE_MASK."""
import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process (the step kernel's device buffers)

import pyoracle

pytestmark = pytest.mark.gpu

NS = 10 ** 9
OPEN = (9 * 3600 + 30 * 60) * NS
SEEDS = [123456789, 1008, 7, 11, 2, 3, 5, 13]  # 1008: a market maker that stalls on a one-sided book
MM, VALUE = 61, range(51, 61)  # rmsc03's agent ids (config/rmsc03.py)
MT_MESSAGE, MT_WAKEUP, MK_CANCEL = 1, 2, 12


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


def records(m):
    """per-env (events, hash, order counter, last trade, every trading agent's cash / holdings / open orders)"""
    s = m.summary()
    assert (s["status"] != 2).all(), s["err"]
    return [(int(s["events"][i]), int(s["hash"][i]), int(s["order_counter"][i]), int(s["last_trade"][i]),
             [(a["cash"], a["shares"], a["n_open"]) for a in m.agents(i)[1:]]) for i in range(m.n_envs)]


def run_to(mx, stop, chunk=None):
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    if stop is not None:
        m.set_stop_time(stop)
    if chunk is None:
        m.run()
    else:
        m.run(chunk=chunk)
    return m


def assert_oracle(m, stop):
    for i, (got, ref) in enumerate(zip(records(m), oracle(stop))):
        assert got[:4] == ref[:4], (i, got[:4], ref[:4])
        assert got[4] == ref[4], (i, [k for k, (a, b) in enumerate(zip(got[4], ref[4])) if a != b])


# EnvHdr words that record how the launches went, not the market: the RNG streams' LDS windows of
# the last launch (rs_w0, rs_wn) and the path counters kc[25..27] (busy requeues, record round
# trips, pops handled as run members: a launch budget cuts runs into single pops)
HDR_LAUNCH_LOCAL = [(248, 280), (368 + 4 * 25, 368 + 4 * 28)]


def raw_state(m):
    """every env's whole block (header, agent records, open orders, RNG streams, saved queue and
    book, transaction ring) with the launch-local header words zeroed"""
    out = []
    for i in range(m.n_envs):
        b = m.raw(i, 0, m.env_bytes).copy()
        for lo, hi in HDR_LAUNCH_LOCAL:
            b[lo:hi] = 0
        out.append(b)
    return out


def test_gpu_chunked_launches_cut_the_group_at_every_position(mx):
    """three market-maker cycles (open + 1, 2, 3 s) under launch budgets of 1-7 and 64 pops: the
    five-pop group is cut at every position, and each cut takes the queued path from there; the
    env blocks end byte for byte as the one-launch run's"""
    stop = OPEN + 3 * NS
    one = run_to(mx, stop)
    assert_oracle(one, stop)
    want, raw = records(one), raw_state(one)
    for c in (1, 2, 3, 4, 5, 6, 7, 64):
        m = run_to(mx, stop, chunk=c)
        assert records(m) == want, c
        assert (m.summary()["max_queue"] == one.summary()["max_queue"]).all(), c
        for e, (a, b) in enumerate(zip(raw_state(m), raw)):
            assert np.array_equal(a, b), (c, e, np.nonzero(a != b)[0][:16].tolist())


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_gpu_stop_time_at_a_market_maker_wake(mx, off):
    stop = OPEN + 2 * NS + off
    assert_oracle(run_to(mx, stop), stop)
    assert_oracle(run_to(mx, stop, chunk=3), stop)


def test_gpu_instant_shared_with_the_momentum_agents(mx):
    """open + 20 s: the momentum agents wake on the market maker's nanosecond (the queued path)"""
    stop = OPEN + 21 * NS
    assert_oracle(run_to(mx, stop), stop)


VALUE_STOP = OPEN + 120 * NS


def test_gpu_value_agent_wakes_with_an_open_order(mx):
    """by VALUE_STOP some value agent of every env has woken with an order still resting (its
    wakeup is followed at once by its CANCEL_ORDER at the exchange): read off the oracle's trace"""
    for sd in SEEDS:
        o = pyoracle.OracleEnv("rmsc03", sd, trace_cap=1 << 20)
        o.set_stop(VALUE_STOP)
        o.run()
        tr = np.asarray(o.trace())
        wake = (tr[:-1, 2] == MT_WAKEUP) & np.isin(tr[:-1, 1], list(VALUE))
        canc = (tr[1:, 2] == MT_MESSAGE) & (tr[1:, 1] == 0) & (tr[1:, 3] == MK_CANCEL) & (tr[1:, 0] == tr[:-1, 0])
        assert (wake & canc).any(), sd
    assert_oracle(run_to(mx, VALUE_STOP), VALUE_STOP)
    assert_oracle(run_to(mx, VALUE_STOP, chunk=5), VALUE_STOP)


def test_gpu_whole_episode_and_high_water_mark(mx):
    """the whole episode, with the queue's high-water mark against the oracle's capacity statistics"""
    m = run_to(mx, None)
    assert_oracle(m, None)
    st = pyoracle.batch_stats("rmsc03", np.array(SEEDS, dtype=np.uint32), 8)
    assert (m.summary()["max_queue"] == st[:, 0]).all(), (m.summary()["max_queue"], st[:, 0])


def test_gpu_step_kernel(mx):
    """rmsc03 + DummyRL, 27 steps: k steps in one launch equal one-step launches and the oracle"""
    from mxabides.gym import ACTION_SIZE, OBS_SIZE, VecABIDESEnv
    n, k = len(SEEDS), 27
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


def test_gpu_outside_the_mask_runtime_market_maker_options(mx):
    """rmsc03 with per-env market-maker options (scripts/rmsc03.sh: a 102-order ladder every 10 s)"""
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


def test_gpu_counters_equal_the_queued_build(mx):
    """mxa_read_counters of an instrumented episode: per-kind pops, requeues, record round trips and
    run members as the build without the in-place path counted them (tests/golden/sync_query_counters.json,
    taken on the parent commit)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "sync_query_counters.json")) as f:
        ref = json.load(f)
    assert ref["seeds"] == SEEDS
    m = run_to(mx, None)
    assert m.counters().tolist() == ref["counters"]
