"""The value agents' resting orders and their acknowledgements in the wake's own pop
(Eng::value_order): after an in-place value wake the agent's
LIMIT_ORDER is the forced next pop, and if it rests, so is its ORDER_ACCEPTED.  Both ride in the
wakeup's pop when the order rests on a book whose two insides the spread reply showed, the book has
a free slot and the launch budget holds the two pops; a crossing order, a one-sided book, a full
book and a budget that cuts the group take the queued path.  mxa_read_inplace word 4 counts the
orders taken; every other observable is the queued sequence's.

The window, the seeds (two stalled market makers: one-sided books) and the helpers are those of
test_gpu_limit_inplace.py, whose oracle traces are computed once per process and shared.  Each test
first asserts from the oracle's trace that its window holds the case it names."""
import json
import os

import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process

import pyoracle
import test_gpu_limit_inplace as W
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu

SEEDS, VALUE, WINDOW, OPEN, NS = W.SEEDS, W.VALUE, W.WINDOW, W.OPEN, W.NS
MT_MESSAGE, MT_WAKEUP = W.MT_MESSAGE, W.MT_WAKEUP
MK_SPREAD_REQ, MK_SPREAD, MK_LIMIT, MK_CANCEL, MK_ACCEPTED, MK_CANCELLED = 5, 6, 11, 12, 14, 16
ERR_BOOK_FULL = 2  # the device's code (mxa_env_summary.err)


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def value_orders(tr, agents=VALUE):
    """every value agent's LIMIT_ORDER pop of trace `tr`: (index, t, agent, rests, behind, both).
    rests: the next pop is its ORDER_ACCEPTED (nothing executed).  behind: the order pops directly
    behind its agent's wake group at the same nanosecond (wakeup, [CANCEL_ORDER,] QUERY_SPREAD,
    [ORDER_CANCELLED,] spread reply, with nothing between).  both: that reply showed a bid and an ask"""
    out = []
    msg = tr[:, 2] == MT_MESSAGE
    for i in np.nonzero(msg & (tr[:, 1] == 0) & (tr[:, 3] == MK_LIMIT) & np.isin(tr[:, 5], list(agents)))[0]:
        t, ag, oid = tr[i, 0], int(tr[i, 5]), tr[i, 4]

        def is_msg(j, rcp, kind):
            return j >= 0 and tr[j, 0] == t and tr[j, 2] == MT_MESSAGE and tr[j, 1] == rcp and tr[j, 3] == kind

        nx = i + 1
        rests = nx < len(tr) and is_msg(nx, ag, MK_ACCEPTED) and tr[nx, 4] == oid
        j = i - 1
        behind = is_msg(j, ag, MK_SPREAD)
        both = bool(behind and tr[j, 4] != -1 and tr[j, 6] != -1)
        if behind:
            j -= 1
            cancelled = is_msg(j, ag, MK_CANCELLED)
            j -= int(cancelled)
            behind = is_msg(j, 0, MK_SPREAD_REQ) and tr[j, 4] == ag
            j -= 1
            if behind and is_msg(j, 0, MK_CANCEL) and tr[j, 5] == ag:
                j -= 1
            else:
                behind = behind and not cancelled
            behind = bool(behind and j >= 0 and tr[j, 0] == t and tr[j, 2] == MT_WAKEUP and tr[j, 1] == ag)
        out.append((int(i), int(t), ag, bool(rests), behind, both))
    return out


def test_gpu_resting_value_orders_are_taken_in_place(mx):
    """open + 60 s, one launch: the run equals the oracle, and word 4 of mxa_read_inplace equals the
    oracle trace's count of value LIMIT_ORDERs that rest, pop directly behind their agent's wake
    group and are directly followed by their ORDER_ACCEPTED.  One legitimate fallback class occurs in
    the window and is counted from the trace too: a reply that shows one side only (the envs whose
    market maker is stalled), where the order is sent as an event although it rests.  Crossing orders
    are in the window as well and stay queued"""
    want = onesided = crossing = 0
    for sd, tr, out in zip(SEEDS, W.traces(), W.orders()):
        vo = value_orders(tr)
        assert len(vo) == sum(1 for t, ag, k in out if ag in VALUE), sd
        assert all(r == (k == "rest") for (i, t, ag, r, b, s), (t2, ag2, k) in
                   zip(vo, [x for x in out if x[1] in VALUE])), sd  # W.orders()' kind "rest"
        want += sum(1 for i, t, ag, r, b, s in vo if r and b and s)
        onesided += sum(1 for i, t, ag, r, b, s in vo if r and b and not s)
        crossing += sum(1 for i, t, ag, r, b, s in vo if not r and b)
    print("value orders behind their group: %d rest (two-sided), %d rest (one-sided reply), %d cross" % (want, onesided, crossing))
    assert want > 0 and onesided > 0 and crossing > 0, (want, onesided, crossing)
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    m.set_stop_time(WINDOW)
    m.inplace_groups()  # clear what earlier runs of this process left
    m.run()
    W.assert_oracle(m, WINDOW)
    g = m.inplace_groups().astype(np.int64)
    print("in-place groups", g.tolist())
    assert g[4] == want, (g.tolist(), want, onesided)
    assert 0 < g[4] <= g[1] and g[3] == 0 and g[5] == 0, g.tolist()


def test_gpu_counters_equal_the_queued_paths(mx):
    """the one-launch run's event-class counters and env blocks equal those of a run whose 4-pop
    budgets force every group onto the queue (a value group with its order is 5 pops at least): pops
    per kind, pushes, RNG words, high-water marks, seqs, the open-order lists, the book"""
    n = sum(1 for tr in W.traces() for i, t, ag, r, b, s in value_orders(tr) if r and b and s)
    assert n > 0
    one = W.run_to(mx, WINDOW)
    W.assert_oracle(one, WINDOW)
    cut = W.run_to(mx, WINDOW, chunk=4)
    W.assert_oracle(cut, WINDOW)
    a, b = one.counters(), cut.counters()
    assert (a[:, :31] == b[:, :31]).all(), np.nonzero(a[:, :31] != b[:, :31])
    W.assert_same_blocks(W.raw_state(cut), W.raw_state(one), "chunk=4")


def neighbours():
    """(t, seed index) of a value order that crosses directly behind (the next value order of its
    env after) one taken in place, and of one taken in place directly behind one that crosses"""
    found = {}
    for e, tr in enumerate(W.traces()):
        vo = value_orders(tr)
        for (i0, t0, a0, r0, b0, s0), (i1, t1, a1, r1, b1, s1) in zip(vo, vo[1:]):
            if t1 <= OPEN + NS:
                continue
            if r0 and b0 and s0 and not r1 and b1:
                found.setdefault("cross_behind_rest", (t1, e))
            if not r0 and b0 and r1 and b1 and s1:
                found.setdefault("rest_behind_cross", (t1, e))
    return found


@pytest.mark.parametrize("case", ["cross_behind_rest", "rest_behind_cross"])
def test_gpu_crossing_and_resting_orders_back_to_back(mx, case):
    """a window that ends at the instant of a crossing value order whose predecessor (the env's
    previous value order) was taken in place, and at the instant of an in-place one whose
    predecessor crossed: the book (both sides, FIFO order within a level), every agent's cash,
    holdings and open orders and the order counter equal the oracle's"""
    found = neighbours()
    assert case in found, (case, "not in the window")
    t, e = found[case]
    m = W.run_to(mx, t)
    W.assert_oracle(m, t)
    for i, sd in enumerate(SEEDS):
        o = pyoracle.OracleEnv("rmsc03", sd)
        o.set_stop(t)
        o.run()
        assert m.book(i, 0) == o.book(0) and m.book(i, 1) == o.book(1), (case, sd)
        assert int(m.summary()["order_counter"][i]) == o.order_counter, (case, sd)
        assert [(a["cash"], a["shares"], a["n_open"]) for a in m.agents(i)[1:]] == o.agents()[1:], (case, sd)


_BOOK = {}


def book_room():
    """tests/golden/cap_rmsc03_b.json (rmsc03 with 18 value agents, 64 book slots: the smallest a
    composition allows) under the oracle with the engine's capacities, once: no cap_*.json whose
    book fills has value agents, and plain rmsc03 peaks at 55-59 resting orders"""
    if not _BOOK:
        from mxabides import composition as C
        with open(os.path.join(GOLDEN, "cap_rmsc03_b.json")) as f:
            cfg = C.from_dict(json.load(f)["composition"])
        cap = C.capacities(cfg)
        seeds = np.array(SEEDS, dtype=np.uint32)
        ev, hs, er, _, st = pyoracle.run_batch_config(cfg, seeds, 8, stats=True)
        cev, chs, cer, _ = pyoracle.run_batch_config(cfg, seeds, 8, capacities=cap)
        _BOOK.update(cfg=cfg, cap=cap, seeds=seeds, peak=st[:, 1], ev=ev, hs=hs, cev=cev, chs=chs, cer=cer)
    return _BOOK


def test_gpu_full_book_fails_in_the_queued_pop(mx):
    """a book of 64 slots that the oracle's peaks straddle: an env that ends exactly full passes with
    the uncapped hash and its 64th order in place or queued alike; the env that needs a 65th slot
    stops with ERR_BOOK_FULL at the oracle's pop with the oracle's hash.  That pop is a value agent's
    resting LIMIT_ORDER directly behind its wake group: with no free slot the order is sent as an
    event and fails where the reference's sequence does"""
    B = book_room()
    assert B["cap"] == (192, 64), B["cap"]
    peak, cer = B["peak"], B["cer"]
    print("peaks", peak.tolist(), "oracle err", cer.tolist(), "events", B["cev"].tolist())
    assert (peak == 64).any() and (peak == 65).any(), peak
    assert ((cer == pyoracle.ERR_BOOK_FULL) == (peak > 64)).all() and ((cer == 0) == (peak <= 64)).all(), (cer, peak)
    for e in np.nonzero(peak > 64)[0]:  # the failing pop, from the capacity-aware oracle's trace
        o = pyoracle.OracleEnv(B["cfg"], int(B["seeds"][e]), trace_cap=1 << 18, capacities=B["cap"])
        o.run()
        tr = np.asarray(o.trace())
        assert len(tr) == o.events == B["cev"][e]
        i, t, ag, rests, behind, both = value_orders(tr, agents=range(51, 69))[-1]
        assert i == len(tr) - 1 and behind and both, (i, len(tr), behind, both)  # (no reply: the env stopped)
    m = mx.VecMarket(B["cfg"], B["seeds"])
    m.set_parity_hash(True)
    m.inplace_groups()
    m.run()
    s = m.summary()
    g = m.inplace_groups().astype(np.int64)
    print("in-place groups", g.tolist(), "status", s["status"].tolist(), "err", s["err"].tolist(), "max_book", s["max_book"].tolist())
    assert (s["status"] == np.where(cer == 0, 1, 2)).all(), s["status"]
    assert (s["err"] == np.where(cer == 0, 0, ERR_BOOK_FULL)).all(), s["err"]
    assert (s["events"] == B["cev"]).all() and (s["hash"] == B["chs"]).all()
    ok = cer == 0
    assert (s["events"][ok] == B["ev"][ok]).all() and (s["hash"][ok] == B["hs"][ok]).all()
    assert (s["max_book"][ok] == peak[ok]).all() and (s["max_book"] <= 64).all(), s["max_book"]
    assert g[4] > 0


def test_gpu_step_kernel(mx):
    """rmsc03 + DummyRL over the window (3 steps: to 09:31:00, :30, 09:32:00): three steps in one
    launch equal one-step launches bit for bit and the oracle, and the step kernel took value orders
    in place (the oracle's run of the same seeds and actions holds value orders that rest behind
    their wake group: the background agents are rmsc03's, seed for seed)"""
    from mxabides.gym import ACTION_SIZE, OBS_SIZE, VecABIDESEnv
    assert sum(1 for tr in W.traces() for i, t, ag, r, b, s in value_orders(tr) if r and b and s) > 0
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
    a.inplace_groups()  # clear
    for i in range(k):
        a.step_device(act[i].data_ptr(), obs_a[i].data_ptr(), flg_a[i].data_ptr())
    torch.cuda.synchronize()
    ga = a.inplace_groups().astype(np.int64)
    b.step_many_device(k, act.data_ptr(), obs_b.data_ptr(), flg_b.data_ptr())
    torch.cuda.synchronize()
    gb = b.inplace_groups().astype(np.int64)
    print("in-place groups: one-step launches", ga.tolist(), "one launch", gb.tolist())
    assert torch.equal(flg_a, flg_b)
    assert torch.equal(obs_a.view(torch.int64), obs_b.view(torch.int64))  # bit for bit
    sa, sb = a.summary(), b.summary()
    for key in ("events", "hash", "status", "err", "current_time", "order_counter"):
        assert (sa[key] == sb[key]).all(), key
    assert (sb["events"] == r["events"]).all() and (sb["hash"] == r["hash"]).all(), (sb["events"], r["events"])
    assert 0 < gb[4] <= gb[1] and 0 < ga[4] <= ga[1], (ga.tolist(), gb.tolist())
