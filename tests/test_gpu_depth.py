"""mxa_write_depth / mxa_read_depth (include/mxa_depth.h): the top k price levels of every env's book in
one launch, on every handle kind and both book formats, exact against two independent references:
the handle's own host reader book() (which other tests pin against oracle and fixtures) and the C
oracle advanced to the same pop count (events and book() are asserted equal to the oracle's first).
The facts about the books at each cut were computed with the oracle on the CPU; the tests assert them
as preconditions, so none passes on an empty or trivial book."""
import os

import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process (the device buffers)

import pyoracle
import synth_tapes as S
from depth_util import check_depth, device_depth, handle_books, refs_of
from golden_util import market_kw
from mxabides.gym import VecABIDESEnv
from test_gpu_partial_reset import RL_SEEDS, SEEDS, SHAPES, cut_rmsc03
from test_synth_tapes import walk

pytestmark = pytest.mark.gpu

KS = [1, 2, 10, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


_ORA = {}


def oracle_at(cfg, seed, pops):
    """(events, bids, asks) of the oracle after `pops` pops (or at its end, if that comes first)"""
    key = (cfg, seed, pops)
    if key not in _ORA:
        o = pyoracle.OracleEnv(cfg, seed)
        o.run(pops)
        assert o.error[0] == 0, o.error
        _ORA[key] = (o.events, o.book(0), o.book(1))
    return _ORA[key]


def assert_at_oracle(m, cfg, seeds, pops):
    """the handle stands where the oracle stands after `pops` pops: events and both book sides, order for
    order; returns the oracle's books"""
    s = m.summary()
    books = []
    for e, sd in enumerate(seeds):
        ev, bids, asks = oracle_at(cfg, int(sd), pops)
        assert int(s["events"][e]) == ev, (e, int(s["events"][e]), ev)
        assert m.book(e, 0) == bids and m.book(e, 1) == asks, e
        books.append((bids, asks))
    return books


def n_levels(books):
    return [len(side) for b in books for side in b]


def has_multi(sides):
    return any(len(lv) >= 2 for side in sides for lv in side)


def check_both(m, ks, oracle_books):
    """every k against the handle's book() and against the oracle's book"""
    own = handle_books(m)
    for k in ks:
        check_depth(m, k, refs_of(own, k))
        check_depth(m, k, refs_of(oracle_books, k))


def test_gpu_depth_rmsc03_cut_end_and_reset(mx):
    """rmsc03 x8 at the 15,000-pop cut (two envs ended, six mid-episode), at the end, and after reset()"""
    m = cut_rmsc03(mx)
    books = assert_at_oracle(m, "rmsc03", SEEDS, 15000)
    lv = {sd: (len(b[0]), len(b[1])) for sd, b in zip(SEEDS, books)}
    assert lv[123456789] == (5, 11) and lv[1008] == (2, 6) and lv[13] == (2, 4), lv
    st = m.summary()["status"]
    assert st[SEEDS.index(1008)] == 1 and st[SEEDS.index(13)] == 1 and (st == 0).sum() == 6, st
    assert min(n_levels(books)) < 10 < max(n_levels(books)), lv  # k = 10: zero-fill and truncation in one call
    assert all(has_multi(b) for b in books)  # every env sums some level of two or more orders
    check_both(m, KS, books)
    m.run()
    assert (m.summary()["status"] == 1).all()
    check_both(m, [1, 10, 64], assert_at_oracle(m, "rmsc03", SEEDS, -1))
    m.reset()
    for k in (1, 10, 65):
        rows, counts = device_depth(m, k)
        assert not counts.any() and not rows.any()
        h_rows, h_counts = m.depth(k)
        assert not h_counts.any() and not h_rows.any()
    assert m.inside(0, 10) == ([], [])


SIZE_SEEDS = [3, 7, 1, 2, 5, 11, 13, 123456789]


@pytest.mark.parametrize("n", [1, 5, 8])
def test_gpu_depth_handle_sizes(mx, n):
    """handles of 1, 5 and 8 envs after one launch of 3,000 pops"""
    seeds = SIZE_SEEDS[:n]
    m = mx.VecMarket("rmsc03", seeds)
    m.set_parity_hash(True)
    assert m.run(chunk=3000, max_launches=1) == 1
    books = assert_at_oracle(m, "rmsc03", seeds, 3000)
    assert len(books[0][1]) == 3 and has_multi(books[0])  # seed 3: an ask side of 3 levels
    if n > 1:
        assert len(books[1][1]) == 6 and all(has_multi(b) for b in books[:4])  # seed 7: 6 ask levels
    check_both(m, [1, 10], books)


# pops to run on to after the cut: the oracle's books of the two 5,101-agent markets are still empty at
# their cuts (the first 20,000 pops are wakeups), so there the cut checks the empty answer and the
# later stop the levels: at 80,000 pops the oracle has 44-96 levels a side, some of several orders
MORE = {"random_fund_value": (35000, 2), "random_fund_diverse": (25000, 3)}  # (chunk, launches) to 80,000 pops


@pytest.mark.parametrize("cfg,chunk,launches", SHAPES + [("random_fund_diverse", 5000, 1)])
def test_gpu_depth_other_slot_book_shapes(mx, cfg, chunk, launches):
    """slot books of 13 (sparse_zi_1000) and 7 (random_fund_diverse) slots a lane and the other queue
    shapes, 2 envs mid-episode.  The oracle-at-pops precondition holds on all four (random_fund_diverse
    too), so both references are used everywhere."""
    seeds = [123456789, 5]
    m = mx.VecMarket(cfg, seeds, **market_kw(cfg))
    m.set_parity_hash(True)
    assert m.run(chunk=chunk, max_launches=launches) == launches
    pops = chunk * launches
    s = m.summary()
    assert (s["status"] == 0).all() and (s["events"] == pops).all(), s
    books = assert_at_oracle(m, cfg, seeds, pops)
    if cfg in MORE:
        assert max(n_levels(books)) == 0  # nobody has placed an order yet: counts 0, every row zero
        check_both(m, [1, 10, 64], books)
        chunk2, launches2 = MORE[cfg]
        assert m.run(chunk=chunk2, max_launches=launches2) == launches2
        pops += chunk2 * launches2
        assert pops == 80000
        s = m.summary()
        assert (s["status"] == 0).all() and (s["events"] == pops).all(), s
        books = assert_at_oracle(m, cfg, seeds, pops)
    assert min(n_levels(books)) > 10 and all(has_multi(b) for b in books), n_levels(books)
    check_both(m, [1, 10, 64], books)


def walk_sides(name, pops):
    """the oracle's (bids, asks) after `pops` pops of a runner tape as [(price, total, orders)]"""
    _, bids, asks, _ = walk(name)[0][pops - 1]
    return bids, asks


def walk_refs(name, pops, n_envs, k):
    rows = np.zeros((n_envs, 2, k, 2), dtype=np.int64)
    counts = np.zeros((n_envs, 2), dtype=np.int32)
    for s, side in enumerate(walk_sides(name, pops)):
        c = min(k, len(side))
        counts[:, s] = c
        if c:
            rows[:, s, :c] = np.array([(p, q) for p, q, _ in side[:c]], dtype=np.int64)
    return rows, counts


GAPS = [1, 63, 64, 65, 127, 128, 129, 1500]


def tape_preconditions(name):
    """what the oracle's walk holds at the pops the tapes were crafted for"""
    if name == "ladder_gaps":
        for pops, s in ((38, 0), (96, 1)):
            side = walk_sides(name, pops)[s]
            assert len(side) == 9 and [abs(side[i + 1][0] - side[i][0]) for i in range(8)] == GAPS
    elif name == "ladder_ends":
        bids = walk_sides(name, 23)[0]
        assert len(bids) == 2 and bids[0][0] - bids[1][0] == 1_000_000
        asks = walk_sides(name, 35)[1]
        assert len(asks) == 3 and asks[1][0] - asks[0][0] == 1_048_570 and asks[2][0] == (1 << 20) - 1
    elif name == "fills":
        assert any(q == 6_442_450_938 and n == 3 for side in walk_sides(name, 103) for _, q, n in side)
    elif name == "fifo_chain":
        assert any(n == 5 for side in walk_sides(name, 23) for _, _, n in side)


@pytest.mark.parametrize("name,pops", [("ladder_gaps", 237), ("ladder_ends", 49), ("fills", 125), ("fifo_chain", 103)])
def test_gpu_depth_ladder_pop_by_pop(mx, name, pops):
    """the replay ladder on a crafted tape, checked after every pop (one-pop launches) against the
    oracle's walk and the handle's book()"""
    tape_preconditions(name)
    assert len(walk(name)[0]) == pops
    tp = S.RUNNER_TAPES[name]()[0]
    n_envs = 2 if name == "ladder_ends" else 3  # ladder_ends: P = 2^20, the widest ladder
    m = mx.VecMarket("marketreplay_runner", np.zeros(n_envs, dtype=np.int64), tape=tp, symbol=tp.symbol)
    for k in (1, 3):
        rows, counts = device_depth(m, k)  # before the first pop
        assert not rows.any() and not counts.any()
    for p in range(1, pops + 1):
        assert m.run(chunk=1, max_launches=1) == 1
        assert (m.summary()["events"] == p).all()
        own = handle_books(m, [0])
        sides = walk_sides(name, p)
        for s in (0, 1):  # book() is where the oracle is: (price, total, orders) level by level
            assert [(lv[0][3], sum(o[2] for o in lv), len(lv)) for lv in own[0][s]] == sides[s], (p, s)
        for k in (1, 3):
            got, _ = check_depth(m, k, walk_refs(name, p, n_envs, k))
            assert np.array_equal(got[:1], refs_of(own, k)[0])
    m.run()
    assert (m.summary()["status"] == 1).all() and (m.summary()["events"] == pops).all()


def test_gpu_depth_ladder_groups(mx):
    """`groups` (1,808 pops, 52 x 50 levels near its end) at 8 evenly spaced cuts and at the end, k up to
    65: more rows than a wave stores at once, and a count between 32 and 64"""
    name, pops = "groups", 1808
    out = walk(name)[0]
    assert len(out) == pops and (len(out[-1][1]), len(out[-1][2])) == (52, 50)
    tp = S.RUNNER_TAPES[name]()[0]
    m = mx.VecMarket("marketreplay_runner", np.zeros(3, dtype=np.int64), tape=tp, symbol=tp.symbol)
    cuts = [pops * i // 9 for i in range(1, 9)] + [pops]
    at, seen = 0, []
    for c in cuts:
        assert m.run(chunk=c - at, max_launches=1) == 1
        at = c
        assert (m.summary()["events"] == c).all()
        own = handle_books(m)
        seen.append((len(own[0][0]), len(own[0][1])))
        for k in (1, 3, 64, 65):
            check_depth(m, k, walk_refs(name, c, 3, k))
            check_depth(m, k, refs_of(own, k))
    assert seen[-1] == (52, 50) and max(max(x) for x in seen[:-1]) > 3, seen
    m.run()
    assert (m.summary()["status"] == 1).all()
    for k in (1, 64):
        check_depth(m, k, refs_of(handle_books(m), k))


def gym_steps_then_fork(v, acts):
    for a in acts:
        v.step(a)
        own = handle_books(v)
        assert max(n_levels(own)) > 1
        check_depth(v, 10, refs_of(own, 10))
    # the other envs start over (empty books; the replay's envs would otherwise all hold the tape's book:
    # DummyRL's first order comes after these steps), so the fork below has something to overwrite
    v.reset(mask=[0] + [1] * (v.n_envs - 1))
    rows0, counts0 = device_depth(v, 10)
    assert counts0[0].max() > 1 and not counts0[1:].any() and not rows0[1:].any()
    v.fork(0)
    rows, counts = check_depth(v, 10, refs_of(handle_books(v), 10))
    for e in range(v.n_envs):
        assert np.array_equal(rows[e], rows0[0]) and np.array_equal(counts[e], counts0[0]), e


def gym_actions(n, steps=5):
    rs = np.random.RandomState(29)
    acts = np.stack([rs.uniform(0.01, 0.05, (steps, n)) * np.arange(1, n + 1), rs.uniform(0, 1, (steps, n)),
                     rs.uniform(0, 1, (steps, n))], 2)
    return acts


def test_gpu_depth_gym_replay_and_fork():
    """the GymKernel replay handle (IBM 2003-01-14) x4: 5 steps with a different action per env, k = 10
    after each step against book(); after fork(0) every env reports env 0's rows"""
    from mxabides import tape
    tp = tape.Tape.load(os.path.join(os.path.dirname(__file__), "golden", "tape_IBM_2003-01-14.npz"))
    gym_steps_then_fork(VecABIDESEnv(tp, 4), gym_actions(4))


def test_gpu_depth_gym_rmsc03_rl_and_fork():
    """the same on rmsc03 + DummyRL x4 (the slot book of a GymKernel handle)"""
    gym_steps_then_fork(VecABIDESEnv(seeds=RL_SEEDS), gym_actions(4))


def test_gpu_depth_is_ordered_on_the_handles_stream(mx):
    """launch, write_depth, launch, write_depth with one sync at the end: each write sees the books as
    the launch queued before it leaves them, and mxa_read_depth after that equals the second"""
    k, n = 10, len(SEEDS)
    ref = mx.VecMarket("rmsc03", SEEDS)
    ref.set_parity_hash(True)
    want = []
    for pops in (5000, 10000):
        assert ref.run(chunk=5000, max_launches=1) == 1
        books = assert_at_oracle(ref, "rmsc03", SEEDS, pops)
        want.append(refs_of(books, k))
        check_depth(ref, k, want[-1])
    assert not np.array_equal(want[0][0], want[1][0])  # the books moved between the two cuts
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    bufs = [torch.full((n, 2, k, 2), -3, dtype=torch.int64, device="cuda") for _ in range(2)]
    cnts = [torch.full((n, 2), -3, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        m.launch(5000)
        m.write_depth(k, bufs[i].data_ptr(), cnts[i].data_ptr())
    m.sync()
    for i in range(2):
        assert np.array_equal(bufs[i].cpu().numpy(), want[i][0]), i
        assert np.array_equal(cnts[i].cpu().numpy(), want[i][1]), i
    rows, counts = m.depth(k)
    assert np.array_equal(rows, want[1][0]) and np.array_equal(counts, want[1][1])


def test_gpu_depth_refusals_on_a_live_handle(mx):
    """levels 0, -1 and 2^20 + 1 and a null depth pointer are MxaError with the message, and leave the
    buffers alone; a NULL counts pointer is accepted"""
    m = mx.VecMarket("rmsc03", SEEDS[:2])
    m.run(chunk=3000, max_launches=1)
    buf = torch.full((2, 2, 4, 2), -3, dtype=torch.int64, device="cuda")
    cnt = torch.full((2, 2), -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for levels, what in ((0, "levels < 1"), (-1, "levels < 1"), ((1 << 20) + 1, "levels > 1 << 20")):
        with pytest.raises(mx.MxaError, match="mxa_write_depth.*" + what):
            m.write_depth(levels, buf.data_ptr(), cnt.data_ptr())
        with pytest.raises(mx.MxaError, match="mxa_read_depth.*" + what):
            m.depth(levels)
    with pytest.raises(mx.MxaError, match="mxa_write_depth.*null depth"):
        m.write_depth(4, 0, cnt.data_ptr())
    host_counts = np.zeros((2, 2), dtype=np.int32)
    rc = m.L.mxa_read_depth(m._h, 4, None, host_counts.ctypes.data)
    assert rc == -1 and b"null depth" in m.L.mxa_last_error(m._h) and not host_counts.any()
    m.sync()
    assert (buf.cpu().numpy() == -3).all() and (cnt.cpu().numpy() == -3).all()
    own = handle_books(m)
    rows, none = device_depth(m, 4, counts=False)  # (asserts the counts array untouched)
    assert none is None and np.array_equal(rows, refs_of(own, 4)[0])
    host_rows = np.full((2, 2, 4, 2), -3, dtype=np.int64)
    assert m.L.mxa_read_depth(m._h, 4, host_rows.ctypes.data, None) == 0
    assert np.array_equal(host_rows, rows)
