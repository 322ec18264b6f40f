"""mxa_write_bars / mxa_read_bars / mxa_bars_from_records (include/mxa_bars.h) on the device, exact against
the tests' own reference bars_util.bars_ref (which tests/test_bars_host.py pins to
mxabides.booklog.rows_from_records on the oracle's streams): crafted streams at the kernel's edges
through the parity entry, several envs of different lengths a launch with guard words around both
outputs, and the handles that carry a book-update log."""
import ctypes
import os

import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process (the device buffers)

from bars_util import OPEN_NS, bars_ref, recs
from mxabides import bars as mbars
from mxabides import booklog as bl

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
GARBAGE = -0x0123456789ABCDEF
S = 10**9
CAP = 1 << 20
M = bl.BL_MODIFY
RX, NT, PLACE = bl.BL_EV_RX, bl.BL_EV_NT, bl.BL_EV_PLACE


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def run_records(mx, streams, level_cap, t0, dt, n_bars, stride=None, counts=None, with_status=True):
    """one mxa_bars_from_records launch over `streams` (a REC_DTYPE array per env) into buffers that hold
    garbage between guard words: (bars [n][n_bars][12], status [n][4] or None) once the guards are seen
    intact.  Records past an env's count are garbage that would change every bar if read."""
    L = mx.load()
    n = len(streams)
    stride = stride or max(1, max(len(s) for s in streams))
    rec = np.zeros((n, stride), dtype=bl.REC_DTYPE)
    rec["t"], rec["price"], rec["qty"] = t0, 1, 7  # past the count: limit orders inside the grid
    for e, s in enumerate(streams):
        rec[e, :min(len(s), stride)] = s[:stride]
    cnt = np.asarray([len(s) for s in streams] if counts is None else counts, dtype=np.int32)
    d_rec = torch.from_numpy(rec.view(np.int32).reshape(n, stride, 4)).cuda()
    d_cnt = torch.from_numpy(cnt).cuda()
    words = n * n_bars * 12
    pad = 24  # guard words on either side: a multiple of two, so the array stays 16-byte aligned
    buf = torch.full((words + 2 * pad,), GUARD, dtype=torch.int64, device="cuda")
    buf[pad:pad + words] = GARBAGE
    st = torch.full((4 * n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    st[8:8 + 4 * n] = -7
    torch.cuda.synchronize()
    rc = L.mxa_bars_from_records(None, n, ctypes.c_void_p(d_rec.data_ptr()), stride, ctypes.c_void_p(d_cnt.data_ptr()),
                                 level_cap, t0, dt, n_bars, ctypes.c_void_p(buf.data_ptr() + 8 * pad),
                                 ctypes.c_void_p(st.data_ptr() + 32) if with_status else None)
    assert rc == 0, L.mxa_last_error(None)
    torch.cuda.synchronize()
    b, c = buf.cpu().numpy(), st.cpu().numpy()
    assert (b[:pad] == GUARD).all() and (b[pad + words:] == GUARD).all(), "a write outside the bars array"
    assert (c[:8] == 0x5A5A5A5A).all() and (c[8 + 4 * n:] == 0x5A5A5A5A).all(), "a write outside the status array"
    if not with_status:
        assert (c[8:8 + 4 * n] == -7).all(), "status written though the pointer was NULL"
    return b[pad:pad + words].reshape(n, n_bars, 12), (c[8:8 + 4 * n].reshape(n, 4) if with_status else None)


def check_records(mx, streams, level_cap, t0, dt, n_bars, stride=None, counts=None, names=None):
    bars, status = run_records(mx, streams, level_cap, t0, dt, n_bars, stride, counts)
    refs = []
    for e, s in enumerate(streams):
        cap = stride or max(1, max(len(x) for x in streams))
        want, wst = bars_ref(s, level_cap, t0, dt, n_bars, capacity=cap, count=len(s) if counts is None else counts[e])
        who = names[e] if names else e
        assert status[e].tolist() == wst.tolist(), (who, status[e].tolist(), wst.tolist())
        bad = np.flatnonzero((bars[e] != want).any(axis=1))
        assert not len(bad), (who, int(bad[0]), bars[e, bad[0]].tolist(), want[bad[0]].tolist())
        refs.append((want, wst))
    return bars, status, refs


def gen(n, seed, t_start, t_step, noise=True):
    """a valid stream of exactly n records: limit orders that rest, cross and sweep, cancellations of
    live levels (partial and whole), with f_log and exchange-log code records between them"""
    rs = np.random.RandomState(seed)
    sides = ({}, {})
    out, t = [], t_start
    while len(out) < n:
        t += int(rs.randint(0, t_step))
        k = rs.randint(0, 10)
        left = n - len(out)
        if noise and k == 0:
            out.append((t + 5 * t_step, bl.BL_FUNDAMENTAL, int(rs.randint(90000, 110000))))  # f_log: a later time
        elif noise and k == 1 and left >= 2:
            out.append((t, NT + 14 + int(rs.randint(0, 3)), 3))
            out.append(((bl.FILL_NONE << 32) | int(rs.randint(1, 1000)), int(rs.randint(95, 105)), int(rs.choice([-5, 5]))))
        elif noise and k == 2:
            out.append((t, RX + int(rs.choice([5, 7, 9])), 4))
        elif k in (3, 4) and (sides[0] or sides[1]):
            s = 0 if sides[0] and (not sides[1] or rs.randint(2)) else 1
            p = int(rs.choice(sorted(sides[s])))
            q = sides[s][p] if rs.randint(2) else int(rs.randint(1, sides[s][p] + 1))
            sides[s][p] -= q
            if not sides[s][p]:
                del sides[s][p]
            out.append((t, -p, q if s == 0 else -q))
        else:
            buy = bool(rs.randint(2))
            p, q = int(rs.randint(90, 111)), int(rs.randint(1, 40))
            out.append((t, p, q if buy else -q))
            own, opp = (sides[0], sides[1]) if buy else (sides[1], sides[0])
            while q and opp:
                best = min(opp) if buy else max(opp)
                if (best > p) if buy else (best < p):
                    break
                c = min(q, opp[best])
                q -= c
                opp[best] -= c
                if not opp[best]:
                    del opp[best]
            if q:
                own[p] = own.get(p, 0) + q
    return recs(out[:n])


T0, DT, NB = 1000, 10, 1200
END = T0 + NB * DT


def crafted():
    """name -> stream, for one launch on the grid (T0, DT, NB) with level_cap 192"""
    c = {}
    for n in (0, 1, 63, 64, 65, 128, 129, 257):
        c["count_%d" % n] = gen(n, 100 + n, T0, 40)
    # an order-carrying code in lane 63, its order record (a would-be sweep) first in the next chunk
    head = gen(63, 5, T0, 30, noise=False)
    t = int(head["t"].max())
    c["code_in_lane_63"] = np.concatenate([head, recs([(t, NT + 15, 2), ((101 << 32) | 7, 1, -1000), (t + 1, 100, 3), (t + 2, 100, -2)])])
    c["rx_limit_in_lane_63"] = np.concatenate([head, recs([(t, RX + 11, 2), (7, 200, 1000), (t + 1, 100, 3)])])
    c["code_ends_the_stream"] = np.concatenate([gen(127, 6, T0, 30, noise=False), recs([(END - 1, RX + 12, 2)])])
    # f_log and code records between book records
    c["noise_between"] = recs([(T0, 100, 5), (END + 7, bl.BL_FUNDAMENTAL, 1), (0, bl.BL_FUND_LO, 2), (0, bl.BL_FUND_HI, 3),
                               (T0 + 1, RX + 5, 1), (T0 + 1, PLACE, 9), (T0 + 2, 101, -5), (T0 + 3, NT + 14, 1),
                               (9, -100, 5), (T0 + 30, -100, 2)])
    # a limit order sweeping three levels and resting its remainder; then one emptying the whole other side
    c["sweeps"] = recs([(T0, 100, -3), (T0 + 1, 101, -2), (T0 + 2, 102, -4), (T0 + 3, 104, -1), (T0 + 15, 102, 12),
                        (T0 + 25, 200, 5), (T0 + 35, 90, -30), (T0 + 36, 95, 1)])
    # the best level cancelled, then the next best, on both sides
    c["cancel_best"] = recs([(T0, 100, 1), (T0, 99, 2), (T0, 98, 3), (T0, 101, -1), (T0, 102, -2), (T0, 103, -3),
                             (T0 + 10, -100, 1), (T0 + 20, -99, 2), (T0 + 30, -101, -1), (T0 + 40, -102, -2),
                             (T0 + 50, -98, 3), (T0 + 60, -103, -3)])
    # a 64th, 65th and 129th live level on one side (the second and third rows of slots), then sweeps through them
    up = [(T0 + i, 1000 + 3 * (i * 37 % 131), 1 + i) for i in range(131)]
    c["levels_131_bids"] = recs(up + [(T0 + 200, 1100, -2000), (T0 + 300, -1000, 1), (T0 + 400, 1, -100000)])
    c["levels_130_asks"] = recs([(T0 + i, 5000 + (i * 29 % 130), -(1 + i)) for i in range(130)] + [(T0 + 500, 5064, 900), (T0 + 900, 6000, 10**6)])
    # a level of three orders of 2^31 - 1 shares: its volume exceeds 2^32
    big = 2**31 - 1
    c["big_level"] = recs([(T0, 1000, big), (T0 + 1, 1000, big), (T0 + 2, 1000, big), (T0 + 15, 1000, -big), (T0 + 16, 999, -big),
                           (T0 + 30, -1000, big)])
    # modify records on both sides
    c["modifies"] = recs([(T0, 10, 5), (T0, 9, 5), (T0, 20, -6), (T0, 21, -6), (T0 + 10, -(10 | M), -2), (T0 + 20, -(20 | M | 1 << 29), 3),
                          (T0 + 30, -(9 | M), 7), (T0 + 40, -(21 | M | 1 << 29), -6), (T0 + 50, -(10 | M), -3), (T0 + 60, 10, -1),
                          (T0 + 70, 21, 4)])
    # the grid's edges
    c["grid_edges"] = recs([(T0 - 1, 50, 10), (T0, 60, -4), (T0 + DT - 1, 50, -2), (T0 + DT, 60, 1), (END - 1, -50, 8), (END, 70, 1),
                            (T0 + 50, 70, 1)])
    c["stops_at_the_end"] = recs([(T0 + 5, 50, 10), (END, 60, -4), (T0 + 6, 61, -4)])
    # gaps of 63, 64, 65 and 1,000 empty bars
    c["gaps"] = recs([(T0 + DT * b, 100 + b % 7, 1 + b % 5) for b in (0, 64, 129, 195, 1196)])
    c["before_t0"] = recs([(5, 50, 10), (T0 - 1, 60, -4), (0, 50, -3)])
    c["time_back"] = recs([(T0 + 55, 50, 10), (T0 + 54, 60, -4), (T0 + 59, 50, -3), (T0 + 60, 50, -1), (T0 + 59, 50, -1), (T0 - 5, 50, -1)])
    # status 3: a cancel of an absent level, a cancel larger than its level, a modify of an absent level
    base = [(T0, 10, 1), (T0 + 1, 11, 1), (T0 + 20, 12, 4)]
    c["cancel_absent"] = recs(base + [(T0 + 45, -13, 1), (T0 + 50, 9, 1)])
    c["cancel_absent_side"] = recs(base + [(T0 + 45, -12, -1), (T0 + 50, 9, 1)])
    c["cancel_too_large"] = recs(base + [(T0 + 45, -12, 5), (T0 + 50, 9, 1)])
    c["cancel_too_large_not_best"] = recs(base + [(T0 + 45, -10, 2), (T0 + 50, 9, 1)])
    c["modify_absent"] = recs(base + [(T0 + 45, -(13 | M), 1), (T0 + 50, 9, 1)])
    c["bad_before_t0"] = recs([(5, -13, 1), (T0, 10, 1)])
    c["long"] = gen(300, 77, T0, 80)
    return c


def test_gpu_bars_crafted_streams_one_launch(mx):
    """every crafted stream as one env of one launch (31 envs of different lengths, level_cap 192), the
    log-overflow env among them: count > rec_stride is code 1 and the bars of the first rec_stride records"""
    c = crafted()
    names = list(c)
    streams = [c[k] for k in names]
    assert max(len(s) for s in streams) == 300
    counts = [len(s) for s in streams]
    names.append("log_overflow")
    streams.append(c["long"])
    counts.append(305)
    bars, status, refs = check_records(mx, streams, 192, T0, DT, NB, stride=300, counts=counts, names=names)
    by = dict(zip(names, zip(bars, status)))
    # the crafted streams do what they were crafted for (facts of the reference, so of the device too)
    assert by["log_overflow"][1].tolist()[:2] == [1, 300] and np.array_equal(by["log_overflow"][0], by["long"][0])
    assert by["count_0"][1].tolist() == [0, 0, 0, 0] and not by["count_0"][0].any()
    assert by["code_in_lane_63"][1][0] == 0 and by["rx_limit_in_lane_63"][1][0] == 0
    assert by["levels_131_bids"][1].tolist() == [0, 134, 131, 1] and by["levels_130_asks"][1].tolist() == [0, 132, 1, 130]
    assert by["big_level"][0][0, 1] == 3 * (2**31 - 1) and by["big_level"][0][1, 8] == 2 * (2**31 - 1)
    assert by["sweeps"][0][1, 4:11].tolist() == [100, 102, 100, 102, 9, 3 * 100 + 2 * 101 + 4 * 102, 1]
    assert by["sweeps"][0][1, :4].tolist() == [102, 3, 104, 1] and by["sweeps"][0][2, :4].tolist() == [200, 4, 0, 0]
    assert by["sweeps"][0][3, :4].tolist() == [0, 0, 90, 22]
    assert [by["cancel_best"][0][i, 0] for i in range(7)] == [100, 99, 98, 98, 98, 0, 0]
    assert [by["cancel_best"][0][i, 2] for i in range(7)] == [101, 101, 101, 102, 103, 103, 0]
    assert by["grid_edges"][1].tolist() == [0, 5, 1, 1] and by["stops_at_the_end"][1].tolist() == [0, 1, 1, 0]
    assert by["gaps"][0][:, 11].sum() == 5 and by["gaps"][0][1196, 11] == 1 and (by["gaps"][0][1:64, 1] == 1).all()
    assert by["before_t0"][1].tolist() == [0, 3, 1, 1] and not by["before_t0"][0][:, 4:].any() and (by["before_t0"][0][:, 1] == 7).all()
    assert by["time_back"][0][5, 11] == 3 and by["time_back"][0][6, 11] == 3
    for k in ("cancel_absent", "cancel_absent_side", "cancel_too_large", "cancel_too_large_not_best", "modify_absent"):
        assert by[k][1].tolist() == [3, 3, 3, 0], k
        assert by[k][0][0, 11] == 2 and by[k][0][2, 11] == 1 and by[k][0][3, 0] == 12 and not by[k][0][4:].any(), k
    assert by["bad_before_t0"][1].tolist() == [3, 0, 0, 0] and not by["bad_before_t0"][0].any()
    assert by["modifies"][1][0] == 0 and by["noise_between"][1].tolist() == [0, 10, 1, 1]


def test_gpu_bars_level_cap_64_and_65(mx):
    """level_cap 64: 64 live levels a side are status 0, a 65th is status 2 with zero rows from the bar it
    falls in on and the earlier rows kept; level_cap 1 and 1024 too"""
    t0, dt, nb = 0, 100, 8
    sixty4 = [(i, 1000 + 2 * (i * 23 % 64), 1 + i) for i in range(64)]
    ok = recs(sixty4 + [(150, 1000, 5), (250, -1000, 6), (350, 2000, -10), (450, 1126, -70)])
    again = recs(sixty4 + [(250, -1002, 40), (350, 999, 1), (450, 998, 1)])  # 64, 63, 64 again, then a 65th
    over = recs(sixty4 + [(150, 5000, -1), (250, 999, 1), (350, 1000, -3)])
    asks = recs([(i, 3000 + i, -1) for i in range(65)] + [(700, 1, 1)])
    bars, status, _ = check_records(mx, [ok, again, over, asks], 64, t0, dt, nb)
    assert status.tolist() == [[0, 68, 64, 2], [2, 66, 64, 0], [2, 65, 64, 1], [2, 64, 0, 64]]
    assert bars[1][2, 11] == 1 and bars[1][3, 11] == 1 and not bars[1][4:].any()
    assert bars[2][0, 11] == 64 and bars[2][1, 11] == 1 and not bars[2][2:].any() and not bars[3].any()
    # the same streams fit a larger table
    _, status, _ = check_records(mx, [ok, again, over, asks], 1024, t0, dt, nb)
    assert (status[:, 0] == 0).all() and status[:, 2:].tolist() == [[64, 2], [65, 0], [65, 1], [1, 65]]
    _, status, _ = check_records(mx, [recs([(1, 10, 1), (2, 10, 1), (3, 11, -1), (4, 9, 1)]), recs([(1, 10, 1), (2, 12, -1), (3, 10, -1), (4, 9, 1)])],
                                 1, t0, dt, nb)
    assert status.tolist() == [[2, 3, 1, 1], [0, 4, 1, 1]]


def test_gpu_bars_level_cap_1024(mx):
    """the whole table: 1,024 live levels a side (16 slots a lane) are status 0, with cancellations in
    every row of slots, a sweep through all of them and levels placed again into freed slots; a 1,025th
    level is status 2"""
    t0, dt, nb = 0, 1000, 8
    n = 1024
    bids = [(i, 20000 + 5 * (i * 389 % n), 1 + i % 9) for i in range(n)]  # 389 is coprime to 1024: distinct prices
    asks = [(i, 40000 + 3 * (i * 611 % n), -(1 + i % 7)) for i in range(n)]
    qty_at = {p: q for _, p, q in bids}
    assert len(qty_at) == n and len({p for _, p, _ in asks}) == n
    full = recs(bids + asks + [(1500, -(20000 + 5 * k), qty_at[20000 + 5 * k]) for k in range(0, n, 37)]  # whole levels, every row
                + [(2500, 20000 + 5 * k, 3) for k in range(0, n, 74)] + [(3500, 50000, 10**6), (4500, 20000, -2 * 10**6), (5500, 30000, 5)])
    over_bid = recs(bids + [(2500, 19999, 1), (3500, 19998, 1)])
    over_ask = recs(asks + [(1500, -40000, -1), (2500, 39999, -1), (3500, 39998, -1), (4500, 39997, -1)])
    bars, status, _ = check_records(mx, [full, over_bid, over_ask], 1024, t0, dt, nb)
    assert status.tolist() == [[0, len(full), 1024, 1024], [2, 1024, 1024, 0], [2, 1026, 0, 1024]]
    # the bids' times 0 .. 999 fall in bar 0, 1000 .. 1023 in bar 1; the asks start over at time 0 and land in
    # bar 1 (the bar index never goes back), as do the 28 cancellations; 14 levels come back in bar 2
    assert bars[0][1, :4].tolist() == [20000 + 5 * 1023, qty_at[20000 + 5 * 1023], 40000, 1] and bars[0][0, 11] == 1000
    assert bars[0][1, 11] == 24 + 1024 + 28 and bars[0][2, 11] == 14
    assert bars[0][3, :4].tolist() == [50000, 10**6 - bars[0][3, 8], 0, 0] and bars[0][3, 8] == sum(-q for _, _, q in asks)
    assert bars[0][4, :4].tolist() == [0, 0, 20000, 2 * 10**6 - bars[0][4, 8]] and bars[0][4, 6] == 20000 and bars[0][4, 5] == 50000
    assert bars[0][5, :4].tolist() == [0, 0, 20000, 2 * 10**6 - bars[0][4, 8] - 5] and bars[0][5, 8:11].tolist() == [5, 100000, 1]
    assert bars[1][0, 11] == 1000 and bars[1][1, 11] == 24 and not bars[1][2:].any()
    assert bars[2][1, 11] == 25 and bars[2][2, 11] == 1 and not bars[2][3:].any()


def test_gpu_bars_one_bar_and_python_entry(mx):
    """n_bars = 1, a NULL status pointer, and mxabides.bars.from_records / mid / vwap on device tensors"""
    c = crafted()
    streams = [c["sweeps"], c["count_257"], c["count_0"], c["big_level"]]
    bars, _, refs = check_records(mx, streams, 192, T0, 10**6, 1)
    assert bars[0, 0].tolist() == [0, 0, 90, 22, 100, 200, 90, 90, 18, 2210, 4, 8]
    none_bars, none = run_records(mx, streams, 192, T0, 10**6, 1, with_status=False)
    assert none is None and np.array_equal(none_bars, bars)
    stride = 257
    rec = np.zeros((4, stride), dtype=bl.REC_DTYPE)
    for e, s in enumerate(streams):
        rec[e, :len(s)] = s
    d_rec = torch.from_numpy(rec.view(np.int32).reshape(4, stride, 4)).cuda()
    d_cnt = torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for st in (None, side):
        b, s = mbars.from_records(d_rec, d_cnt, 192, T0, DT, NB, stream=st)
        (st or torch.cuda.current_stream()).synchronize()
        assert b.shape == (4, NB, 12) and b.dtype == torch.int64 and s.shape == (4, 4) and s.dtype == torch.int32
        for e, x in enumerate(streams):
            want, wst = bars_ref(x, 192, T0, DT, NB)
            assert np.array_equal(b[e].cpu().numpy(), want) and s[e].cpu().numpy().tolist() == wst.tolist(), e
    mid, vw = mbars.mid(b), mbars.vwap(b)
    assert mid.shape == vw.shape == (4, NB) and np.isnan(mid[2]).all() and np.isnan(vw[2]).all()
    assert np.isnan(mid[0, 0]) and mid[0, 1] == 103.0 and np.isnan(mid[0, 2]) and vw[0, 1] == (3 * 100 + 2 * 101 + 4 * 102) / 9 and np.isnan(vw[0, 0])
    with pytest.raises(mx.MxaError, match="mxa_bars_from_records: level_cap > 1024"):
        mbars.from_records(d_rec, d_cnt, 1025, T0, DT, NB)
    with pytest.raises(mx.MxaError, match="mxa_bars_from_records: n_bars < 1"):
        mbars.from_records(d_rec, d_cnt, 192, T0, DT, 0)


# ---- handles

def handle_refs(m, t0, dt, n_bars, envs=None):
    out = []
    for e in (range(m.n_envs) if envs is None else envs):
        r = m.book_log_records(e, partial=True)
        out.append(bars_ref(r, 1024, t0, dt, n_bars))
    return out


def assert_bars(got, refs, what=""):
    bars, status = got
    for e, (want, wst) in enumerate(refs):
        assert status[e].tolist() == wst.tolist(), (what, e, status[e].tolist(), wst.tolist())
        bad = np.flatnonzero((bars[e] != want).any(axis=1))
        assert not len(bad), (what, e, int(bad[0]), bars[e, bad[0]].tolist(), want[bad[0]].tolist())


def test_gpu_bars_value_noise_with_and_without_the_exchange_log(mx):
    seeds = [7, 123456789]
    m = mx.VecMarket("value_noise", seeds, book_log=CAP)
    m.run()
    assert (m.summary()["status"] == 1).all()
    x = mx.VecMarket("value_noise", seeds, book_log=CAP, exchange_log=True)
    x.run()
    for dt, n in ((60 * S, 60), (S, 3600)):
        got = m.bars(OPEN_NS, dt, n)
        assert got[0].shape == (2, n, 12) and got[0].dtype == np.int64 and got[1].shape == (2, 4) and got[1].dtype == np.int32
        refs = handle_refs(m, OPEN_NS, dt, n)
        assert_bars(got, refs, dt)
        assert (got[1][:, 0] == 0).all() and got[0][:, :, 8].sum() > 0
        logged = x.bars(OPEN_NS, dt, n)
        assert np.array_equal(logged[0], got[0]) and np.array_equal(logged[1][:, [0, 2, 3]], got[1][:, [0, 2, 3]])
        assert (logged[1][:, 1] > got[1][:, 1]).all()  # the log's records are consumed too
    assert int(got[0][0, :, 8].sum()) == 4154 and got[1][0, 2:].tolist() == [25, 17]  # seed 7, as on the CPU oracle


def test_gpu_bars_rmsc03_mid_episode_end_and_reset(mx):
    """rmsc03 x2 in launches of 3,001 pops on a torch side stream: write_bars between two launches sees the
    records so far, at the end the whole episode; after reset() every row is 0"""
    seeds, n, dt = [123456789, 7], 900, S
    ref = mx.VecMarket("rmsc03", seeds, book_log=CAP)
    assert ref.run(chunk=3001, max_launches=1) == 1
    want_mid = handle_refs(ref, OPEN_NS, dt, n)
    n_mid = [len(ref.book_log_records(e)) for e in range(2)]
    ref.run(chunk=3001)
    want_end = handle_refs(ref, OPEN_NS, dt, n)
    n_end = [len(ref.book_log_records(e)) for e in range(2)]
    assert all(0 < a < b for a, b in zip(n_mid, n_end)), (n_mid, n_end)
    assert all(w[1][1] == a for w, a in zip(want_mid, n_mid)) and all(w[1][1] < b for w, b in zip(want_end, n_end))  # the end stops at 09:45

    stream = torch.cuda.Stream()
    m = mx.VecMarket("rmsc03", seeds, book_log=CAP)
    m.set_stream(stream.cuda_stream)
    bufs = [torch.full((2, n, 12), -3, dtype=torch.int64, device="cuda") for _ in range(2)]
    sts = [torch.full((2, 4), -3, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    m.launch(3001)
    m.write_bars(OPEN_NS, dt, n, bufs[0].data_ptr(), sts[0].data_ptr())
    m.launch(3001)
    m.sync()
    m.run(chunk=3001)
    assert (m.summary()["status"] == 1).all()
    m.write_bars(OPEN_NS, dt, n, bufs[1].data_ptr(), sts[1].data_ptr())
    m.sync()
    assert_bars((bufs[0].cpu().numpy(), sts[0].cpu().numpy()), want_mid, "mid")
    assert_bars((bufs[1].cpu().numpy(), sts[1].cpu().numpy()), want_end, "end")
    assert_bars(m.bars(OPEN_NS, dt, n), want_end, "read")
    assert not np.array_equal(bufs[0].cpu().numpy(), bufs[1].cpu().numpy())
    m.reset()
    bars, status = m.bars(OPEN_NS, dt, n)
    assert not bars.any() and not status.any()


def test_gpu_bars_full_log_is_status_1(mx):
    m = mx.VecMarket("rmsc03", [123456789, 7], book_log=1000)
    m.run()
    s = m.summary()
    assert (s["status"] == 2).all() and (s["err"] == 20).all()
    got = m.bars(OPEN_NS, S, 900)
    assert (got[1][:, 0] == 1).all() and (got[1][:, 1] == 1000).all()
    refs = []
    for e in range(2):
        r = m.book_log_records(e, partial=True)
        assert len(r) == 1000
        want, wst = bars_ref(r, 1024, OPEN_NS, S, 900, capacity=1000, count=1001)
        refs.append((want, wst))
    assert_bars(got, refs)


def test_gpu_bars_ibm_replay_runner(mx):
    from test_oracle_replay_runner import load_replay
    _, _, _, tp = load_replay("IBM", "2003-01-14")
    m = mx.VecMarket("marketreplay_runner", [0], tape=tp, symbol="IBM", book_log=CAP)
    m.run()
    assert m.summary()["status"][0] == 1
    got = m.bars(OPEN_NS, 60 * S, 390)
    assert got[1][0, 0] == 0 and got[1][0, 2:].tolist() == [106, 102]
    r = m.book_log_records(0)
    assert ((r["price"] < 0) & ((-r["price"].astype(np.int64)) & M != 0) & bl.book_mask(r)).any()  # modifyOrder records
    assert_bars(got, handle_refs(m, OPEN_NS, 60 * S, 390))
    assert got[0][0, :, 8].sum() > 0 and (got[0][0, -1, 1] > 0) and (got[0][0, -1, 3] > 0)


def test_gpu_bars_refusals_on_live_handles(mx):
    """every MXA_EINVAL case that needs a real handle, with its message; the buffers stay untouched"""
    from mxabides.gym import VecABIDESEnv
    from test_gpu_partial_reset import RL_SEEDS
    buf = torch.full((2, 4, 12), -3, dtype=torch.int64, device="cuda")
    st = torch.full((2, 4), -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plain = mx.VecMarket("rmsc03", [1, 2])
    with pytest.raises(mx.MxaError, match="mxa_write_bars.*mxa_set_book_log first"):
        plain.write_bars(OPEN_NS, S, 4, buf.data_ptr(), st.data_ptr())
    with pytest.raises(ValueError, match="book_log=0"):
        plain.bars(OPEN_NS, S, 4)
    host = np.full((2, 4, 12), -3, dtype=np.int64)
    assert plain.L.mxa_read_bars(plain._h, OPEN_NS, S, 4, host.ctypes.data, None) == -1
    assert b"mxa_read_bars: no book-update log" in plain.L.mxa_last_error(plain._h)
    v = VecABIDESEnv(seeds=RL_SEEDS[:2])
    for f, name in ((v.L.mxa_write_bars, b"mxa_write_bars"), (v.L.mxa_read_bars, b"mxa_read_bars")):
        assert f(v._h, OPEN_NS, S, 4, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())) == -1
        err = v.L.mxa_last_error(v._h)
        assert err.startswith(name) and b"GymKernel handle" in err, err
    m = mx.VecMarket("rmsc03", [1, 2], book_log=4096)
    m.run(chunk=3000, max_launches=1)
    I64 = 2**63 - 1
    for t0, dt, n, what in ((OPEN_NS, 0, 4, "dt_ns <= 0"), (OPEN_NS, -S, 4, "dt_ns <= 0"), (OPEN_NS, S, 0, "n_bars < 1"),
                            (OPEN_NS, S, (1 << 24) + 1, "n_bars > 1 << 24"), (-1, S, 4, "t0_ns < 0"),
                            (OPEN_NS, I64 // 4, 4, "beyond int64"), (I64, 1, 1, "beyond int64")):
        with pytest.raises(mx.MxaError, match="mxa_write_bars: .*" + what):
            m.write_bars(t0, dt, n, buf.data_ptr(), st.data_ptr())
        with pytest.raises(mx.MxaError, match="mxa_read_bars: .*" + what):
            m.bars(t0, dt, n)
    with pytest.raises(mx.MxaError, match="mxa_write_bars: null bars"):
        m.write_bars(OPEN_NS, S, 4, 0, st.data_ptr())
    with pytest.raises(mx.MxaError, match="mxa_write_bars: bars array not 16-byte aligned"):
        m.write_bars(OPEN_NS, S, 4, buf.data_ptr() + 8, st.data_ptr())
    m.sync()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == -3).all() and (st.cpu().numpy() == -3).all() and (host == -3).all()
    m.write_bars(OPEN_NS, S, 4, buf.data_ptr(), 0)  # a NULL status pointer is accepted
    m.sync()
    want = handle_refs(m, OPEN_NS, S, 4)
    assert all(np.array_equal(buf[e].cpu().numpy(), want[e][0]) for e in range(2)) and (st.cpu().numpy() == -3).all()
