"""The bars tests' own reference (include/mxa_bars.h), written from OrderBook.py's semantics and the
header's definitions, not from the kernel: a dict of level volumes per side, executeOrder's loop
(OrderBook.py:172-240) at price-level granularity, and the bar rules one by one.  Plain Python ints
throughout, so nothing wraps."""
import numpy as np

from mxabides import booklog as bl

WORDS, STATUS_WORDS = 12, 4
OK, LOG_OVERFLOW, LEVELS_EXCEEDED, STREAM_INCONSISTENT = 0, 1, 2, 3
LIMIT, CANCEL, MODIFY = "limit", "cancel", "modify"
OPEN_NS = bl.MKT_OPEN_NS


def recs(rows):
    """[(t, price, qty)] or an [n][3] array -> a REC_DTYPE array"""
    a = np.zeros(len(rows), dtype=bl.REC_DTYPE)
    if len(rows):
        r = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        a["t"], a["price"], a["qty"] = r[:, 0], r[:, 1], r[:, 2]
    return a


class Stop(Exception):
    def __init__(self, code):
        self.code = code


def _book_changing(records):
    """(index in the stream, t, price, qty) of the records that change the book"""
    records = np.asarray(records, dtype=bl.REC_DTYPE)
    keep = np.flatnonzero(bl.book_mask(records)) if len(records) else []
    for i in keep:
        r = records[i]
        yield int(i), int(r["t"]), int(r["price"]), int(r["qty"])


def _apply(sides, level_cap, p, q):
    """one book-changing record on sides = (bids, asks) dicts price -> volume; returns (kind, fills),
    fills the [(price, shares)] of a limit order; raises Stop(code)"""
    if p < 0 and (-p) & bl.BL_MODIFY:
        s, price = ((-p) >> 29) & 1, (-p) & ((1 << 29) - 1)
        if price not in sides[s] or sides[s][price] + q < 0:
            raise Stop(STREAM_INCONSISTENT)
        sides[s][price] += q  # modifyOrder: the level's head takes the new quantity, the level stays
        return MODIFY, []
    if p < 0:
        s, price = (0 if q > 0 else 1), -p
        if price not in sides[s] or sides[s][price] < abs(q):
            raise Stop(STREAM_INCONSISTENT)
        sides[s][price] -= abs(q)
        if sides[s][price] == 0:
            del sides[s][price]
        return CANCEL, []
    own = 0 if q > 0 else 1
    opp, left, fills = sides[1 - own], abs(q), []
    while left and opp:
        best = min(opp) if own == 0 else max(opp)
        if (best > p) if own == 0 else (best < p):
            break
        take = min(left, opp[best])
        left -= take
        if take:
            fills.append((best, take))
        if take == opp[best]:
            del opp[best]
        else:
            opp[best] -= take
    if left:
        if p not in sides[own] and len(sides[own]) >= level_cap:
            raise Stop(LEVELS_EXCEEDED)
        sides[own][p] = sides[own].get(p, 0) + left
    return LIMIT, fills


def _inside(sides):
    bids, asks = sides
    b, a = (max(bids) if bids else None), (min(asks) if asks else None)
    return (b or 0, bids[b] if bids else 0, a or 0, asks[a] if asks else 0)


def replay(records, level_cap=1 << 30):
    """per book-changing record: (t, kind, best bid, bid vol, best ask, ask vol, fills) after it"""
    sides = ({}, {})
    for _, t, p, q in _book_changing(records):
        kind, fills = _apply(sides, level_cap, p, q)
        yield (t, kind) + _inside(sides) + (fills,)


def bars_ref(records, level_cap, t0, dt, n_bars, capacity=None, count=None):
    """(bars [n_bars][12] int64, status [4] int32) of one env's stream.  capacity / count: the log's
    capacity and the count the device holds (count > capacity: the log overflowed and `records` are its
    first `capacity` ones)"""
    records = np.asarray(records, dtype=bl.REC_DTYPE)
    if capacity is not None:
        records = records[:capacity]
    bars = [[0] * WORDS for _ in range(n_bars)]
    end = t0 + n_bars * dt
    sides = ({}, {})
    peak = [0, 0]
    cur, acc = -1, None  # the open bar and its words 4-11
    code, consumed = OK, len(records)

    def close(upto):
        """the open bar and the empty ones after it, below `upto`, get the quotes as they stand"""
        q = list(_inside(sides))
        if cur >= 0:
            bars[cur] = q + acc
        for b in range(cur + 1, upto):
            bars[b] = q + [0] * 8

    for i, t, p, q in _book_changing(records):
        if t >= end:
            consumed = i
            break
        idx = -1 if t < t0 else (t - t0) // dt
        if idx > cur:  # the bar index never goes back
            close(idx)
            cur, acc = idx, [0] * 8
        try:
            kind, fills = _apply(sides, level_cap, p, q)
        except Stop as s:
            code, consumed = s.code, i
            break
        for s in (0, 1):
            peak[s] = max(peak[s], len(sides[s]))
        if cur < 0:
            continue
        for price, shares in fills:
            if acc[4] == 0:
                acc[0] = acc[1] = acc[2] = price
            acc[1], acc[2], acc[3] = max(acc[1], price), min(acc[2], price), price
            acc[4] += shares
            acc[5] += price * shares
        acc[6] += 1 if fills else 0
        acc[7] += 1
    if code == OK:
        close(n_bars)
        if count is not None and capacity is not None and count > capacity:
            code = LOG_OVERFLOW
    else:  # the bar the record falls in and every later one are zero rows
        for b in range(max(cur, 0), n_bars):
            bars[b] = [0] * WORDS
    return np.asarray(bars, dtype=np.int64).reshape(n_bars, WORDS), np.asarray([code, consumed] + peak, dtype=np.int32)


def oracle_records(o):
    """an oracle's book_records() as a REC_DTYPE array"""
    return recs(o.book_records())
