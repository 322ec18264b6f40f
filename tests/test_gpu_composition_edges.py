"""Runtime compositions at their price and parameter edges on the device (composition_edges.py,
include/mxa.h MXA_PRICE_MAX): 32 envs per composition, one launch sequence per test, each env
against the oracle under the same price range (ora_set_price_words), the envs that stop with
ERR_ORDER_PRICE (31) included, at the same event.  The engines are prebuilt by
__graft_entry__.build() from tests/golden/cfg_*.json; nothing compiles here.  What the pool holds
(who stops, on whose order) is asserted on the CPU by test_composition_edges.py."""
import numpy as np
import pytest

import bars_util
import composition_edges as E

pytestmark = pytest.mark.gpu

KEYS = ("status", "err", "events", "hash", "current_time", "order_counter", "last_trade")
ALL = E.EDGES + ("rmsc03_shocks",)


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def _expected(rs):
    x = {k: E.column(rs, k) for k in KEYS if k != "err"}
    x["err"] = np.array([E.ERR_DEVICE[r.err] for r in rs])
    return x


def _assert_summary(name, s, rs, what=""):
    x = _expected(rs)
    for k in KEYS:
        bad = np.nonzero(s[k] != x[k])[0]
        assert len(bad) == 0, "%s %s: %s of envs %s: device %s, oracle %s" % (name, what, k, bad.tolist()[:8], s[k][bad][:4],
                                                                             x[k][bad][:4])


@pytest.mark.parametrize("name", ALL)
def test_gpu_edge_equals_oracle(mx, name):
    """status, err, events, hash, current_time, order_counter and last_trade of every env, in one
    launch sequence and through 997-pop launches (which save and reload the env between them)"""
    rs = E.runs(name)
    cfg = E.composition(name)
    one = mx.VecMarket(cfg, E.SEEDS)
    one.run()
    s = one.summary()
    one.close()
    print(name, "status 1 x%d, 2 x%d; err %s" % ((s["status"] == 1).sum(), (s["status"] == 2).sum(), sorted(set(s["err"].tolist()))))
    _assert_summary(name, s, rs)
    many = mx.VecMarket(cfg, E.SEEDS)
    many.run(chunk=997)
    _assert_summary(name, many.summary(), rs, "in 997-pop launches")
    many.close()


@pytest.mark.parametrize("exchange_log", [False, True], ids=["book", "exlog"])
@pytest.mark.parametrize("name", ALL)
def test_gpu_edge_records_equal_oracle(mx, name, exchange_log):
    """the book-update log, record for record up to each env's end (the f_log records of the
    megashocks among them), the same summary with the log on, and bars over a stream that never
    holds an ambiguous record: status 0 for every env (the log is sized so that none fills)"""
    rs = E.runs(name, exchange_log)
    cfg = E.composition(name)
    assert max(len(r.records) for r in rs) <= E.BOOK_LOG
    m = mx.VecMarket(cfg, E.SEEDS, book_log=E.BOOK_LOG, exchange_log=exchange_log)
    m.run()
    _assert_summary(name, m.summary(), rs, "with the book log")
    for i, r in enumerate(rs):
        d = m.book_log_records(i)
        a = r.records
        assert len(d) == len(a), (name, i, len(d), len(a))
        for j, k in enumerate(("t", "price", "qty")):
            bad = np.nonzero(d[k] != a[:, j])[0]
            assert len(bad) == 0, (name, "env", i, k, "record", int(bad[0]), d[bad[0]], a[bad[0]])
        if name == "rmsc03_shocks":
            f = d[d["price"] == E.BL_FUNDAMENTAL]
            assert len(f) >= 2000 and (f["t"] == r.f_log[:, 0]).all() and (f["qty"] == r.f_log[:, 2]).all()
    t0, dt, nb = cfg.mkt_open_ns, 10 ** 10, 36  # ten-second bars from the open to the kernel's stop
    bars, status = m.bars(t0, dt, nb)
    m.close()
    assert (status[:, 0] == 0).all(), (name, np.nonzero(status[:, 0])[0], status[status[:, 0] != 0][:4])
    from mxabides import composition as C
    level_cap = (C.capacities(cfg)[1] + 63) // 64 * 64
    for i in (0, 1, 16, 31):  # the bars themselves against the tests' own replay of the oracle's records
        want, st = bars_util.bars_ref(bars_util.recs(rs[i].records), level_cap, t0, dt, nb)
        assert (status[i] == st).all() and (bars[i] == want).all(), (name, i, status[i], st)


def _shocks64():
    seeds = tuple(range(101, 165))
    return np.array(seeds, dtype=np.uint32), E.runs("rmsc03_shocks", False, seeds)


def test_gpu_shocks_masked_reset_mid_episode(mx):
    """64 envs stopped after 3,000 pops, every other one rebuilt from its seed, all run on: the
    rebuilt env starts its megashock series over (o_mst, o_msv, o_pt, o_pv are per-env state the
    reset must rebuild), its neighbours continue theirs"""
    seeds, rs = _shocks64()
    m = mx.VecMarket(E.composition("rmsc03_shocks"), seeds)
    m.launch(3000)
    m.sync()
    mid = m.summary()
    assert (mid["events"] == np.minimum(3000, E.column(rs, "events"))).all()
    mask = (np.arange(64) % 2).astype(np.uint8)
    m.reset(mask)
    after = m.summary()
    assert (after["events"][mask == 1] == 0).all() and (after["events"][mask == 0] == mid["events"][mask == 0]).all()
    m.run()
    _assert_summary("rmsc03_shocks", m.summary(), rs, "after a masked reset")
    m.close()


def test_gpu_shocks_snapshot_fork_at_a_launch_boundary(mx):
    """64 envs saved after 3,000 pops and run to the end; then envs 32-63 restored from the slots
    of envs 0-31 (a fork: block, seed word and with them the megashock state) and envs 0-31 from
    their own, and all run on: env i ends as the oracle's env i % 32"""
    seeds, rs = _shocks64()
    m = mx.VecMarket(E.composition("rmsc03_shocks"), seeds)
    m.launch(3000)
    m.sync()
    snap = m.snapshot()
    snap.save()
    m.run()
    _assert_summary("rmsc03_shocks", m.summary(), rs, "after the save")
    snap.restore({i: i % 32 for i in range(64)})
    back = m.summary()
    assert (back["events"] == np.minimum(3000, E.column(rs, "events"))[np.arange(64) % 32]).all()
    m.run()
    _assert_summary("rmsc03_shocks", m.summary(), [rs[i % 32] for i in range(64)], "after the fork")
    snap.close()
    m.close()
