"""Runtime compositions at their price and parameter edges, on the CPU (composition_edges.py):
the refusals of mxa_config_compile and ora_create_config from one list, the unbounded oracle
against reference runs at megashocks every 0.1 s, at prices <= 0 and beyond INT32_MAX, and the
oracle's opt-in price range (ora_set_price_words on a composition: include/mxa.h MXA_PRICE_MAX) over
the seed pool test_gpu_composition_edges.py runs, with the conditions it relies on."""
import math

import numpy as np
import pytest

import bars_util
import composition_edges as E
import pyoracle
from golden_util import first_mismatch, load_composition

NAN, INF = float("nan"), float("inf")
# (base, fields, message): each refused by the device and the oracle with the same words
REFUSED = [
    ("rmsc03", dict(r_bar=NAN), "r_bar is not finite"),
    ("rmsc03", dict(kappa=INF), "kappa is not finite"),
    ("rmsc03", dict(fund_vol=NAN), "fund_vol is not finite"),
    ("rmsc03", dict(megashock_lambda_a=INF), "megashock_lambda_a is not finite"),
    ("rmsc03", dict(megashock_mean=-INF), "megashock_mean is not finite"),
    ("rmsc03", dict(megashock_var=INF), "megashock_var is not finite"),
    ("rmsc03", dict(value_sigma_n=INF), "value_sigma_n is not finite"),
    ("rmsc03", dict(value_r_bar=NAN), "value_r_bar is not finite"),
    ("rmsc03", dict(value_kappa=NAN), "value_kappa is not finite"),
    ("rmsc03", dict(value_sigma_s=INF), "value_sigma_s is not finite"),
    ("rmsc03", dict(value_lambda_a=INF), "value_lambda_a is not finite"),
    ("rmsc03", dict(zi_sigma_pv=NAN), "zi_sigma_pv is not finite"),  # (a field its base never reads)
    ("rmsc03", dict(lat_high=INF), "lat_high is not finite"),
    ("rmsc03", dict(mm={"mm_pov": NAN}), "mm.mm_pov is not finite"),
    ("sparse_zi_100", dict(zi_sigma_n=INF), "zi_sigma_n is not finite"),
    ("sparse_zi_100", dict(zi_lambda_a=NAN), "zi_lambda_a is not finite"),
    ("rmsc03", dict(kappa=0.0), "kappa must be > 0"),
    ("rmsc03", dict(kappa=-1.67e-12), "kappa must be > 0"),
    ("value_noise", dict(kappa=0.0), "kappa must be > 0"),
    ("sparse_zi_100", dict(kappa=0.0), "kappa must be > 0"),
    ("rmsc03", dict(value_kappa=0.0), r"value_kappa must lie in \(0, 1\]"),
    ("rmsc03", dict(value_kappa=-1e-15), r"value_kappa must lie in \(0, 1\]"),
    ("rmsc03", dict(value_kappa=math.nextafter(1.0, 2.0)), r"value_kappa must lie in \(0, 1\]"),
    ("value_noise", dict(value_kappa=2.0), r"value_kappa must lie in \(0, 1\]"),
    ("sparse_zi_100", dict(zi_kappa=0.0), r"zi_kappa must lie in \(0, 1\]"),
    ("sparse_zi_1000", dict(zi_kappa=1.5), r"zi_kappa must lie in \(0, 1\]"),
    ("rmsc03", dict(value_sigma_n=0.0), "value_sigma_n must be > 0"),
    ("rmsc03", dict(value_sigma_n=-1.0), "value_sigma_n must be > 0"),
    ("sparse_zi_100", dict(zi_sigma_n=0.0), "zi_sigma_n must be > 0"),
    ("rmsc03", dict(value_sigma_s=-1e-4), "value_sigma_s must be >= 0"),
    ("sparse_zi_100", dict(zi_sigma_s=-1e-4), "zi_sigma_s must be >= 0"),
    ("rmsc03", dict(r_bar=-1.0), r"r_bar must lie in \[0, 2\^31\)"),
    ("rmsc03", dict(r_bar=2.0 ** 31), r"r_bar must lie in \[0, 2\^31\)"),
    ("rmsc03", dict(value_r_bar=2.0 ** 31), r"value_r_bar must lie in \[0, 2\^31\)"),
    ("rmsc03", dict(value_r_bar=-0.5), r"value_r_bar must lie in \[0, 2\^31\)"),
    ("sparse_zi_100", dict(zi_r_bar=2.0 ** 31), r"zi_r_bar must lie in \[0, 2\^31\)"),
]
# just inside each bound: accepted by both
ACCEPTED = [
    ("rmsc03", dict(kappa=5e-324)),
    ("rmsc03", dict(value_kappa=5e-324)),
    ("rmsc03", dict(value_kappa=1.0)),
    ("sparse_zi_100", dict(zi_kappa=1.0)),
    ("sparse_zi_100", dict(zi_kappa=5e-324)),
    ("rmsc03", dict(value_sigma_n=5e-324)),
    ("rmsc03", dict(value_sigma_s=0.0)),
    ("sparse_zi_100", dict(zi_sigma_s=0.0)),
    ("rmsc03", dict(r_bar=0.0, value_r_bar=0.0)),
    ("rmsc03", dict(r_bar=math.nextafter(2.0 ** 31, 0.0), value_r_bar=math.nextafter(2.0 ** 31, 0.0))),
    # the fields of the other bases' agents are not read, whatever they hold
    ("rmsc03", dict(zi_kappa=0.0, zi_sigma_n=0.0, zi_r_bar=-1.0)),
    ("sparse_zi_100", dict(value_kappa=0.0, value_sigma_n=0.0, value_r_bar=-1.0)),
]


@pytest.fixture(scope="module")
def C():
    from mxabides import composition
    return composition


def _make(C, base, fields):
    f = dict(fields)
    return C.make(base, mm=f.pop("mm", None), **f)


@pytest.mark.parametrize("base,fields,msg", REFUSED, ids=["%s-%s" % (b, "-".join(f)) + str(i) for i, (b, f, _) in enumerate(REFUSED)])
def test_refused_by_device_and_oracle_before_any_compile(C, base, fields, msg):
    from mxabides import _lib
    c = _make(C, base, fields)
    with pytest.raises(_lib.MxaError, match=msg):
        C.compile(c, cache_dir="/nonexistent/never/written")
    with pytest.raises(ValueError, match=msg):
        pyoracle.OracleEnv(c, 1)


@pytest.mark.parametrize("base,fields", ACCEPTED, ids=["%s-%s" % (b, "-".join(f)) + str(i) for i, (b, f) in enumerate(ACCEPTED)])
def test_just_inside_each_bound_is_accepted_by_both(C, base, fields):
    """the device's check passes (mxa_config_capacities runs it and compiles nothing) and the
    oracle builds the env"""
    c = _make(C, base, fields)
    assert len(C.capacities(c)) == 2
    pyoracle.OracleEnv(c, 1)


@pytest.mark.parametrize("name,seed", E.EDGE_FIXTURES)
def test_unbounded_oracle_equals_reference_at_the_edge(C, name, seed):
    """trace, events, hash, book, order counter, last trade and report lines of the reference's own
    run; without ora_set_price_words the oracle's prices are int64, as the reference's are ints"""
    d, ref, summ = load_composition(name, seed)
    cfg = C.from_dict(d["composition"])
    assert bytes(cfg) == bytes(pyoracle.as_config(cfg))
    e = pyoracle.OracleEnv(cfg, seed, trace_cap=len(ref))
    e.run()
    assert e.error[0] == 0, e.error
    assert first_mismatch(e.trace(), ref) == -1
    assert e.events == d["events"]
    assert "%016x" % e.hash == d["hash"]
    assert e.book(0) == d["bids"] and e.book(1) == d["asks"]
    assert e.order_counter - 1 == d["order_id_counter"]
    assert e.last_trade == d["last_trade"]
    e.finish()
    rep = e.report()
    assert [l for l in rep if l.startswith("Final holdings")] == d["final_holdings_lines"]
    assert [l for l in rep if not l.startswith("Final holdings")] == d["mean_lines"]
    # what each fixture is there for
    p = ref[ref[:, 3] == E.K_LIMIT][:, 8]
    if name == "rmsc03_low":
        assert (p <= 0).sum() >= 10 and p.min() < 0, "the reference places orders at prices <= 0 and runs on"
    if name == "rmsc03_high":
        assert (p > 2 ** 31 - 1).sum() >= 10
    if name in E.FINISH + E.STOP_FIRST:
        r_bar = int(d["composition"]["r_bar"])
        assert len(p) > 100 and (p == r_bar).all(), "every order at py_round(r_T) = r_bar exactly"
        assert r_bar == {"rmsc03_top": E.PRICE_MAX, "rmsc03_over": E.PRICE_MAX + 1, "rmsc03_bottom": 1, "rmsc03_zero": 0}[name]


def test_shocks_pool_conditions(C):
    """the 256 seeds of test_gpu_composition_batch_equals_oracle under rmsc03_shocks, from the
    oracle's f_log records: error 0 everywhere, at least 2,000 fundamental values per env, prices
    inside the range, and an observation interval with two or more megashocks.  A fundamental value
    is computed once per megashock, at its own time, and once per observation, at the time of the
    pop that observes (SparseMeanRevertingOracle.py:155-179): an f_log time that is no pop's time is
    a megashock, and two of them in a row lie inside one observation interval (first 8 seeds, with
    the trace; every env's count of 2,000 against some 300 observations says the same)"""
    cfg = E.composition("rmsc03_shocks")
    seeds = ((np.arange(256, dtype=np.int64) * 7919 + 3) & 0xFFFFFFFF).astype(np.uint32)
    ev, hs, er, _ = pyoracle.run_batch_config(cfg, seeds, threads=8)
    assert (er == 0).all()
    for i, s in enumerate(seeds):
        r = E.Run(cfg, s, False, price_words=False)
        assert r.err == 0 and r.events == ev[i] and r.hash == hs[i]
        f = r.f_log
        assert len(f) >= 2000, (s, len(f))
        assert f[:, 2].min() > 0 and f[:, 2].max() < E.PRICE_MAX
        if i < 8:
            o = pyoracle.OracleEnv(cfg, int(s), trace_cap=int(ev[i]))
            o.run()
            shock = ~np.isin(f[:, 0], o.trace()[:, 0])
            assert shock.sum() >= 1500 and (shock[1:] & shock[:-1]).any(), (s, shock.sum())
        w = E.Run(cfg, s, False)  # the price range changes nothing here
        assert (w.err, w.events, w.hash) == (0, r.events, r.hash)


@pytest.mark.parametrize("name", E.EDGES)
def test_price_range_stops_over_the_pool(C, name):
    """32 seeds under ora_set_price_words: which envs stop and on whose order, never an ambiguous
    record"""
    cfg = E.composition(name)
    rs = E.runs(name)
    err = E.column(rs, "err")
    cls = [r.msg.split(" ")[0] if r.err else "" for r in rs]
    print(name, "stopped %d of %d" % ((err != 0).sum(), len(rs)), {c: cls.count(c) for c in set(cls)},
          "events", E.column(rs, "events").tolist())
    assert np.isin(err, (0, pyoracle.ERR_ORDER_PRICE)).all()
    assert all(c in ("ValueAgent", "POVMarketMakerAgent", "NoiseAgent", "MomentumAgent") for c in cls if c)
    for r, s in zip(rs, E.SEEDS):
        u = E.Run(cfg, s, False, price_words=False)
        # which env stops, at which event and on whose order: from the unbounded run's trace, the
        # earliest pop that pushes an order outside the range (an aggressive order that matches in
        # full leaves no record, but it is in the trace)
        want = E.expected_stop(cfg, s)
        if r.err == 0:  # inside the range the switch changes nothing
            assert want is None, (name, s, want)
            assert (r.events, r.hash, r.last_trade) == (u.events, u.hash, u.last_trade)
        else:
            assert want is not None and (r.events, r.msg.split(" ")[0]) == want, (name, s, r.events, r.msg, want)
            assert r.events < u.events and "outside the device's 1 .. 2^30 - 1" in r.msg
            price = int(r.msg.split(" outside")[0].split(" ")[-1])
            assert price < 1 or price > E.PRICE_MAX, r.msg
        # the records written up to the stop: a prefix of the unbounded run's, every limit price
        # inside the range, and a stream bars_ref finds consistent
        assert len(r.records) <= len(u.records) and (r.records == u.records[:len(r.records)]).all()
        book = r.records[r.records[:, 1] > E.BL_FUNDAMENTAL + 1024]
        assert (np.abs(book[:, 1]) >= 1).all() and (np.abs(book[:, 1]) <= E.PRICE_MAX).all()
        _, st = bars_util.bars_ref(bars_util.recs(r.records), 1 << 30, cfg.mkt_open_ns, 10 ** 10, 30)
        assert st[0] == bars_util.OK, (name, s, st)
    if name in E.FINISH:
        assert (err == 0).all()
        for r in rs:
            p = r.records[r.records[:, 1] > 0][:, 1]
            assert len(p) > 100 and (p == (E.PRICE_MAX if name == "rmsc03_top" else 1)).all()
    if name in E.STOP_FIRST:
        assert (err != 0).all() and all(c == "ValueAgent" for c in cls)
        for r, s in zip(rs, E.SEEDS):
            k, first = E.first_value_order(cfg, s)
            assert r.events == k, (s, r.events, k)
            assert str(int(first[8])) in r.msg
    if name == "rmsc03_high":
        assert (err != 0).all() and all(c == "ValueAgent" for c in cls)
    if name == "rmsc03_top_mm":
        assert cls.count("POVMarketMakerAgent") >= 8 and cls.count("") >= 4
        for r in rs:  # value orders pass up to the range's top, the ladder never does
            p = r.records[r.records[:, 1] > 0][:, 1]
            assert len(p) and p.max() <= E.PRICE_MAX and p.min() >= E.PRICE_MAX - 40
    if name == "rmsc03_low":
        assert cls.count("ValueAgent") >= 4 and cls.count("POVMarketMakerAgent") >= 1 and cls.count("") >= 4
        zero_first = [r for r in rs if r.err and (r.f_log[:, 2] == 0).any()]
        assert len(zero_first) >= 3, "an f_log value of 0 precedes the stop"


def test_stops_by_both_classes_across_the_set():
    cls = {r.msg.split(" ")[0] for n in E.EDGES for r in E.runs(n) if r.err}
    assert {"ValueAgent", "POVMarketMakerAgent"} <= cls


def test_f_log_value_beyond_int32_stops_with_the_book_log_only(C):
    """a fundamental past INT32_MAX (r_bar just under 2^31, megashocks of +-1e6 every 0.1 s, no
    agent that places an order): the env stops at that value when the book log is on, and runs on
    without it, as the device's f_log record is written by the book-log kernels only"""
    c = C.make("rmsc03", n_noise=1, n_value=1, n_mm=0, n_momentum=0, r_bar=2147483000.0, value_r_bar=1e5,
               megashock_lambda_a=1e-8, megashock_mean=1e6, megashock_var=0.0, mkt_close_ns=(9 * 3600 + 31 * 60) * 10 ** 9,
               kernel_stop_ns=(9 * 3600 + 32 * 60) * 10 ** 9, value_lambda_a=1e-9)
    o = pyoracle.OracleEnv(c, 10)  # (the seed whose fundamental passes INT32_MAX before any order is placed)
    o.set_book_log()
    o.set_price_words()
    o.run()
    assert o.error[0] == pyoracle.ERR_ORDER_PRICE and "fundamental value" in o.error[1]
    f = o.book_records()
    f = f[f[:, 1] == E.BL_FUNDAMENTAL]
    assert len(f) and (f[:, 2] <= 2 ** 31 - 1).all() and (f[:, 2] >= 0).all()
    o = pyoracle.OracleEnv(c, 10)
    o.set_book_log()
    o.run()
    f = o.book_records()
    assert o.error[0] == 0 and (f[f[:, 1] == E.BL_FUNDAMENTAL][:, 2] > 2 ** 31 - 1).any()
