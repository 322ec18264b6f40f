"""The crafted replay tapes (tests/synth_tapes.py) on the CPU: (a) every builder still gives the
committed tape, (b) the C oracle reproduces the reference's run of each tape
(tests/golden/synth_*, gen_synth_tape_fixtures.py), (c) each tape still reaches the edge it was
built for: its coverage facts hold on the oracle's trace, books and stats(), and its pending
events stay far below the replay queue's capacity.  tests/test_gpu_synth_tapes.py then holds the
device to the same fixtures and oracle runs."""
import hashlib
import json
import os

import numpy as np
import pytest

import pyoracle
import synth_tapes as S
from golden_util import GOLDEN, load_named
from mxabides import tape

K_WAKEUP, K_LIMIT, K_CANCEL, K_MODIFY, K_ACCEPTED, K_EXECUTED, K_CANCELLED, K_MODIFIED = 0, 11, 12, 13, 14, 15, 16, 18
RUNNER = list(S.RUNNER_TAPES)
TRACE_CAP = 1 << 14  # every runner tape pops fewer events


def committed_tape(tp):
    return tape.Tape.load(os.path.join(GOLDEN, "tape_%s_%s.npz" % (tp.symbol, tp.date)))


def oracle_run(tp, max_pops=-1, twap=None, logs=False):
    e = pyoracle.OracleReplayRunner(tp, symbol=tp.symbol, trace_cap=TRACE_CAP, twap=twap)
    if logs:
        e.set_book_log(True)
        e.set_exchange_log(True)
    e.run(max_pops)
    return e


_WALKS = {}


def walk(name):
    """the oracle's run pop by pop: [(trace record, bids, asks, last_trade)] with a side as
    [(price, total quantity, orders)] best first; computed once per tape"""
    if name not in _WALKS:
        tp, _ = S.RUNNER_TAPES[name]()
        e = pyoracle.OracleReplayRunner(tp, symbol=tp.symbol, trace_cap=TRACE_CAP)
        out = []
        while e.run(1):
            sides = [[(lv[0][3], sum(o[2] for o in lv), len(lv)) for lv in e.book(s)] for s in (0, 1)]
            out.append((e.trace()[-1].copy(), sides[0], sides[1], e.last_trade))
        _WALKS[name] = (out, e)
    return _WALKS[name]


def best_removals(name):
    """(side, "cancel" | "fill", distance to the side's next level, that level's price or None)
    for every pop that removed a side's best level"""
    out, prev = [], ([], [])
    for rec, bids, asks, _ in walk(name)[0]:
        for s, (was, now) in enumerate(zip(prev, (bids, asks))):
            if was and was[0][0] not in [lv[0] for lv in now]:
                kind = {K_CANCEL: "cancel", K_LIMIT: "fill"}[int(rec[3])]
                worse = [lv[0] for lv in now if (lv[0] < was[0][0] if s == 0 else lv[0] > was[0][0])]
                out.append((s, kind, abs(worse[0] - was[0][0]) if worse else None, worse[0] if worse else None))
        prev = (bids, asks)
    return out


def modified_per_modify(trace):
    """ORDER_MODIFIED records delivered after each MODIFY_ORDER (the tapes' groups lie 1 s apart)"""
    counts = []
    for k in trace[:, 3]:
        if k == K_MODIFY:
            counts.append(0)
        elif k == K_MODIFIED:
            counts[-1] += 1
    return counts


def refused_pop(name, trace):
    """0-based index of the pop at which the device refuses the tape's modify, from the oracle's
    trace: the MODIFY_ORDER's delivery at the exchange (a price change: rp_modify), or the replay
    agent's wakeup that builds it (a side change: mr_place_record_as)"""
    _, facts = S.RUNNER_TAPES[name]()
    kind, oid, price = facts["refused"]
    (i,) = np.nonzero((trace[:, 3] == kind) & (trace[:, 4] == oid) & (trace[:, 8] == price))[0][-1:]
    if "refused_wakeup_t" in facts:
        (i,) = np.nonzero((trace[:, 3] == K_WAKEUP) & (trace[:, 1] == 1) & (trace[:, 0] == facts["refused_wakeup_t"]))[0]
    return int(i)


@pytest.mark.parametrize("name", RUNNER + list(S.GYM_TAPES))
def test_builder_equals_committed_tape(name):
    tp, _ = getattr(S, name)()
    c = committed_tape(tp)
    for k in ("t", "oid", "price", "size", "buy"):
        assert (getattr(tp, k) == getattr(c, k)).all() and getattr(tp, k).dtype == getattr(c, k).dtype, k
    assert (c.symbol, c.date) == (tp.symbol, tp.date)
    assert tp.oid[tp.oid > 0].min() == S.first_id(tp.n_auto)  # the smallest id create_replay accepts


@pytest.mark.parametrize("name", RUNNER)
def test_oracle_matches_reference(name):
    """as test_oracle_replay_runner.py; for modify_price and modify_side the oracle follows the
    reference past the modify the device refuses (the head is re-keyed and the run goes on)"""
    tp, _ = S.RUNNER_TAPES[name]()
    d, trace, summ = load_named("synth_" + name)
    e = oracle_run(tp)
    assert e.error[0] == 0, e.error
    assert len(trace) == d["events"] and (e.trace() == trace).all()
    assert e.events == d["events"] and "%016x" % e.hash == d["hash"]
    assert e.book(0) == d["bids"] and e.book(1) == d["asks"]
    assert e.last_trade == d["last_trade"]
    assert max(e.order_counter - 1, 0) == d["order_id_counter"]
    (ag,) = d["agents"]
    assert e.agents()[ag["id"]] == (ag["cash"], ag["shares"], len(ag["open_orders"]))
    e.finish()
    rep = e.report()
    assert [l for l in rep if l.startswith("Final holdings")] == d["final_holdings_lines"]
    assert [l for l in rep if not l.startswith("Final holdings")] == d["mean_lines"]
    got = e.summary_log()
    assert got == summ and all(type(a["Event"]) is type(b["Event"]) for a, b in zip(got, summ))


def test_groups_ns_is_the_same_run_at_other_times():
    """the 1 ns variant has no reference fixture (the reference parses float seconds): the oracle's
    records equal the millisecond tape's up to the last sweep, but for the times"""
    a, b = oracle_run(S.groups()[0]), oracle_run(S.groups(ns=True)[0])
    n = len(b.trace()) - 20
    assert b.error[0] == 0 and n > 1700 and (a.trace()[:n, 1:] == b.trace()[:n, 1:]).all()
    assert b.stats()[0] <= S.QUEUE_CAP // 2, b.stats()
    assert (np.diff(np.unique(S.groups(ns=True)[0].t)) == 1).all()


@pytest.mark.parametrize("name", RUNNER)
def test_queue_cap_and_ladder(name):
    """the cap is a condition, not a measurement: pending events stay at or below half the replay
    queue's 256 slots on every tape (queue overflow is pinned elsewhere)"""
    tp, facts = S.RUNNER_TAPES[name]()
    e = oracle_run(tp)
    assert e.stats()[0] <= S.QUEUE_CAP // 2, e.stats()
    if "P" in facts:
        assert (int(tp.price.min()), int(tp.price.max())) == (facts["pmin"], facts["pmax"])
        assert facts["pmax"] - facts["pmin"] + 1 == facts["P"]


@pytest.mark.parametrize("name", ["ladder_gaps", "ladder_ends"])
def test_facts_best_level_removals(name):
    tp, facts = S.RUNNER_TAPES[name]()
    got = best_removals(name)
    assert set(facts["removals"]) <= {g[:3] for g in got}, sorted(set(facts["removals"]) - {g[:3] for g in got})
    # the next level at the ladder's two ends: index 0 (bids) and P - 1 (asks)
    assert any(s == 0 and nxt == facts["pmin"] for s, _, _, nxt in got)
    assert any(s == 1 and nxt == facts["pmax"] for s, _, _, nxt in got)
    if name == "ladder_gaps":
        for s in (0, 1):  # both kinds of removal over every gap, and the side emptied and refilled
            assert {(k, g) for s2, k, g, _ in got if s2 == s} >= {(k, g) for k in ("cancel", "fill") for g in S.GAPS}
            assert (s, "cancel" if s == 0 else "fill", None, None) in got
        out = walk(name)[0]
        assert out[-1][1] and out[-1][2]


def test_facts_one_level():
    out, e = walk("one_level")
    assert {lv[0] for _, b, a, _ in out for lv in b + a} == {12_345}
    assert any(b and not a for _, b, a, _ in out) and any(a and not b for _, b, a, _ in out)
    kinds = set(e.trace()[:, 3].tolist())
    assert {K_LIMIT, K_CANCEL, K_MODIFY, K_EXECUTED, K_CANCELLED, K_MODIFIED} <= kinds


def test_facts_fifo_chain():
    tp, facts = S.fifo_chain()
    out, e = walk("fifo_chain")
    assert modified_per_modify(e.trace()) == facts["modified"]
    assert e.book(0) == facts["final_bids"]
    assert max(lv[2] for _, b, _, _ in out for lv in b) >= 5  # a level of five entries
    # head, middle, tail and only-entry cancels: ORDER_CANCELLED for 7 of the 9 SIZE 0 records
    assert int((e.trace()[:, 3] == K_CANCELLED).sum()) == 7 and int((tp.size == 0).sum()) == 9
    # two entries of one id at the level when its cancel arrives: the head (the earlier arrival)
    # goes, so the level keeps its count minus one and loses the head's quantity, not the tail's
    h = facts["final_bids"][0][0][0]
    hits = [(out[i - 1][1], out[i][1]) for i in range(1, len(out)) if out[i][0][3] == K_CANCEL and out[i][0][4] == h]
    assert [(was[0][1] - now[0][1], was[0][2] - now[0][2]) for was, now in hits] == [(44, 1), (60, 1)]


def test_facts_epochs():
    tp, facts = S.epochs()
    _, e = walk("epochs")
    tr = e.trace()
    assert modified_per_modify(tr) == facts["modified"]
    r = S.first_id() + 1
    assert int(((tr[:, 3] == K_LIMIT) & (tr[:, 4] == r)).sum()) == facts["id_epochs"] > S.ID_EPOCHS
    assert 1 < facts["modified"][1] < S.STREAM_HISTORY + 1  # some of the id's epochs in the window, some not


def test_facts_fills():
    tp, facts = S.fills()
    out, e = walk("fills")
    tr = e.trace()
    p = facts["big_price"]
    assert any(lv[0] == p and lv[1] == facts["big_total"] for _, b, _, _ in out for lv in b)
    assert facts["big_total"] > 1 << 32
    ex = tr[tr[:, 3] == K_EXECUTED]
    assert (ex[:, 7] * ex[:, 9]).max() > 1 << 50
    trades = [lt for (_, _, _, lt), (_, _, _, prev) in zip(out[1:], out[:-1]) if lt != prev]
    it = iter(trades)
    assert all(x in it for x in facts["last_trades"]), trades  # in this order
    # a partial fill of the head, an exact fill, a sweep of three levels with a rest, a side emptied
    lim = [i for i, (rec, _, _, _) in enumerate(out) if rec[3] == K_LIMIT]
    swept = [(len(out[i - 1][2]) - len(out[i][2]), len(out[i][1]) - len(out[i - 1][1])) for i in lim]
    assert (3, 1) in swept
    assert any(out[i - 1][1] and not out[i][1] for i in lim)
    assert any(len(out[i][2]) == len(out[i - 1][2]) and out[i][2] and out[i - 1][2] and out[i][2][0][0] == out[i - 1][2][0][0]
               and out[i][2][0][2] == out[i - 1][2][0][2] and out[i][2][0][1] < out[i - 1][2][0][1] for i in lim)


def test_facts_groups():
    tp, facts = S.groups()
    _, counts = np.unique(tp.t, return_counts=True)
    assert counts.tolist() == facts["group_sizes"] and {1, 2, 63, 64, 65, 100} <= set(counts.tolist())
    assert tp.t[0] == facts["first_t"] == S.OPEN_NS and tp.t[-1] == facts["last_t"] == S.CLOSE_NS - S.NS_MS
    _, e = walk("groups")
    tr = e.trace()
    assert tr[tr[:, 3] == K_LIMIT][-1, 0] == S.CLOSE_NS - 2 * S.NS_MS  # the last submitted group


def test_facts_auto_ids():
    tp, facts = S.auto_ids()
    _, e = walk("auto_ids")
    tr = e.trace()
    assert tp.n_auto == facts["n_zero"] and e.order_counter == facts["order_counter"]
    mods = tr[tr[:, 3] == K_MODIFY]
    assert sorted(mods[:, 4].tolist()) == [1, S.first_id(tp.n_auto)]  # auto id 1: the modify that is not the same order
    assert modified_per_modify(tr) == [1, 0]
    assert set(tr[(tr[:, 3] == K_LIMIT) & (tr[:, 4] < 4096), 4].tolist()) == {0, 2, 3, 4, 5, 6}
    assert tr[tr[:, 3] == K_CANCEL][:, 4].tolist() == [0]


@pytest.mark.parametrize("name", ["modify_price", "modify_side"])
def test_facts_refused_modify(name):
    tp, facts = S.RUNNER_TAPES[name]()
    e = oracle_run(tp)
    tr = e.trace()
    i = refused_pop(name, tr)
    assert 0 < i < len(tr) - 4  # records follow the refused modify
    kind, oid, price = facts["refused"]
    m = tr[(tr[:, 3] == K_MODIFY) & (tr[:, 4] == oid)][-1]
    before = oracle_run(tp, max_pops=i)
    level = [lv for lv in before.book(0) if lv[0][3] == 9_500]
    assert level and len(level[0]) == 2  # the old level holds orders when the modify arrives
    if name == "modify_price":
        assert tr[i, 3] == K_MODIFY and m[8] == price == 9_501
        # the reference re-keys the head in place: an order priced 9501 heads the 9500 level
        assert [o[3] for o in oracle_run(tp, max_pops=i + 1).book(0)[0]] == [9_501, 9_500]
    else:
        assert tr[i, 3] == K_WAKEUP and m[6] == 0  # the new order sells; the order it replaces buys


# ---- gym tapes (ABIDESEnv: the replay plus DummyRL, whose every step reads a QUERY_SPREAD at depth 500)
GYM = list(S.GYM_TAPES)  # the ones with a reference fixture (gym_skip_over is gym_skip_fit plus one record)
OBS_RTOL = 1e-9
K_SPREAD = 6
INT32_MAX = (1 << 31) - 1


def book_digest(levels):
    """gen_synth_tape_fixtures.book_digest: a side of the book as (orders, sha256 of its levels)"""
    return [sum(len(lv) for lv in levels), hashlib.sha256(json.dumps(levels, separators=(",", ":")).encode()).hexdigest()]


def load_gym(name):
    """the fixture's episodes: the JSON record of each (events, hash, counters, book digests, agents)
    with its arrays: actions, trace (head), obs [steps][9] (NaN rows: none), done, step_events"""
    with open(os.path.join(GOLDEN, "synth_%s.json" % name)) as f:
        d = json.load(f)
    z = np.load(os.path.join(GOLDEN, "synth_%s.npz" % name), allow_pickle=False)
    for k, ep in enumerate(d["episodes"], start=1):
        ep.update(actions=z["actions_%d" % k], trace=z["trace_%d" % k], obs=z["obs_%d" % k], done=z["done_%d" % k],
                  step_events=z["events_%d" % k])
    return d["episodes"]


def gym_actions(n_envs, fixture_actions, seed=7):
    """[steps][n_envs][3]: env 0 the reference's own actions, env 1 a steady 1,000 shares split in
    halves (both orders of every step non-empty), env 2 random, the last env nothing at all"""
    n = len(fixture_actions)
    acts = np.zeros((n, n_envs, 3))
    acts[:, 0] = fixture_actions
    acts[:, 1] = [0.01, 0.5, 0.5]
    rs = np.random.RandomState(seed)
    for e in range(2, n_envs - 1):
        acts[:, e, 0] = rs.uniform(0, 0.03, n)
        acts[:, e, 1:] = rs.uniform(0, 1, (n, 2))
    return acts


def check_step(ep, i, events, done, obs):
    """step i of a run on the reference's actions against the fixture"""
    assert events == ep["step_events"][i] and int(done) == ep["done"][i], i
    if not np.isnan(ep["obs"][i]).any():
        np.testing.assert_allclose(obs, ep["obs"][i], rtol=OBS_RTOL, atol=1e-12, err_msg="step %d" % i)


def check_episode_end(ep, events, hash_, trace, bids, asks, order_counter, agents, ticker):
    """an episode's end state against the fixture: the hash covers every pop of the episode"""
    assert events == ep["events"] and "%016x" % hash_ == ep["hash"]
    assert (trace[:len(ep["trace"])] == ep["trace"]).all()
    assert book_digest(bids) == ep["bids"] and book_digest(asks) == ep["asks"]
    assert order_counter == ep["order_id_counter"] + 1
    for ref in ep["agents"]:
        assert tuple(agents[ref["id"]]) == (ref["holdings"]["CASH"], ref["holdings"].get(ticker, 0), ref["n_open"])


@pytest.mark.parametrize("name", GYM)
def test_oracle_gym_episodes_match_reference(name):
    """one episode, or (gym_skip_fit) three of one reference process: ids continue, used explicit
    ids are stepped over"""
    tp, _ = S.GYM_TAPES[name]()
    e = None
    for k, ep in enumerate(load_gym(name)):
        if e is None:
            e = pyoracle.OracleGymEnv(tp, trace_cap=len(ep["trace"]))
        else:
            e.reset(trace_cap=len(ep["trace"]))
        assert e.order_counter == (ep["order_id_counter_start"] + 1 if k else 0)
        for i, a in enumerate(ep["actions"]):
            obs, done, rc = e.step(a)
            assert rc == 0, e.error
            check_step(ep, i, e.events, done, obs)
        check_episode_end(ep, e.events, e.hash, e.trace(), e.book(0), e.book(1), e.order_counter, e.agents(), tp.symbol)
        assert e.stats()[0] <= S.QUEUE_CAP // 2
    assert len(load_gym(name)) == S.GYM_EPISODES.get(name, 1)


def spread_quotes(name, acts=(0.0, 0.5, 0.5)):
    """the QUERY_SPREAD replies of one oracle episode: trace records of kind 6"""
    tp, _ = getattr(S, name)()
    e = pyoracle.OracleGymEnv(tp, trace_cap=1 << 16)
    while True:
        _, done, rc = e.step(acts)
        if rc or done:
            break
    tr = e.trace()
    return tr[tr[:, 3] == K_SPREAD], tr


def test_facts_ladder_gaps_gym():
    """the quoted best bid / ask cross every gap between two consecutive replies' books, and DummyRL's
    second order goes to the level-2 bid price rp_spread read across the gap (lvl_next)"""
    sp, tr = spread_quotes("ladder_gaps_gym", (0.01, 0.5, 0.5))
    assert len(sp) >= 760 and (sp[:, 9] % (1 << 20) // 2).min() >= 1 and (sp[:, 9] >> 20).min() >= 1  # two-sided throughout
    bids = np.unique(sp[:, 4])
    assert len(bids) >= 6  # the best bid is quoted at most of the nine levels
    rl = tr[(tr[:, 3] == K_LIMIT) & (tr[:, 5] == 2)]
    gaps = {int(a - b) for a, b in zip(rl[:-1, 8], rl[1:, 8]) if a > b}
    assert set(S.GAPS) <= gaps, sorted(gaps)  # level-1 / level-2 prices every gap apart, the stride edges included


def first_big_quote(sp):
    big = np.nonzero((sp[:, 5] > INT32_MAX) | (sp[:, 7] > INT32_MAX))[0]
    return int(big[0]) if len(big) else None


def test_facts_fills_gym_quotes_the_big_level():
    """a level total above 2^32 is quoted (the reference's Python int); the device's reply carries a
    signed 32-bit quantity, so it stops the env there (ERR_RP_QUOTE_SIZE, test_gpu_synth_tapes.py)"""
    sp, _ = spread_quotes("fills_gym")
    _, facts = S.fills_gym()
    assert sp[:, 5].max() == facts["big_total"] > 1 << 32
    k = first_big_quote(sp)
    assert k is not None and k >= 5 and sp[k, 4] == facts["big_price"]  # ordinary steps come first


def skip_episode_ids(name):
    """(first auto id, last auto id) of each of the three oracle episodes, steady actions"""
    tp, _ = getattr(S, name)()
    e = pyoracle.OracleGymEnv(tp)
    out = []
    for k in range(3):
        if k:
            e.reset()
        c0 = e.order_counter
        while True:
            _, done, rc = e.step((0.01, 0.5, 0.5))
            assert rc == 0
            if done:
                break
        out.append((c0, e.order_counter - 1))
    return out


def test_facts_gym_skip_bound():
    """Derivation of the dense-id bound (not found on the device).  create_replay sizes the dense
    range D = n_ids + (rl_ids + n_zero) + MXA_AUTO_SKIP + 1 and agent_dense maps auto id `id` to
    d = n_ids + (id - id_base), refusing d >= D - 1: an order may carry id - id_base <
    rl_ids + n_zero + MXA_AUTO_SKIP = 4096 + 0 + 1024 = 5120 (synth_tapes.SKIP_BOUND), id_base the
    episode's first auto id.  Episodes 1 and 2 draw 1,520 ids each and meet no explicit id
    (the smallest is 4097); episode 3 starts at 3040, draws 1,520 and steps over every used explicit
    id: 6 + 7 + the stream.  With SKIP_STREAM_FIT stream orders its last id is 3040 + 5119; with one
    more it is 3040 + 5120 and the order that carries it must end the env in ERR_RP_IDS.  The id
    of the never-submitted last group lies inside the run and is taken, not skipped."""
    assert S.SKIP_BOUND == S.RL_IDS + S.AUTO_SKIP == 5120
    fit, over = skip_episode_ids("gym_skip_fit"), skip_episode_ids("gym_skip_over")
    assert fit[:2] == over[:2] == [(0, 1519), (1520, 3039)]
    assert fit[2] == (3040, 3040 + S.SKIP_BOUND - 1) and over[2] == (3040, 3040 + S.SKIP_BOUND)
    tp, facts = S.gym_skip_fit()
    used = set(tp.oid[:-1].tolist())
    assert facts["hole"] not in used and facts["hole"] - 1 in used and facts["hole"] + 1 in used
    assert {4097, 4099, 4100, 4102} <= used and not {4098, 4101} & used  # runs of 1 and 2, then the long run
    # the hole is taken by an auto id in episode 3 (a LIMIT_ORDER of DummyRL carries it)
    e = pyoracle.OracleGymEnv(tp)
    for k in range(3):
        if k:
            e.reset(trace_cap=1 << 16)
        while not e.step((0.01, 0.5, 0.5))[1]:
            pass
    tr = e.trace()
    rl_ids = tr[(tr[:, 3] == K_LIMIT) & (tr[:, 5] == 2), 4]
    assert facts["hole"] in rl_ids and 4098 in rl_ids and 4101 in rl_ids and not set(rl_ids.tolist()) & used
    assert rl_ids.max() == 3040 + S.SKIP_BOUND - 1


CUT_SCHEDULE = [S.CUT_STEPS] * (S.CUT_EPISODES - 1) + [S.CUT_LAST_STEPS]


def test_facts_gym_skip_cut_short_episodes():
    """ids used only later in the same episode are not skipped yet.  Six episodes of gym_skip_fit are
    cut short by a reset after 300 steps: the process has used the tape's first 1,595 records
    (tape_hi) and its counter stands at 3588.  The seventh runs 500 steps: its auto ids pass 4097,
    step over the ids those records used, and then carry explicit ids that the tape places later in
    this same episode; once the replay passes record 1,595 the skips are decided by this episode's
    own progress (mr_done), not by tape_hi"""
    tp, _ = S.gym_skip_fit()
    first = {}
    for i, (oid, size) in enumerate(zip(tp.oid.tolist(), tp.size.tolist())):
        if size > 0:
            first.setdefault(oid, i)
    e = pyoracle.OracleGymEnv(tp, trace_cap=1 << 16)
    reach = []
    for k, steps in enumerate(CUT_SCHEDULE):
        if k:
            e.reset(trace_cap=1 << 16)
        for _ in range(steps):
            assert e.step((0.01, 0.5, 0.5))[2] == 0, e.error
        tr = e.trace()
        reach.append(max(first[x] for x in tr[(tr[:, 3] == K_LIMIT) & (tr[:, 5] == 1), 4].tolist()) + 1)
        assert e.stats()[0] <= S.QUEUE_CAP // 2
    hi, done = max(reach[:-1]), reach[-1]
    assert hi == 1595 and done == 2595 and e.order_counter > 4097 + 2500
    rl = tr[(tr[:, 3] == K_LIMIT) & (tr[:, 5] == 2), 4].tolist()
    assert rl[0] < 4097  # the last episode starts below the explicit ids
    later = [x for x in rl if hi <= first.get(x, -1) < done]
    assert len(later) > 100, len(later)  # auto ids equal to explicit ids the tape places later in this episode
    skipped = [x for a, b in zip(rl[:-1], rl[1:]) for x in range(a + 1, b)]
    assert all(first.get(x, done) < done for x in skipped)  # only used ids are stepped over
    assert sum(first[x] < hi for x in skipped) > 1000 and sum(first[x] >= hi for x in skipped) > 100
