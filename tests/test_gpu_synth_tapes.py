"""The replay book on the device against crafted tapes (tests/synth_tapes.py): the HBM price
ladder, its per-level FIFO lists, the entry pool, the per-id live-entry chains and epoch register,
lvl_next's 64-level strides and the head-replace modify (mxa_kernels.hip rp_*, mr_*), at the edges
the real LOBSTER days never reach.  Every comparison is exact, against the reference's fixture of
the same tape (tests/golden/synth_*) and the C oracle, which tests/test_synth_tapes.py holds to
those fixtures and to each tape's coverage facts on the CPU."""
import numpy as np
import pytest
import torch  # (before libmxa initialises HIP, as the other GPU test modules that share a process)

import pyoracle
import synth_tapes as S
from golden_util import load_named
from mxabides import booklog as bl
from mxabides.gym import OBS_SIZE, VecABIDESEnv
from test_synth_tapes import (CUT_SCHEDULE, INT32_MAX, K_LIMIT, K_SPREAD, OBS_RTOL, RUNNER, TRACE_CAP,
                              check_episode_end, check_step, gym_actions, load_gym, oracle_run, refused_pop)

pytestmark = pytest.mark.gpu

REFUSED = ["modify_price", "modify_side"]
ERR_RP_MODIFY = 16
LOG_CAP = 1 << 14


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def runner_tape(name):
    return S.groups(ns=True)[0] if name == "groups_ns" else S.RUNNER_TAPES[name]()[0]


def agent_tuples(m, env):
    return [(a["cash"], a["shares"], a["n_open"]) for a in m.agents(env)]


def assert_env_equals_oracle(m, env, o, s=None):
    s = m.summary() if s is None else s
    assert s["status"][env] == 1, "env error %d" % s["err"][env]
    assert int(s["events"][env]) == o.events and int(s["hash"][env]) == o.hash
    assert (m.trace(env) == o.trace()).all()
    assert m.book(env, 0) == o.book(0) and m.book(env, 1) == o.book(1)
    assert agent_tuples(m, env) == [tuple(a) for a in o.agents()]


@pytest.mark.parametrize("name", [n for n in RUNNER if n not in REFUSED] + ["groups_ns"])
def test_gpu_runner_tape_matches_reference_and_oracle(mx, name):
    """config/marketreplay.py on the tape: trace, events, hash, both books (every resting order,
    FIFO), agent state, report and summary log against the reference fixture and the oracle; three
    envs run whole, then pop by pop (chunk=1: every pop a save / restore boundary, mid-group
    included) and in launches of 7; reset and rerun gives the same hash"""
    tp = runner_tape(name)
    o = oracle_run(tp)
    n_envs = 2 if name == "ladder_ends" else 3  # ladder_ends: P = 2^20, the widest ladder
    m = mx.VecMarket("marketreplay_runner", np.zeros(n_envs, dtype=np.int64), tape=tp, symbol=tp.symbol,
                     trace_cap=TRACE_CAP)
    if name == "ladder_ends":
        print("ladder_ends mxa_env_bytes", m.env_bytes)
    m.run()
    for env in range(n_envs):
        assert_env_equals_oracle(m, env, o)
    if name != "groups_ns":  # (no reference run of nanosecond times: the reference parses float seconds)
        d, trace, summ = load_named("synth_" + name)
        s = m.summary()
        assert (m.trace(0) == trace).all() and int(s["events"][0]) == d["events"]
        assert "%016x" % int(s["hash"][0]) == d["hash"]
        assert m.book(0, 0) == d["bids"] and m.book(0, 1) == d["asks"]
        (ag,) = d["agents"]
        assert agent_tuples(m, 0)[ag["id"]] == (ag["cash"], ag["shares"], len(ag["open_orders"]))
        holdings, means = m.report(0)
        assert holdings == d["final_holdings_lines"] and means == d["mean_lines"]
        got = m.summary_log(0)
        assert got == summ and all(type(x["Event"]) is type(y["Event"]) for x, y in zip(got, summ))
    for chunk in (1, 7):
        m.reset()
        m.run(chunk=chunk)
        for env in range(n_envs):
            assert_env_equals_oracle(m, env, o)
    m.reset()
    m.run()
    assert (m.summary()["hash"] == o.hash).all()


@pytest.mark.parametrize("name", REFUSED)
def test_gpu_refused_modify_stops_the_env_at_that_pop(mx, name):
    """a price- or side-changing modify is env error 16 where the reference goes on.  The refused
    pop i comes from the oracle's trace (test_synth_tapes.refused_pop), not from the device: the
    device has counted and traced pops 0 .. i (a pop is accounted before its handler runs, as the
    reference's trace holds the pop in which it raises), and its books and agents are the
    oracle's after i pops, OracleEnv.run(i): the refused modify changed nothing"""
    tp = runner_tape(name)
    full = oracle_run(tp).trace()
    i = refused_pop(name, full)
    before = oracle_run(tp, max_pops=i)
    m = mx.VecMarket("marketreplay_runner", np.zeros(3, dtype=np.int64), tape=tp, symbol=tp.symbol, trace_cap=TRACE_CAP)
    for chunk in (1 << 20, 1, 7):
        m.run(chunk=chunk)
        s = m.summary()
        assert (s["status"] == 2).all() and (s["err"] == ERR_RP_MODIFY).all(), (s["status"], s["err"])
        assert (s["events"] == i + 1).all(), (s["events"], i)
        for env in range(3):
            assert len(m.trace(env)) == i + 1 and (m.trace(env) == full[:i + 1]).all()
            assert m.book(env, 0) == before.book(0) and m.book(env, 1) == before.book(1)
            assert agent_tuples(m, env) == [tuple(a) for a in before.agents()]
        m.reset()


@pytest.mark.parametrize("name", ["fifo_chain", "fills", "ladder_gaps", "one_level", "epochs"])
def test_gpu_book_and_exchange_logs_equal_oracle(mx, name):
    """the book-update records with the exchange's own log riding in them, record for record; the
    OrderBook.book_log rows and the BEST_BID / BEST_ASK / LAST_TRADE events rebuilt from them.
    The head-replace modifies are BL_MODIFY records (six of fifo_chain's eight find an entry)"""
    tp = runner_tape(name)
    o = oracle_run(tp, logs=True)
    a = o.book_records()
    m = mx.VecMarket("marketreplay_runner", [0, 0], tape=tp, symbol=tp.symbol, book_log=LOG_CAP, exchange_log=True)
    m.run(chunk=5)
    s = m.summary()
    assert (s["status"] == 1).all() and (s["hash"] == o.hash).all()
    mod = a[(a[:, 1] < 0) & (a[:, 1] > -(1 << 31) + 4096) & ((-a[:, 1]) & (1 << 30) != 0)]
    assert name != "fifo_chain" or len(mod) == 6  # the modifies that found an entry (matches > 0)
    for env in range(2):
        d = m.book_log_records(env)
        assert len(d) == len(a)
        assert np.array_equal(d["t"], a[:, 0]) and np.array_equal(d["price"], a[:, 1]) and np.array_equal(d["qty"], a[:, 2])
        assert np.array_equal(m.book_log_rows(env), o.book_log())
    ev = m.exchange_events(1)
    ref = bl.exchange_events_frame(o.book_log(), tp.symbol, tp.date)
    assert len(ev) == len(ref) and ev["Event"].tolist() == ref["Event"].tolist() and (ev.index == ref.index).all()


@pytest.mark.parametrize("name", ["ladder_gaps", "fills"])
def test_gpu_twap_handle_passive_equals_oracle(mx, name):
    """execution_marketreplay.py without -e on the tape: the third agent learns the market hours
    and sleeps (a passive TWAP agent sends no QUERY_SPREAD; rp_spread is read by the gym tapes'
    steps), the replay runs through mxa_create_replay_twap's own build of the book"""
    tp = runner_tape(name)
    o = oracle_run(tp, twap=False)
    m = mx.VecMarket("marketreplay_twap", [0, 0], tape=tp, symbol=tp.symbol, trace_cap=TRACE_CAP)
    m.run(chunk=11)
    for env in range(2):
        assert_env_equals_oracle(m, env, o)


# ---- the gym handle (mxa_create_replay + mxa_step): DummyRL reads a QUERY_SPREAD (rp_spread, depth
# 500) in every step and places at the level-1 and level-2 bid prices it was quoted
ERR_RP_IDS, ERR_RP_QUOTE_SIZE = 12, 30
N_GYM = 4


def step_batch(v, oras, acts_i, alive, stop=None):
    """one step of the batch on the device and on each live env's oracle; stop[e](oracle, records
    the step added) -> True where the device must refuse the step.  Returns the envs refused"""
    before = [o.events for o in oras]
    obs, done, valid, err = v.step(acts_i)
    ev = v.summary()["events"]
    refused = []
    for e in np.nonzero(alive)[0]:
        n0 = len(oras[e].trace())
        o_obs, o_done, rc = oras[e].step(acts_i[e])
        assert rc == 0, oras[e].error
        if stop is not None and stop(e, oras[e].trace()[n0:]):
            assert err[e], e
            refused.append((int(e), before[e], oras[e].trace()[n0:]))
            alive[e] = False
            continue
        assert not err[e], (e, v.summary()["err"][e], oras[e].order_counter, oras[e].trace()[n0:][:, 3:9].tolist()[:12])
        assert ev[e] == oras[e].events and bool(done[e]) == o_done, e
        if o_obs is not None:
            assert valid[e]
            np.testing.assert_allclose(obs[e], o_obs, rtol=OBS_RTOL, atol=1e-12, err_msg="env %d" % e)
        alive[e] = not o_done
    return refused


def assert_gym_env_equals_oracle(v, e, o, s):
    assert s["status"][e] == 1 and s["events"][e] == o.events and s["hash"][e] == o.hash, (e, s["err"][e])
    assert s["order_counter"][e] == o.order_counter
    assert v.book(e, 0) == o.book(0) and v.book(e, 1) == o.book(1), e
    assert v.agents(e) == [tuple(x) for x in o.agents()], e


def test_gpu_gym_ladder_gaps_matches_reference_and_oracle():
    """4 envs with different action streams on ladder_gaps_gym: level-2 prices read across the
    64-level strides decide where DummyRL's second order goes, so every step's records show them"""
    tp, _ = S.ladder_gaps_gym()
    (ep,) = load_gym("ladder_gaps_gym")
    acts = gym_actions(N_GYM, ep["actions"])
    v = VecABIDESEnv(tp, N_GYM, trace_cap=1 << 15)
    oras = [pyoracle.OracleGymEnv(tp, trace_cap=1 << 15) for _ in range(N_GYM)]
    alive = np.ones(N_GYM, dtype=bool)
    for i in range(len(acts)):
        step_batch(v, oras, acts[i], alive)
        check_step(ep, i, v.summary()["events"][0], v.flags[0] & 1, v.obs[0])
    s = v.summary()
    check_episode_end(ep, s["events"][0], int(s["hash"][0]), v.trace(0), v.book(0, 0), v.book(0, 1),
                      s["order_counter"][0], v.agents(0), tp.symbol)
    for e in range(N_GYM):
        assert_gym_env_equals_oracle(v, e, oras[e], s)
        assert (v.trace(e) == oras[e].trace()).all()


def test_gpu_gym_step_many_equals_one_step_launches_on_ladder_gaps():
    tp, _ = S.ladder_gaps_gym()
    k = 200
    acts = gym_actions(N_GYM, load_gym("ladder_gaps_gym")[0]["actions"])[:k]
    act = torch.tensor(acts, dtype=torch.float64, device="cuda")
    obs_a = torch.zeros((k, N_GYM, OBS_SIZE), dtype=torch.float64, device="cuda")
    flg_a = torch.zeros((k, N_GYM), dtype=torch.int32, device="cuda")
    obs_b, flg_b = torch.zeros_like(obs_a), torch.zeros_like(flg_a)
    a, b = VecABIDESEnv(tp, N_GYM), VecABIDESEnv(tp, N_GYM)
    for v in (a, b):
        v.set_parity_hash(True)
        v.reset()
    torch.cuda.synchronize()
    for i in range(k):
        a.step_device(act[i].data_ptr(), obs_a[i].data_ptr(), flg_a[i].data_ptr())
    b.step_many_device(k, act.data_ptr(), obs_b.data_ptr(), flg_b.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(flg_a, flg_b) and torch.equal(obs_a.view(torch.int64), obs_b.view(torch.int64))
    sa, sb = a.summary(), b.summary()
    for key in ("events", "hash", "status", "err", "current_time"):
        assert (sa[key] == sb[key]).all(), key


def test_gpu_gym_fills_big_level_quote_is_an_env_error():
    """fills_gym rests 3 x (2^31 - 2) shares at the best bid: the reference (and the oracle) quote
    6,442,450,938; the device's QUERY_SPREAD reply and its trace record carry a level's quantity
    in a signed 32-bit word (before this test rp_spread sent the total's low 32 bits, 2,147,483,642,
    silently).  Now the env stops with error 30 in the exchange's pop of the QUERY_SPREAD request,
    in the step where the oracle first quotes more than 2^31 - 1; every step before it equals the
    oracle, and the device's trace ends with that request"""
    tp, _ = S.fills_gym()
    acts = gym_actions(N_GYM, load_gym("fills_gym")[0]["actions"])
    v = VecABIDESEnv(tp, N_GYM, trace_cap=1 << 14)
    oras = [pyoracle.OracleGymEnv(tp, trace_cap=1 << 14) for _ in range(N_GYM)]
    alive = np.ones(N_GYM, dtype=bool)

    def big(e, recs):
        q = recs[recs[:, 3] == K_SPREAD]
        return bool(((q[:, 5] > INT32_MAX) | (q[:, 7] > INT32_MAX)).any())

    refused, steps = [], 0
    while alive.any():
        refused += step_batch(v, oras, acts[steps], alive, stop=big)
        steps += 1
    assert steps > 5 and sorted(e for e, _, _ in refused) == list(range(N_GYM))
    s = v.summary()
    assert (s["status"] == 2).all() and (s["err"] == ERR_RP_QUOTE_SIZE).all(), (s["status"], s["err"])
    for e, ev0, recs in refused:
        (k,) = np.nonzero((recs[:, 3] == K_SPREAD) & (recs[:, 5] > INT32_MAX))[0][:1]
        assert recs[k - 1, 3] == 5 and s["events"][e] == ev0 + k  # pops up to and with the request
        full = oras[e].trace()
        assert (v.trace(e) == full[:ev0 + k]).all()


def run_skip_episodes(name, stop=None):
    """three episodes of one process: env 0 on the reference's own actions and held to its fixture
    while it runs, three other action streams beside it"""
    tp, _ = S.GYM_TAPES[name]()
    eps = load_gym(name)
    cap = 1 << 16  # an env that trades more than the reference's actions pops more events than the fixture
    v = VecABIDESEnv(tp, N_GYM, trace_cap=cap)
    oras = [pyoracle.OracleGymEnv(tp, trace_cap=cap) for _ in range(N_GYM)]
    out = []
    for k, ep in enumerate(eps):
        acts = gym_actions(N_GYM, ep["actions"], seed=7 + k)
        if k:
            v.reset()
            for o in oras:
                o.reset(trace_cap=cap)
        base = [o.order_counter for o in oras]
        alive = np.ones(N_GYM, dtype=bool)
        refused = []
        for i in range(len(acts)):
            refused += step_batch(v, oras, acts[i], alive, stop=(lambda e, r: stop(k, base[e], r)) if stop else None)
            if not any(e == 0 for e, _, _ in refused):
                check_step(ep, i, v.summary()["events"][0], v.flags[0] & 1, v.obs[0])
        s = v.summary()
        gone = {e for e, _, _ in refused}
        for e in range(N_GYM):
            if e in gone:
                continue
            assert_gym_env_equals_oracle(v, e, oras[e], s)
            assert (v.trace(e) == oras[e].trace()).all()
        if 0 not in gone:
            check_episode_end(ep, s["events"][0], int(s["hash"][0]), v.trace(0), v.book(0, 0), v.book(0, 1),
                              s["order_counter"][0], v.agents(0), tp.symbol)
        out.append((s, refused, base))
    return v, out, eps


def test_gpu_gym_skip_fit_three_episodes_id_for_id():
    """id persistence on: in the third episode the auto ids step over 3,600 used explicit ids (runs
    of 1, 2 and up to 703) and take the free ones between them, the last order carrying
    id_base + 5119, the highest the dense range admits (test_synth_tapes.test_facts_gym_skip_bound).
    Every episode equals the reference fixture (env 0) and the oracle; with persistence off the
    first episode equals a fresh process"""
    v, out, eps = run_skip_episodes("gym_skip_fit")
    tp, _ = S.gym_skip_fit()
    s3, refused, base = out[2]
    assert not refused and base == [3040] * N_GYM
    assert (s3["order_counter"] == 3040 + S.SKIP_BOUND).all()
    v.set_id_persistence(False)
    v.reset()
    fresh = [pyoracle.OracleGymEnv(tp, trace_cap=1 << 16) for _ in range(N_GYM)]
    acts = gym_actions(N_GYM, eps[0]["actions"], seed=7)
    alive = np.ones(N_GYM, dtype=bool)
    for i in range(len(acts)):
        step_batch(v, fresh, acts[i], alive)
    s = v.summary()
    assert (s["hash"] == out[0][0]["hash"]).all() and (s["order_counter"] == 1520).all()


def test_gpu_gym_skip_over_ends_in_err_rp_ids():
    """one used id more: the third episode's last id is id_base + 5120.  An env whose order of
    non-zero size carries an id >= id_base + SKIP_BOUND (read from the oracle's records of that
    step: DummyRL's LIMIT_ORDERs) ends in ERR_RP_IDS in that step, with the events of the step
    before (the order is refused when it is placed); every step before equals the oracle, and the
    env that places nothing (zero sizes still draw ids, but no order carries them) finishes equal"""
    def over(k, base, recs):
        rl = recs[(recs[:, 3] == K_LIMIT) & (recs[:, 5] == 2)]
        return bool((rl[:, 4] - base >= S.SKIP_BOUND).any())

    v, out, _ = run_skip_episodes("gym_skip_over", stop=over)
    assert not out[0][1] and not out[1][1]
    s3, refused, base = out[2]
    gone = sorted(e for e, _, _ in refused)
    assert 1 in gone and N_GYM - 1 not in gone  # the steady 500 + 500 env reaches the bound; the idle env never
    for e, ev0, _ in refused:
        assert s3["status"][e] == 2 and s3["err"][e] == ERR_RP_IDS and s3["events"][e] == ev0
    assert s3["status"][N_GYM - 1] == 1 and s3["order_counter"][N_GYM - 1] == 3040 + S.SKIP_BOUND + 1


def test_gpu_gym_skip_ids_used_later_in_the_episode_are_not_skipped_yet():
    """rp_skip_used's max(tape_hi, mr_done): six episodes cut short by a reset leave tape_hi at the
    tape's first 1,595 records; in the seventh the auto ids pass the explicit ids, step over the
    used ones, carry ids the tape places later in that episode, and from record 1,595 on the
    skips follow mr_done (test_synth_tapes.test_facts_gym_skip_cut_short_episodes has the facts).
    No reference run (its fixtures run whole episodes): 4 envs against the oracle, every step a
    launch, every episode's trace, books, agents and counter"""
    tp, _ = S.gym_skip_fit()
    cap = 1 << 16
    v = VecABIDESEnv(tp, N_GYM, trace_cap=cap)
    oras = [pyoracle.OracleGymEnv(tp, trace_cap=cap) for _ in range(N_GYM)]
    acts = gym_actions(N_GYM, load_gym("gym_skip_fit")[0]["actions"])
    for k, steps in enumerate(CUT_SCHEDULE):
        if k:
            v.reset()
            for o in oras:
                o.reset(trace_cap=cap)
        alive = np.ones(N_GYM, dtype=bool)
        for i in range(steps):
            step_batch(v, oras, acts[i], alive)
        s = v.summary()
        for e in range(N_GYM):
            assert s["status"][e] == 0 and s["events"][e] == oras[e].events and s["hash"][e] == oras[e].hash, (k, e)
            assert s["order_counter"][e] == oras[e].order_counter, (k, e)
            assert (v.trace(e) == oras[e].trace()).all(), (k, e)
            assert v.book(e, 0) == oras[e].book(0) and v.book(e, 1) == oras[e].book(1), (k, e)
            assert v.agents(e) == [tuple(x) for x in oras[e].agents()], (k, e)
    assert (s["order_counter"] > 4097 + 2500).all()
