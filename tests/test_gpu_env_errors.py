"""The env stop codes on the device (env_error_cases.py): every case's envs against the C oracle's
run of the same input, the stopping ones included: status 2, the code, the events, hash, time,
order counter and last trade at the stop, the trace record for record up to the stopping pop, and
the books and agents of that pop (the state before the failing action).  Stopping envs sit between
clean ones, whole, in 7-pop and in 1000-pop launches.  Then, once per handle kind, that a stop is
sticky.  Every comparison is exact.  The engines of the compositions are prebuilt by
__graft_entry__.build() from tests/golden/cfg_*.json; test_env_errors.py holds the oracle's runs to
the reference's fixtures on the CPU."""
import time

import numpy as np
import pytest
import torch  # (before libmxa initialises HIP, as the other GPU test modules that share a process)

import env_error_cases as E
from golden_util import first_mismatch
from mxabides import shard
from mxabides.gym import VecABIDESEnv

pytestmark = pytest.mark.gpu

KEYS = ("status", "events", "hash", "current_time", "order_counter", "last_trade")
# oracle fail() code -> device code, by handle kind (the oracle numbers a stop by its cause)
COMPOSITION_ERR = {0: 0, -5: 5, -3: 6, -6: 7}
TAPE_ERR = {0: 0, -3: 6, -17: 25, -18: 26}
EINVAL = -1


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def _agents(m, env):
    return [(a["cash"], a["shares"], a["n_open"]) if isinstance(a, dict) else tuple(a) for a in m.agents(env)]


def assert_env(m, env, r, to_dev, s=None, what="", exchange=False):
    """env of handle m is the oracle's Stop r: the summary, the trace through first_mismatch (the
    same pops, ending with the stopping one), both books and the agents"""
    s = m.summary() if s is None else s
    assert int(s["err"][env]) == to_dev[r.err], (what, env, int(s["err"][env]), r.err, r.msg)
    for k in KEYS:
        assert int(s[k][env]) == getattr(r, k), (what, env, k, int(s[k][env]), getattr(r, k))
    if m.trace_cap:
        t = m.trace(env)
        assert first_mismatch(t, r.trace) == -1, (what, env, first_mismatch(t, r.trace), len(t), len(r.trace))
    assert m.book(env, 0) == r.bids and m.book(env, 1) == r.asks, (what, env)
    a = _agents(m, env)
    assert (a if exchange else a[1:]) == (r.agents if exchange else r.agents[1:]), (what, env)


def run_bounded(m, chunk, max_events):
    """run() in launches of `chunk` pops, bounded by the launches the oracle's longest env needs: an
    env that fails to stop ends here as status 0, a failed assertion and not a hang"""
    bound = max_events // chunk + 2
    n = m.run(chunk=chunk, max_launches=bound)
    s = m.summary()
    assert (s["status"] != 0).all(), ("envs still running after %d launches of %d pops" % (n, chunk), np.nonzero(s["status"] == 0)[0])
    return s


@pytest.mark.parametrize("case", list(E.COMPOSITION_CASES))
def test_gpu_composition_case_equals_oracle(mx, case):
    """the case's batch in one launch sequence, then in 7-pop and in 1000-pop launches (each a save
    and reload of every env; a stopped env leaves the list of running envs and stays stopped)"""
    c = E.COMPOSITION_CASES[case]
    rs = E.composition_runs(c["fixture"], c["seeds"])
    longest = max(r.events for r in rs)
    t0 = time.time()
    m = mx.VecMarket(E.composition(c["fixture"]), c["seeds"], trace_cap=E.TRACE_CAP)
    for chunk in (1 << 20, 7, 1000):
        s = run_bounded(m, chunk, longest)
        for env, r in enumerate(rs):
            assert_env(m, env, r, COMPOSITION_ERR, s, "%s chunk %d" % (case, chunk))
        m.reset()
    m.close()
    print("%s: code %d, events at the stops %s, %d clean envs, %.2f s" % (
        case, c["code"], sorted({r.events for r in rs if r.err}), sum(r.err == 0 for r in rs), time.time() - t0))


@pytest.mark.parametrize("case", list(E.COMPOSITION_CASES))
def test_gpu_composition_case_equals_reference(mx, case):
    """the fixture seeds against the reference's own run: the trace up to the raise, events, hash,
    final time, books and agents; the clean neighbours (other compositions) run to status 1"""
    c = E.COMPOSITION_CASES[case]
    todo = [(c["fixture"], list(c["stops"]) + list(c["clean"]))] + [(f, [s]) for f, s in c["neighbours"]]
    for name, seeds in todo:
        m = mx.VecMarket(E.composition(name), seeds, trace_cap=E.TRACE_CAP)
        m.run()
        s = m.summary()
        for env, seed in enumerate(seeds):
            d, trace = E.fixture(name, seed)
            stops = name == c["fixture"] and seed in c["stops"]
            assert (int(s["status"][env]), int(s["err"][env])) == ((2, c["code"]) if stops else (1, 0)), (name, seed)
            assert (d["stop_error"] is not None) == stops
            assert first_mismatch(m.trace(env), trace) == -1, (name, seed)
            assert int(s["events"][env]) == d["events"] and "%016x" % int(s["hash"][env]) == d["hash"], (name, seed)
            assert int(s["current_time"][env]) == d["final_time"] and int(s["order_counter"][env]) == d["n_order_ids"]
            assert m.book(env, 0) == d["bids"] and m.book(env, 1) == d["asks"], (name, seed)
            assert _agents(m, env)[1:] == [(a["cash"], a["shares"], len(a["open_orders"])) for a in d["agents"]], (name, seed)
            (r,) = E.composition_runs(name, (seed,))
            assert_env(m, env, r, COMPOSITION_ERR, s, name)
        m.close()


@pytest.mark.parametrize("case", list(E.TAPE_CASES))
def test_gpu_tape_case_equals_oracle(mx, case):
    """three envs on the crafted tape, whole, pop by pop and in 7-pop launches; a further run
    changes nothing.  The TWAP stops (26 with one side of the book missing at 10:00, 25 with both)
    place nothing: the agent holds no order and the book is the tape's"""
    c = E.TAPE_CASES[case]
    tp, r = E.tape_run(case)
    t0 = time.time()
    m = mx.VecMarket(c["kind"], np.zeros(3, dtype=np.int64), tape=tp, symbol=tp.symbol, trace_cap=E.TRACE_CAP)
    for chunk in (1 << 20, 1, 7):
        s = run_bounded(m, chunk, r.events)
        assert (s["status"] == r.status).all() and (s["err"] == c["code"]).all(), (case, chunk, s["status"], s["err"])
        for env in range(3):
            assert_env(m, env, r, TAPE_ERR, s, "%s chunk %d" % (case, chunk), exchange=True)
        if c["twap"]:
            assert all(_agents(m, env)[2] == (0, 0, 0) for env in range(3))
        m.run()
        after = m.summary()
        assert all((after[k] == s[k]).all() for k in KEYS + ("err",)), (case, chunk)
        m.reset()
    m.close()
    print("%s: code %d after %d events, %.2f s" % (case, c["code"], r.events, time.time() - t0))


def _records(m):
    out = torch.zeros((m.n_envs, shard.RECORD_WORDS), dtype=torch.int64, device="cuda")
    m.write_records(out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_gpu_runner_handle_stop_is_sticky(mx):
    """a Kernel.runner handle (the late_start batch: envs 1 and 4 stop at pops 6 and 11).  Further
    launches change nothing in any env; mxa_write_records carries the code in its err word; a
    snapshot saved after 3 pops and restored revives the envs to reach the same stops; a masked
    reset of only the stopped envs rebuilds them and leaves the others alone"""
    c = E.COMPOSITION_CASES["late_start"]
    rs = E.composition_runs(c["fixture"], c["seeds"])
    n = len(rs)
    stopped = np.array([r.err != 0 for r in rs])
    assert stopped.sum() == 2
    longest = max(r.events for r in rs)

    def check(what):
        s = m.summary()
        for env, r in enumerate(rs):
            assert_env(m, env, r, COMPOSITION_ERR, s, what)
        return s

    m = mx.VecMarket(E.composition(c["fixture"]), c["seeds"], trace_cap=E.TRACE_CAP)
    m.launch(3)
    m.sync()
    assert (m.summary()["events"] == 3).all()
    snap = m.snapshot()
    snap.save()
    run_bounded(m, 1 << 20, longest)
    s = check("first run")
    m.run()
    m.launch(100)
    m.sync()
    again = m.summary()
    assert all((again[k] == s[k]).all() for k in KEYS + ("err",))
    check("after further launches")
    rec = _records(m)
    assert (rec[:, shard.R_ERR] == s["err"]).all() and (rec[:, shard.R_STATUS] == s["status"]).all()
    assert (rec[stopped, shard.R_ERR] == 6).all() and (rec[~stopped, shard.R_ERR] == 0).all()
    assert (rec[:, shard.R_EVENTS] == s["events"]).all()
    snap.restore()
    back = m.summary()
    assert (back["events"] == 3).all() and (back["status"] == 0).all() and (back["err"] == 0).all()
    run_bounded(m, 5, longest)
    check("after the restore")
    snap.close()
    m.reset(stopped.astype(np.uint8))
    r0 = m.summary()
    assert (r0["events"][stopped] == 0).all() and (r0["status"][stopped] == 0).all() and (r0["err"][stopped] == 0).all()
    assert all((r0[k][~stopped] == s[k][~stopped]).all() for k in KEYS + ("err",))
    run_bounded(m, 1 << 20, longest)
    check("after the masked reset")
    m.close()


def test_gpu_gym_handle_stop_is_sticky(mx):
    """a GymKernel handle (rmsc03 + DummyRL, zero actions): env 1 stops in its third step in
    get_observation (14), the others run on, each step's events the oracle's.  A further step
    returns the stopped env's observation unchanged with flag bit 2 set and changes nothing in it;
    the records carry the code; a snapshot of the first step restored reaches the same stop; a
    masked reset of env 1 rebuilds it alone.  The handle keeps its stop time (the way to
    ERR_RP_STOPPING that a caller's stop time would open is closed)"""
    runs = E.gym_runs()
    n = len(runs)
    zeros = np.zeros((n, 3))
    o1, steps1 = runs[1]
    v = VecABIDESEnv(seeds=E.GYM_SEEDS)
    assert v.L.mxa_set_stop_time(v._h, 35_000 * 10 ** 9) == EINVAL

    def step(i, what):
        obs, done, valid, err = v.step(zeros)
        s = v.summary()
        for e, (_, steps) in enumerate(runs):
            ev, o_done, rc, o_obs = steps[min(i, len(steps) - 1)]
            assert int(s["events"][e]) == ev, (what, i, e, int(s["events"][e]), ev)
            assert bool(err[e]) == (rc != 0) and int(s["err"][e]) == (14 if rc else 0), (what, i, e)
            assert (int(s["status"][e]) == 2) == (rc != 0), (what, i, e)
        return obs, v.flags.copy(), s

    step(0, "first")
    snap = v.snapshot()
    snap.save()
    step(1, "first")
    obs2, fl2, s2 = step(2, "first")
    assert fl2[1] & 4 and int(s2["hash"][1]) == o1.hash and int(s2["current_time"][1]) == o1.current_time
    assert v.book(1, 0) == o1.book(0) and v.book(1, 1) == o1.book(1)
    assert v.agents(1)[1:] == [tuple(a) for a in o1.agents()][1:]
    for i in (3, 4):
        obs, fl, s = step(i, "first")
        assert fl[1] & 4 and fl[1] & 1 and fl[1] == fl2[1]
        assert np.array_equal(obs[1].view(np.int64), obs2[1].view(np.int64))  # the sticky observation, bit for bit
        assert all(s[k][1] == s2[k][1] for k in KEYS + ("err",))
    rec = _records(v)
    assert rec[1, shard.R_ERR] == 14 and rec[1, shard.R_STATUS] == 2 and (np.delete(rec[:, shard.R_ERR], 1) == 0).all()
    snap.restore()
    for i in (1, 2):
        _, fl, s = step(i, "restored")
    assert fl[1] & 4 and all(s[k][1] == s2[k][1] for k in KEYS + ("err",))
    snap.close()
    mask = np.zeros(n, dtype=np.uint8)
    mask[1] = 1
    v.reset(mask=mask)
    r0 = v.summary()
    assert r0["events"][1] == 0 and r0["status"][1] == 0 and r0["err"][1] == 0 and v.flags[1] == 0 and not v.obs[1].any()
    assert all((np.delete(r0[k], 1) == np.delete(s[k], 1)).all() for k in KEYS + ("err",))
    v.step(zeros)
    r1 = v.summary()
    assert r1["events"][1] == steps1[0][0] and r1["status"][1] == 0
    for e in (0, 2):  # the others took their fourth step
        assert r1["events"][e] == runs[e][1][3][0]
    v.close()
