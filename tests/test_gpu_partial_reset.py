"""mxa_reset with an env mask (include/mxa.h): a vectorised RL loop restarts the envs that ended
while their neighbours keep running.  A rebuilt env starts from a block that still holds the cut
episode's saved queue, book, RNG windows and book-log count, and the next mxa_run compacts a list
in which finished, running and rebuilt envs are mixed.  Every env is compared with the C oracle
for the seed its episode was built from (events, per-pop hash, order counter, last trade, every
trading agent's cash / holdings / open orders), and an env the mask leaves alone keeps its whole
block byte for byte.  Kernel.runner handles of every queue shape, the settings that outlive a
reset (stop time, exchange log), the episode record's seed word, and GymKernel handles (order ids
carry over: mask value 2)."""
import os

import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process (write_records' device buffer)

import pyoracle
from golden_util import FNV_OFF, market_kw
from mxabides import shard
from test_gpu_records import _check as check_record_words

pytestmark = pytest.mark.gpu

NS = 10 ** 9
OPEN = (9 * 3600 + 30 * 60) * NS
SEEDS = [123456789, 1008, 7, 11, 2, 3, 5, 13]  # 1008 (and 13): a market maker that stalls on a one-sided book
NEW_SEEDS = [99, 17, 2024, 31, 1008, 4294967295, 8, 77]
MASK_MID = [1, 0, 1, 0, 1, 0, 1, 0]
MASK_END = [0, 1, 0, 0, 0, 0, 0, 1]


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


_ORACLE = {}


def oracle(cfg, seed, stop=None):
    """the oracle's record of one env run to the end (or to stopTime `stop`), computed once"""
    key = (cfg, seed, stop)
    if key not in _ORACLE:
        o = pyoracle.OracleEnv(cfg, seed)
        if stop is not None:
            o.set_stop(stop)
        o.run()
        assert o.error[0] == 0, o.error
        _ORACLE[key] = (o.events, o.hash, o.order_counter, o.last_trade, o.agents()[1:])
    return _ORACLE[key]


def records(m):
    """per-env (events, hash, order counter, last trade, every trading agent's cash / holdings / open orders)"""
    s = m.summary()
    assert (s["status"] != 2).all(), s["err"]
    return [(int(s["events"][i]), int(s["hash"][i]), int(s["order_counter"][i]), int(s["last_trade"][i]),
             [(a["cash"], a["shares"], a["n_open"]) for a in m.agents(i)[1:]]) for i in range(m.n_envs)]


def assert_oracle(m, cfg, seeds, stop=None, envs=None):
    s = m.summary()
    got = records(m)
    for i in (range(m.n_envs) if envs is None else envs):
        ref = oracle(cfg, int(seeds[i]), stop)
        assert s["status"][i] == 1, (i, s["status"][i])
        assert got[i][:4] == ref[:4], (i, got[i][:4], ref[:4])
        assert got[i][4] == ref[4], (i, [k for k, (a, b) in enumerate(zip(got[i][4], ref[4])) if a != b][:8])


def blocks(m):
    """every env's whole block, no word left out"""
    return [m.raw(i, 0, m.env_bytes) for i in range(m.n_envs)]


def assert_blocks_equal(a, b, envs, what):
    for i in envs:
        assert np.array_equal(a[i], b[i]), (what, i, np.nonzero(a[i] != b[i])[0][:16].tolist())


def sel(mask, v):
    return [i for i, x in enumerate(mask) if bool(x) == bool(v)]


def assert_reads_as_never_run(m, fresh, envs):
    """through the readers (nothing says a fresh allocation is zeroed): status, events, hash, every
    other summary word, both book sides and every agent as a handle that never ran"""
    s, f = m.summary(), fresh.summary()
    for i in envs:
        assert s["status"][i] == 0 and s["events"][i] == 0 and int(s["hash"][i]) == FNV_OFF, i
        for k in s:
            assert s[k][i] == f[k][i], (i, k, s[k][i], f[k][i])
        assert m.book(i, 0) == [] and m.book(i, 1) == [], i
        assert m.agents(i) == fresh.agents(i), i


def cut_rmsc03(mx, **kw):
    """rmsc03 x8 cut at 15,000 pops (three launches of 5,000): the stalled envs have ended, the
    others are mid-episode"""
    m = mx.VecMarket("rmsc03", SEEDS, **kw)
    m.set_parity_hash(True)
    assert m.run(chunk=5000, max_launches=3) == 3
    st = m.summary()["status"]
    assert any(st[i] == 0 for i in sel(MASK_MID, 1)) and any(st[i] == 0 for i in sel(MASK_MID, 0)), st
    return m


@pytest.mark.parametrize("chunk", [None, 997])
def test_gpu_masked_reset_mid_episode(mx, chunk):
    """A1: envs 0, 2, 4, 6 restart while 3 and 5 are mid-episode and 1 and 7 have ended"""
    m = cut_rmsc03(mx)
    before = blocks(m)
    m.reset(MASK_MID)
    assert_blocks_equal(before, blocks(m), sel(MASK_MID, 0), "reset")
    assert_reads_as_never_run(m, mx.VecMarket("rmsc03", SEEDS), sel(MASK_MID, 1))
    if chunk is None:
        m.run()
    else:
        m.run(chunk=chunk)
    assert_oracle(m, "rmsc03", SEEDS)  # the masked envs ran a fresh episode, the others continued theirs


def test_gpu_masked_reset_after_the_end(mx):
    """A2: finished envs restart (the stalled ones); a finished env is never loaded again"""
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    m.run()
    assert_oracle(m, "rmsc03", SEEDS)
    b0 = blocks(m)
    m.reset(MASK_END)
    b1 = blocks(m)
    assert_blocks_equal(b0, b1, sel(MASK_END, 0), "reset")
    for i in sel(MASK_END, 1):
        assert not np.array_equal(b0[i], b1[i]), i
    assert (m.summary()["status"][sel(MASK_END, 1)] == 0).all()
    m.run()
    b2 = blocks(m)
    assert_blocks_equal(b0, b2, sel(MASK_END, 0), "run")
    assert_oracle(m, "rmsc03", SEEDS)
    assert m.run() == 0  # nothing left to run: no launch, no block changes
    assert_blocks_equal(b2, blocks(m), range(m.n_envs), "run on a finished handle")


def test_gpu_masked_reset_with_new_seeds_and_the_record_seed(mx):
    """A3: set_seeds for every slot, then a masked reset mid-episode: a masked env runs new[i], the
    others finish old[i], and the episode record (mxa_write_records) names for every env the seed
    its episode was built from, before and after the run"""
    m = cut_rmsc03(mx)
    m.set_seeds(NEW_SEEDS)
    out = torch.zeros((m.n_envs, shard.RECORD_WORDS), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def record_rows():
        m.write_records(out.data_ptr())
        m.sync()
        return out.cpu().numpy()

    # set_seeds alone rebuilds nothing: every env is still in (or past) its episode of SEEDS
    check_record_words(record_rows(), m.summary(), SEEDS)
    m.reset(MASK_MID)
    built = [NEW_SEEDS[i] if MASK_MID[i] else SEEDS[i] for i in range(m.n_envs)]
    check_record_words(record_rows(), m.summary(), built)
    m.run()
    assert_oracle(m, "rmsc03", built)
    rec, s = record_rows(), m.summary()
    S = shard
    check_record_words(rec, s, built)
    assert (rec[:, S.R_LAST] == s["last_trade"]).all() and (rec[:, S.R_OCNT] == s["order_counter"]).all()
    assert (rec[:, S.R_ERR] == 0).all()
    for e in range(m.n_envs):
        ag = m.agents(e)[1:]
        assert rec[e, S.R_CASH] == sum(a["cash"] for a in ag)
        assert rec[e, S.R_HOLD] == sum(a["shares"] for a in ag) == 0
        assert rec[e, S.R_GAIN] == sum(a["cash"] + (a["last_trade"] * a["shares"] if a["shares"] else 0)
                                       - a["starting_cash"] for a in ag)
    # a whole-handle reset builds every env from the current seeds
    m.reset()
    check_record_words(record_rows(), m.summary(), NEW_SEEDS)


def test_gpu_stop_time_outlives_a_masked_reset(mx):
    """A4: mxa_set_stop_time is kept by a masked reset (the build clears the rebuilt envs' header)"""
    stop = OPEN + 3 * NS
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    m.set_stop_time(stop)
    m.run()
    assert_oracle(m, "rmsc03", SEEDS, stop)
    b0 = blocks(m)
    m.reset(MASK_MID)
    assert_blocks_equal(b0, blocks(m), sel(MASK_MID, 0), "reset")
    m.run()
    assert_oracle(m, "rmsc03", SEEDS, stop)
    assert_blocks_equal(b0, blocks(m), sel(MASK_MID, 0), "run")
    assert (m.summary()["events"] < 5000).all()  # nobody ran on to the config's stop


_STREAM = {}


def oracle_stream(seed):
    """rmsc03's book-update stream with the exchange log on, as the oracle records it"""
    if seed not in _STREAM:
        o = pyoracle.OracleEnv("rmsc03", seed)
        o.set_book_log()
        o.set_exchange_log()
        o.run()
        assert o.error[0] == 0
        _STREAM[seed] = o.book_records()
    return _STREAM[seed]


def test_gpu_exchange_log_outlives_a_masked_reset(mx):
    """A4: a masked env's book-update stream restarts at zero and is the oracle's record for
    record; an env left alone carries the oracle's whole stream, with no gap or repeat where the
    reset fell; the exchange-log switch stays fixed until a whole-handle reset"""
    m = cut_rmsc03(mx, book_log=1 << 20, exchange_log=True)
    mid = [len(m.book_log_records(i)) for i in range(m.n_envs)]
    assert all(n > 0 for n in mid)
    m.reset(MASK_MID)
    for i in range(m.n_envs):
        assert len(m.book_log_records(i)) == (0 if MASK_MID[i] else mid[i]), i
    with pytest.raises(mx.MxaError):
        m.set_exchange_log(False)
    m.run()
    assert_oracle(m, "rmsc03", SEEDS)
    for i, sd in enumerate(SEEDS):
        a, d = oracle_stream(sd), m.book_log_records(i)
        assert len(d) == len(a), (i, len(d), len(a))
        assert (d["t"] == a[:, 0]).all() and (d["price"] == a[:, 1]).all() and (d["qty"] == a[:, 2]).all(), i
    with pytest.raises(mx.MxaError):
        m.set_exchange_log(False)
    m.reset()
    m.set_exchange_log(False)  # accepted after a whole-handle reset


# (config, launch budget that leaves both envs mid-episode)
SHAPES = [("sparse_zi_1000", 5000, 2),      # grouped queue, payload in HBM
          ("random_fund_value", 5000, 2),   # two-tier queue, 5,101 agents
          ("rmsc03_sbmm", 2000, 2)]         # subscription table and ladder deques in the record


@pytest.mark.parametrize("cfg,chunk,launches", SHAPES)
def test_gpu_masked_reset_other_queue_shapes(mx, cfg, chunk, launches):
    """A5: env 0 restarts mid-episode, env 1 continues"""
    seeds = [123456789, 5]
    m = mx.VecMarket(cfg, seeds, **market_kw(cfg))
    m.set_parity_hash(True)
    assert m.run(chunk=chunk, max_launches=launches) == launches
    s = m.summary()
    assert (s["status"] == 0).all() and (s["events"] == chunk * launches).all(), s
    b0 = blocks(m)
    m.reset([1, 0])
    assert_blocks_equal(b0, blocks(m), [1], "reset")
    assert_reads_as_never_run(m, mx.VecMarket(cfg, seeds, **market_kw(cfg)), [0])
    m.run()
    assert_oracle(m, cfg, seeds)


# ---- GymKernel handles

from mxabides.gym import VecABIDESEnv  # noqa: E402
from test_oracle_rl import OBS_RTOL  # noqa: E402  (the comparison test_gpu_episodes defines)

RL_SEEDS = [123456789, 7, 11, 2024]
RL_NEW = [99, 1234, 5, 4321]  # entries 1 and 3 wait for a reset that never comes
RL_MASK = [1, 0, 1, 0]
RL_CUT, RL_STEPS = 10, 27


def gym_blocks(v):
    """every env's whole block of a GymKernel handle (mxa_read_raw)"""
    nb = v.L.mxa_env_bytes(v._h)
    out = []
    for i in range(v.n_envs):
        b = np.zeros(nb, dtype=np.uint8)
        v._check(v.L.mxa_read_raw(v._h, i, 0, nb, b.ctypes.data), "mxa_read_raw")
        out.append(b)
    return out


def _step_all(v, oras, alive, a, tag):
    obs, done, valid, err = v.step(a)
    for e in np.nonzero(alive)[0]:
        o_obs, o_done, rc = oras[e].step(a[e])
        assert bool(err[e]) == (rc != 0), (tag, e, rc)
        if rc:
            alive[e] = False
            continue
        assert bool(done[e]) == o_done, (tag, e)
        if o_obs is not None:
            np.testing.assert_allclose(obs[e], o_obs, rtol=OBS_RTOL, atol=1e-12, err_msg="%s env %d" % (tag, e))
        alive[e] = not o_done
    return obs


@pytest.mark.parametrize("persist", [True, False])
def test_gpu_rl_masked_reset(persist):
    """A6: rmsc03 + DummyRL x4, envs 0 and 2 restart with new seeds after 10 steps.  One process per
    env (the default): their order ids continue from the first episode (mask value 2).  After
    set_id_persistence(False) they are fresh processes, ids from 0.  Envs 1 and 3 step on either way."""
    n = len(RL_SEEDS)
    rs = np.random.RandomState(17)
    acts = rs.uniform(0, 1, (RL_CUT + RL_STEPS, n, 3))
    acts[..., 0] *= 0.02
    v = VecABIDESEnv(seeds=RL_SEEDS)
    v.set_parity_hash(True)
    oras = [pyoracle.OracleGymEnv(seed=s) for s in RL_SEEDS]
    alive = np.ones(n, dtype=bool)
    for i in range(RL_CUT):
        obs = _step_all(v, oras, alive, acts[i], "step %d" % i)
    assert alive.all()
    first = v.summary()["order_counter"].copy()
    flags0 = v.flags.copy()
    assert (first > 0).all() and obs.any(axis=1).all() and flags0.all()
    b0 = gym_blocks(v)
    if not persist:
        v.set_id_persistence(False)
    v.reset(seeds=RL_NEW, mask=RL_MASK)
    assert_blocks_equal(b0, gym_blocks(v), sel(RL_MASK, 0), "reset")
    for e in range(n):  # host rows: cleared for the masked envs only
        if RL_MASK[e]:
            assert not v.obs[e].any() and v.flags[e] == 0
            if persist:
                oras[e].reset(seed=RL_NEW[e])
            else:
                oras[e] = pyoracle.OracleGymEnv(seed=RL_NEW[e])
        else:
            assert (v.obs[e] == obs[e]).all() and v.flags[e] == flags0[e]
    s = v.summary()
    for e in range(n):
        assert s["events"][e] == oras[e].events and s["order_counter"][e] == oras[e].order_counter, e
        assert s["order_counter"][e] == (first[e] if persist or not RL_MASK[e] else 0), e
    for i in range(RL_CUT, RL_CUT + RL_STEPS):
        _step_all(v, oras, alive, acts[i], "step %d" % i)
        if not alive.any():
            break
    assert not alive.any()
    s = v.summary()
    for e in range(n):
        assert s["events"][e] == oras[e].events and s["hash"][e] == oras[e].hash, e
        assert s["order_counter"][e] == oras[e].order_counter, e
        assert v.agents(e)[1:] == [tuple(x) for x in oras[e].agents()][1:], e
    # the same second episode as a fresh process: same length, ids from 0
    for e in sel(RL_MASK, 1):
        f = pyoracle.OracleGymEnv(seed=RL_NEW[e])
        for i in range(RL_CUT, RL_CUT + RL_STEPS):
            if f.step(acts[i, e])[1:] != (False, 0):
                break
        assert f.events == s["events"][e], e
        if persist:
            assert s["order_counter"][e] == f.order_counter + first[e] and s["hash"][e] != f.hash, e
        else:
            assert s["order_counter"][e] == f.order_counter and s["hash"][e] == f.hash, e


def test_gpu_replay_masked_reset():
    """A6: the replay handle (IBM 2003-01-14) x4 with an action stream per env; env 1 restarts
    mid-episode (the tape's explicit ids and the auto ids carry over) while the others step on"""
    from mxabides import tape
    tp = tape.Tape.load(os.path.join(os.path.dirname(__file__), "golden", "tape_IBM_2003-01-14.npz"))
    n, cut, cap = 4, 40, 1200
    rs = np.random.RandomState(23)
    acts = np.stack([rs.uniform(0, 0.05, (cap, n)) * np.arange(1, n + 1), rs.uniform(0, 1, (cap, n)),
                     rs.uniform(0, 1, (cap, n))], 2)
    v = VecABIDESEnv(tp, n)
    v.set_parity_hash(True)
    oras = [pyoracle.OracleGymEnv(tp) for _ in range(n)]
    alive = np.ones(n, dtype=bool)
    for i in range(cut):
        _step_all(v, oras, alive, acts[i], "step %d" % i)
    assert alive.all()
    first = v.summary()["order_counter"].copy()
    b0 = gym_blocks(v)
    v.reset(mask=[0, 1, 0, 0])
    oras[1].reset()
    assert_blocks_equal(b0, gym_blocks(v), [0, 2, 3], "reset")
    s1 = v.summary()
    for e in range(n):
        assert s1["events"][e] == oras[e].events and s1["order_counter"][e] == oras[e].order_counter, e
    assert s1["events"][1] == 0 and s1["order_counter"][1] >= first[1] > 0
    steps = cut
    while alive.any():
        assert steps < cap, "the episodes did not end within %d steps" % cap
        _step_all(v, oras, alive, acts[steps], "step %d" % steps)
        steps += 1
    s = v.summary()
    for e in range(n):
        assert s["events"][e] == oras[e].events and s["hash"][e] == oras[e].hash, e
        assert s["order_counter"][e] == oras[e].order_counter, e
        assert v.book(e, 0) == oras[e].book(0) and v.book(e, 1) == oras[e].book(1), e
        assert v.agents(e) == [tuple(x) for x in oras[e].agents()], e
