"""The run kernel's variate tables (DESIGN.md §3 "Variate tables"; include/mxa_variates.h): a draw
taken from a table must be the serial draw bit for bit, value and stream state, and the engine with
its tables must stay the C oracle's episode through chunked launches, resets onto other seeds
(stream positions restart: the stale-table case), snapshots, restores and forks.

The probe runs one script of draws through a table and through the serial code on one wave and
returns both; the engine tests run rmsc03 x64 with the parity hash on and read the tables' hit, fill
and fall-back counts, so none of them can pass with the table path dead."""
import numpy as np
import pytest

import pyoracle
from test_gpu_partial_reset import oracle, records

pytestmark = pytest.mark.gpu

SEED0 = 123456789  # bench.py's seeds: SEED0 + global env index
SEEDS = [SEED0 + i for i in range(63)] + [1008]  # 1008: the market maker that stalls on a one-sided book
OTHER = [(7919 * i + 11) & 0xFFFFFFFF for i in range(64)]
HALF = 60000  # pops: about half of an rmsc03 episode (the full envs take about 127,000)

EXP, GAUSS, U32, RANDINT = 0, 1, 2, 3
N = 3000  # draws per script: about 15 MT blocks of an alternating script
ALT = [EXP, GAUSS] * (N // 2)


def _every(script, k, kind):
    s = list(script)
    for i in range(k - 1, len(s), k):
        s[i] = kind
    return s


# name -> (script, lookahead words)
SCRIPTS = {
    "alternating": (ALT, 256),
    "gauss_only": ([GAUSS] * N, 256),                    # the oracle stream's pattern
    "stray_u32": (_every(ALT, 50, U32), 256),            # odd alignment: forced refills
    "stray_randint": (_every(ALT, 50, RANDINT), 256),    # one or more words, by rejection
    "cached_start": ([GAUSS] + ALT[:-1], 256),           # the alternating script from a cached gauss
    "lookahead_2": (ALT, 2),                             # spans of one double: no attempt fits
    "lookahead_3": (ALT, 3),
    "lookahead_4": (ALT, 4),                             # two doubles: the second attempt's partner is outside
}


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def probe(L, seed, script, lookahead):
    s = np.asarray(script, dtype=np.uint8)
    out = np.zeros((2, len(s)), dtype=np.float64)
    state = np.zeros((2, len(s), 3), dtype=np.uint64)
    assert L.mxa_variate_probe(0, seed, s.ctypes.data, len(s), lookahead, out.ctypes.data, state.ctypes.data) == 0
    return out, state


@pytest.mark.parametrize("seed", [0, 424242, 4294967295])
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_probe_table_path_equals_serial_path(mx, name, seed):
    """values and (position, gauss flag, cached gauss) after every draw, bit for bit"""
    script, la = SCRIPTS[name]
    out, state = probe(mx.load(), seed, script, la)
    bad = np.nonzero(out[0].view(np.uint64) != out[1].view(np.uint64))[0]
    assert len(bad) == 0, (name, seed, int(bad[0]), out[0][bad[0]], out[1][bad[0]])
    bad = np.nonzero((state[0] != state[1]).any(axis=1))[0]
    assert len(bad) == 0, (name, seed, int(bad[0]), state[0][bad[0]].tolist(), state[1][bad[0]].tolist())
    assert int(state[0][-1][0]) > 624 + N  # the script drew: positions moved past a block and more


@pytest.mark.parametrize("seed", [0, 424242, 4294967295])
@pytest.mark.parametrize("name", ["alternating", "gauss_only"])
def test_probe_table_path_equals_numpy(mx, name, seed):
    """the table pass against numpy.random.RandomState itself, one draw at a time, bit patterns"""
    script, la = SCRIPTS[name]
    out, _ = probe(mx.load(), seed, script, la)
    r = np.random.RandomState(seed)
    ref = np.array([float(r.standard_exponential() if k == EXP else r.standard_normal()) for k in script])
    bad = np.nonzero(out[0].view(np.uint64) != ref.view(np.uint64))[0]
    assert len(bad) == 0, (name, seed, int(bad[0]), out[0][bad[0]], ref[bad[0]])


def test_probe_refuses_bad_arguments(mx):
    L = mx.load()
    s = np.zeros(4, dtype=np.uint8)
    o = np.zeros(8)
    st = np.zeros(24, dtype=np.uint64)
    good = [0, 1, s.ctypes.data, 4, 256, o.ctypes.data, st.ctypes.data]
    for i, v in [(2, None), (3, 0), (4, 1), (4, 257), (5, None), (6, None)]:
        a = list(good)
        a[i] = v
        assert L.mxa_variate_probe(*a) == -1, (i, v)
    s[2] = 4
    assert L.mxa_variate_probe(*good) == -1  # a script byte above 3


# ---- the engine: rmsc03 x64 against the C oracle

_REF = {}


def reference(seeds):
    """per-env (events, hash) of the C oracle's batch run and its per-seed record, computed once"""
    key = tuple(seeds)
    if key not in _REF:
        from concurrent.futures import ThreadPoolExecutor
        ev, hs, _ = pyoracle.run_batch("rmsc03", np.array(seeds, dtype=np.uint32), threads=16)
        with ThreadPoolExecutor(16) as ex:
            rec = list(ex.map(lambda s: oracle("rmsc03", int(s)), seeds))
        for i in range(len(seeds)):
            assert rec[i][0] == ev[i] and rec[i][1] == int(hs[i]), i
        _REF[key] = rec
    return _REF[key]


def assert_reference(m, seeds, envs=None):
    ref, got = reference(seeds), records(m)
    assert (m.summary()["status"] == 1).all()
    for i in (range(m.n_envs) if envs is None else envs):
        assert got[i] == ref[i], (i, got[i][:4], ref[i][:4])


def market(mx, seeds=SEEDS):
    m = mx.VecMarket("rmsc03", seeds)
    m.set_parity_hash(True)
    return m


def test_engine_equals_oracle_and_takes_the_tables(mx):
    """one launch: every env is the oracle's episode; per user (words 6-8 the oracle stream, 9-11
    the value agents' streams) at least nine draws in ten came from a table and fills happened.
    The same episode in launches of 1,000 pops (the oracle table is dropped at every launch start)"""
    m = market(mx)
    m.inplace_groups()  # clear what earlier runs of this process left
    m.run()
    g = m.inplace_groups().astype(np.int64)
    print("variate tables (hits, fills, fall-backs): oracle stream %s, value agents %s" % (g[6:9].tolist(), g[9:12].tolist()))
    assert_reference(m, SEEDS)
    for u in (6, 9):
        hits, fills, serial = g[u:u + 3]
        assert fills > 0 and hits >= 0.9 * (hits + serial), (u, g[6:12].tolist())
    c = market(mx)
    c.run(chunk=1000)
    assert_reference(c, SEEDS)
    g = c.inplace_groups().astype(np.int64)
    assert g[6] > 0 and g[9] > 0, g.tolist()


def test_engine_reset_onto_other_seeds(mx):
    """half an episode, then other seeds and a reset: every stream restarts at position 624, where
    the old episode's tables must not answer.  Equals the oracle on the new seeds"""
    m = market(mx)
    assert m.run(chunk=HALF, max_launches=1) == 1
    assert (m.summary()["status"] == 0).sum() >= 32  # most envs are mid-episode
    m.set_seeds(OTHER)
    m.reset()
    m.run()
    assert_reference(m, OTHER)


def test_engine_snapshot_restore_and_fork(mx):
    """a snapshot at half an episode, run on, restore, run on: the uninterrupted episode.  Then env 3's
    saved state forked into slot 5 as well: both continue as env 3's seed"""
    m = market(mx)
    assert m.run(chunk=HALF, max_launches=1) == 1
    snap = m.snapshot()
    snap.save()
    m.run(chunk=20000, max_launches=1)
    snap.restore()
    m.run()
    assert_reference(m, SEEDS)
    fork = [-1] * 64
    fork[3] = fork[5] = 3
    snap.restore(fork)
    assert (m.summary()["status"][[3, 5]] == 0).all()
    m.run()
    got, ref = records(m), reference(SEEDS)
    assert got[3] == ref[3] and got[5] == ref[3]
    assert_reference(m, SEEDS, envs=[i for i in range(64) if i != 5])
    snap.close()
