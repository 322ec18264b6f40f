"""The RNG streams' LDS windows (DESIGN.md §3 "RNG stream windows", Appendix R.12): where the
configuration's MXA_TEMPER_FILL_MASK bit is set (rmsc03, sparse_zi_100, value_noise) the windows of
the global streams G/O/K/L hold tempered outputs, the unit's stream handles are typed at compile time
and o_observe holds one o_advance.  An agent's own stream is not windowed in any build (the window
built for it did not pass its A/B and was taken out again, Appendix R.12): its draws read HBM.
Every result stays bit for bit: whole rmsc03 episodes against the oracle in one launch and in ~160
launches (every window lost and refilled at each boundary), a cached second gauss consumed launches
after it was made, streams that cross MT block boundaries, and rmsc03_rl's step kernel (outside the
mask: the parent's code) against the oracle's GymKernel.

Stream positions are read through mxa_read_raw at mxa_layout.h's offsets (as
test_gpu_limit_inplace.py's HDR_LAUNCH_LOCAL reads the header): mxa_read_agents does not return them
and the C-ABI stays as it is.
Agent record: AF_RS_POS (dword 32, the stream's output index; the first output is 624, block b holds
624 b .. 624 b + 623) and AF_RS_HASG (dword 33, bit 0: the legacy_gauss cache holds the polar
method's second value).  Header: EnvHdr.rs_pos[4] (bytes 168-183), the same index for G, O, K, L."""
import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process

import pyoracle
import test_gpu_limit_inplace as W
from golden_util import first_mismatch, load
from test_oracle_episodes import OBS_RTOL

pytestmark = pytest.mark.gpu

SEED0 = 123456789  # bench.py's seeds: SEED0 + global env index
SEEDS = [SEED0 + i for i in range(4)]
VALUE = range(51, 61)  # rmsc03's ValueAgents (config/rmsc03.py)
AF_RS_POS, AF_RS_HASG, AGENT_BYTES, MT_N = 32, 33, 512, 624


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


_ORACLE = []


def oracle():
    """whole rmsc03 episodes of SEEDS under the oracle, once: (events, hash, order counter, last
    trade, every trading agent's cash / holdings / open orders) per env, as W.records gives them"""
    if not _ORACLE:
        for sd in SEEDS:
            o = pyoracle.OracleEnv("rmsc03", sd)
            o.run()
            assert o.error[0] == 0, o.error
            _ORACLE.append((o.events, o.hash, o.order_counter, o.last_trade, o.agents()[1:]))
    return _ORACLE


def stream_words(m, env):
    """[n_agents][2] (AF_RS_POS, AF_RS_HASG) of every agent record of `env`"""
    rec = m.raw(env, m.layout()["ag"], m.n_agents * AGENT_BYTES).view(np.uint32).reshape(m.n_agents, AGENT_BYTES // 4)
    return rec[:, [AF_RS_POS, AF_RS_HASG]].astype(np.int64)


_ONE = []


def one_launch(mx):
    """the one-launch run of SEEDS (parity hash on), shared by the tests below and left as it is"""
    if not _ONE:
        m = mx.VecMarket("rmsc03", SEEDS)
        m.set_parity_hash(True)
        assert m.run() == 1
        _ONE.append(m)
    return _ONE[0]


def test_gpu_rmsc03_full_episodes_equal_oracle(mx):
    """4 envs with the benchmark's seeds, one launch: events, hash, order counter, last trade and
    every agent's final cash, holdings and open orders are the oracle's.  Prints the furthest any
    agent's own stream got: rmsc03's value agents stay inside block 1 (the block-boundary case is
    test_gpu_stream_crosses_block_boundaries_while_windowed's)"""
    m = one_launch(mx)
    s = m.summary()
    assert (s["status"] == 1).all(), s["err"]
    for i, (got, ref) in enumerate(zip(W.records(m), oracle())):
        assert got[:-1] == ref[:-1], (i, got[:-1], ref[:-1])
        assert got[-1] == ref[-1], (i, [k for k, (a, b) in enumerate(zip(got[-1], ref[-1])) if a != b])
    pos = np.stack([stream_words(m, e)[1:, 0] for e in range(len(SEEDS))])
    print("rmsc03 agent streams: words drawn, max %d (agent %d), value agents max %d" % (
        pos.max() - MT_N, 1 + int(pos.max(0).argmax()), pos[:, VALUE.start - 1:VALUE.stop - 1].max() - MT_N))
    assert (pos[:, VALUE.start - 1:VALUE.stop - 1] > MT_N).all()  # every value agent drew from its own stream


def test_gpu_rmsc03_chunked_launches_and_gauss_cache(mx):
    """the same episodes in launches of 1000 pops (~160 boundaries; a launch keeps no window, so
    every stream refills at each): env blocks byte-identical to the one-launch run (mxa_read_raw,
    the launch-local header words apart, as W.raw_state), and the oracle's records.

    The gauss cache: a value agent's observation noise is one legacy_gauss per wake, so a wake
    whose polar draw caches the second value (AF_RS_HASG bit 0) is followed by a wake that takes
    it without drawing a word.  Read at every launch boundary: some value agent's bit is 1 at one
    boundary and 0 at a later one, which only a consumed cache does (a fresh polar draw sets it),
    with the window it was drawn through long gone.  The fixture event: the first such pair is
    printed (env, agent, launches); the values themselves are pinned by the hash"""
    one = one_launch(mx)
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    hasg, launches = [], 0
    while (m.summary()["status"] == 0).any():
        assert m.run(chunk=1000, max_launches=1) == 1
        launches += 1
        assert launches < 1000
        hasg.append(np.stack([stream_words(m, e)[VALUE.start:VALUE.stop, 1] & 1 for e in range(len(SEEDS))]))
    hasg = np.stack(hasg)  # [launch][env][value agent]
    print("launches", launches)
    assert launches >= 100
    for i, (got, ref) in enumerate(zip(W.records(m), oracle())):
        assert got == ref, i
    W.assert_same_blocks(W.raw_state(m), W.raw_state(one), "chunk=1000")
    made = np.argwhere((hasg[:-1] == 1) & (hasg[1:] == 0))
    assert len(made) > 0, "no cached gauss was consumed across a launch boundary"
    k, e, a = made[0]
    print("cached gauss of env %d agent %d: held after launch %d, consumed in launch %d; %d such pairs" % (
        e, VALUE.start + a, k + 1, k + 2, len(made)))
    assert len(made) >= len(SEEDS) * len(VALUE)  # every value agent, many times over


@pytest.mark.parametrize("cfg,seed", [("sparse_zi_100", 123456789), ("rmsc01", 7)])
def test_gpu_streams_cross_block_boundaries(mx, cfg, seed):
    """reference fixtures whose streams leave blocks 1 and 2 (a position past 1248: block 2 was
    generated into block 0's half of the double buffer while draws went on) and every later block in
    turn; rmsc03's and value_noise's agents stay inside block 1 (value_noise seed 7: 59 words at most).
    The windowed crossing of the shipped build is sparse_zi_100's (seed 123456789, in
    MXA_TEMPER_FILL_MASK): its global streams O and L draw through tempered windows across many
    block boundaries.  rmsc01 seed 7 adds an agent's own stream that crosses (the MarketMakerAgent
    draws its ladder's sizes at every wake), but not windowed: rmsc01 is outside the mask (it
    measured neutral), so all its draws go through the unchanged handle that tests the window
    pointer, the agent's from HBM.  The case found is printed.  The trace, events and hash are the
    reference's own"""
    d, ref = load(cfg, seed)
    m = mx.VecMarket(cfg, [seed], trace_cap=len(ref))
    m.run()
    s = m.summary()
    assert s["status"][0] == 1, "env error %d" % s["err"][0]
    pos = stream_words(m, 0)[1:, 0]
    gpos = m.raw(0, 168, 16).view(np.int32)
    past = int((pos > 2 * MT_N).sum())
    print("%s seed %d: global streams G/O/K/L at %s; %d of %d agent streams end past 1248, furthest %d (block %d, agent %d)" % (
        cfg, seed, gpos.tolist(), past, len(pos), pos.max(), pos.max() // MT_N, 1 + int(pos.argmax())))
    assert gpos[1] > 2 * MT_N, gpos  # the oracle stream O (G draws only the megashocks)
    if cfg == "rmsc01":
        assert past > 0, pos.max()
    assert first_mismatch(m.trace(0), ref) == -1
    assert int(s["events"][0]) == d["events"] and "%016x" % int(s["hash"][0]) == d["hash"]


def test_gpu_rmsc03_rl_steps_equal_oracle(mx):
    """the step kernel: 4 envs of rmsc03 + DummyRL, 3 ABIDESEnv.steps with fixed actions, against
    the oracle's GymKernel (events, hash, the last observation)"""
    from mxabides.gym import ACTION_SIZE, VecABIDESEnv
    n, k = len(SEEDS), 3
    acts = np.random.RandomState(41).uniform(0, 1, (k, n, ACTION_SIZE))
    acts[:, :, 0] *= 0.05
    r = pyoracle.gym_batch(acts, 4, seeds=np.array(SEEDS, dtype=np.uint32))
    assert (r["err"] == 0).all(), r["err"]
    v = VecABIDESEnv(seeds=SEEDS)
    v.set_parity_hash(True)
    v.reset()
    obs = None
    for i in range(k):
        o, done, valid, err = v.step(acts[i])
        assert not np.asarray(err).any(), v.summary()["err"]
        obs = np.where(np.asarray(valid, dtype=bool)[:, None], o, obs if obs is not None else o)
    s = v.summary()
    assert (s["events"] == r["events"]).all() and (s["hash"] == r["hash"]).all(), (s["events"], r["events"])
    np.testing.assert_allclose(obs, r["obs"], rtol=OBS_RTOL, atol=1e-12)