"""Env-state snapshots (include/mxa_snap.h): envs saved mid-episode into device slots,
restored and forked from them.  "Restore, then continue" must reproduce what the C oracle computes
for an uninterrupted run of the seed the state was built from (events, per-pop hash, order counter,
last trade, every agent), a restored env is the saved block byte for byte, and an env the map leaves
out keeps every byte.  Kernel.runner handles of every queue shape, the book-update log with the
exchange's own log, the episode record's seed word, GymKernel handles (rmsc03 + DummyRL, the IBM
replay) with their host obs / flags rows, and everything the calls refuse."""
import ctypes
import os

import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process (write_records' device buffer)

import pyoracle
from golden_util import market_kw
from mxabides import shard
from mxabides.gym import VecABIDESEnv
from test_gpu_partial_reset import (SEEDS, SHAPES, RL_SEEDS, _step_all, assert_blocks_equal, assert_oracle, blocks,
                                    cut_rmsc03, gym_blocks, oracle_stream)
from test_gpu_records import _check as check_record_words

pytestmark = pytest.mark.gpu

ALL = range(len(SEEDS))


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def status(m):
    return m.summary()["status"]


def test_gpu_snapshot_identity_save_restore(mx):
    """1: rmsc03 x8 cut at 15,000 pops, saved whole; each restore is the saved bytes, each
    continuation the oracle's episode, and one schedule twice gives the same end bytes"""
    m = cut_rmsc03(mx)
    snap = m.snapshot()
    assert (snap.n_slots, snap.slot_bytes, snap.filled, snap.has_log) == (8, m.env_bytes + 256, 0, False)
    snap.save()
    assert snap.filled == 8
    saved = blocks(m)
    m.run()
    assert_oracle(m, "rmsc03", SEEDS)
    end = blocks(m)
    snap.restore()
    assert_blocks_equal(saved, blocks(m), ALL, "restore")
    m.run(chunk=997)
    assert_oracle(m, "rmsc03", SEEDS)
    snap.restore()
    assert_blocks_equal(saved, blocks(m), ALL, "second restore")
    m.run()
    assert_oracle(m, "rmsc03", SEEDS)
    assert_blocks_equal(end, blocks(m), ALL, "the first continuation's schedule again")
    snap.close()
    with pytest.raises(mx.MxaError):
        snap.n_slots  # closed


def test_gpu_snapshot_partial_restore(mx):
    """2: envs 0, 2, 4, 6 go back to the cut while 3 and 5 are 10,000 pops further on and 1 and 7
    have ended"""
    m = cut_rmsc03(mx)
    snap = m.snapshot()
    snap.save()
    saved = blocks(m)
    assert m.run(chunk=5000, max_launches=2) == 2
    st = status(m)
    assert st[1] == 1 and st[7] == 1 and st[3] == 0 and st[5] == 0, st
    b1 = blocks(m)
    smap = [0, -1, 2, -1, 4, -1, 6, -1]
    snap.restore(smap)
    b2 = blocks(m)
    assert_blocks_equal(b1, b2, [1, 3, 5, 7], "restore, envs left out")
    assert_blocks_equal(saved, b2, [0, 2, 4, 6], "restore")
    m.run()
    assert_blocks_equal(b1, blocks(m), [1, 7], "run, finished envs")
    assert_oracle(m, "rmsc03", SEEDS)
    # the same through a dict, on a finished handle: the others keep their end bytes
    end = blocks(m)
    snap.restore({2: 2})
    assert_blocks_equal(end, blocks(m), [0, 1, 3, 4, 5, 6, 7], "restore of env 2 alone")
    assert status(m)[2] == 0
    m.run(chunk=997)
    assert_blocks_equal(end, blocks(m), [0, 1, 3, 4, 5, 6, 7], "run of env 2 alone")
    assert_oracle(m, "rmsc03", SEEDS)


def test_gpu_snapshot_fork_and_bank(mx):
    """3: a 2-slot bank of envs 3 and 5 feeds all eight envs; the episode record names the seed each
    state was built from; env 1 (seed 1008, ended before the cut) runs again from a running slot"""
    m = cut_rmsc03(mx)
    assert status(m)[1] == 1 and status(m)[3] == 0 and status(m)[5] == 0
    bank = m.snapshot(2)
    bank.save({3: 0, 5: 1})
    assert (bank.n_slots, bank.filled) == (2, 2)
    b0 = blocks(m)
    out = torch.zeros((m.n_envs, shard.RECORD_WORDS), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def record_rows():
        m.write_records(out.data_ptr())
        m.sync()
        return out.cpu().numpy()

    check_record_words(record_rows(), m.summary(), SEEDS)
    m.set_seeds([1, 2, 3, 4, 5, 6, 7, 8])  # the next reset's seeds: no part of a snapshot, not read by a restore
    bank.restore([0, 0, 0, 0, 1, 1, 1, 1])
    built = [SEEDS[3]] * 4 + [SEEDS[5]] * 4
    b1 = blocks(m)
    for e in ALL:
        assert np.array_equal(b1[e], b0[3 if e < 4 else 5]), e
    assert (status(m) == 0).all()
    check_record_words(record_rows(), m.summary(), built)
    m.run()
    assert_oracle(m, "rmsc03", built)
    check_record_words(record_rows(), m.summary(), built)
    m.reset()  # d_seeds was left alone
    check_record_words(record_rows(), m.summary(), [1, 2, 3, 4, 5, 6, 7, 8])


@pytest.mark.parametrize("cfg,chunk,launches", SHAPES)
def test_gpu_snapshot_other_queue_shapes(mx, cfg, chunk, launches):
    """4: the grouped queue, the two-tier queue and the subscription table: env 0 goes back to the
    cut after both have finished, env 1 keeps its bytes"""
    seeds = [123456789, 5]
    m = mx.VecMarket(cfg, seeds, **market_kw(cfg))
    m.set_parity_hash(True)
    assert m.run(chunk=chunk, max_launches=launches) == launches
    assert (status(m) == 0).all()
    snap = m.snapshot()
    snap.save()
    saved = blocks(m)
    m.run()
    assert_oracle(m, cfg, seeds)
    end = blocks(m)
    snap.restore({0: 0})
    b = blocks(m)
    assert_blocks_equal(saved, b, [0], "restore")
    assert_blocks_equal(end, b, [1], "restore, env left out")
    m.run()
    assert_oracle(m, cfg, seeds)
    assert_blocks_equal(end, blocks(m), [1], "run")


def assert_streams(m, seeds, envs=None):
    for i in (range(m.n_envs) if envs is None else envs):
        a, d = oracle_stream(int(seeds[i])), m.book_log_records(i)
        assert len(d) == len(a), (i, len(d), len(a))
        assert (d["t"] == a[:, 0]).all() and (d["price"] == a[:, 1]).all() and (d["qty"] == a[:, 2]).all(), i


def test_gpu_snapshot_book_and_exchange_log(mx):
    """5: the book-update log rows travel with the env: after save, run, restore, run every stream is
    the oracle's record for record, and a forked env carries its source's stream"""
    cap = 1 << 20
    m = cut_rmsc03(mx, book_log=cap, exchange_log=True)
    snap = m.snapshot()
    assert snap.has_log and snap.slot_bytes == m.env_bytes + 256 + 16 * cap
    snap.save()
    mid = [len(m.book_log_records(i)) for i in ALL]
    assert all(n > 0 for n in mid)
    m.run()
    assert_oracle(m, "rmsc03", SEEDS)
    assert_streams(m, SEEDS)
    snap.restore()
    assert [len(m.book_log_records(i)) for i in ALL] == mid
    for i in ALL:  # the restored rows are the stream's first rows
        a, d = oracle_stream(SEEDS[i]), m.book_log_records(i)
        assert (d["t"] == a[:mid[i], 0]).all() and (d["price"] == a[:mid[i], 1]).all(), i
    m.run(chunk=997)
    assert_oracle(m, "rmsc03", SEEDS)
    assert_streams(m, SEEDS)
    # a fork: envs 0 and 1 take env 3's state and its rows (env 0's own finished stream is longer)
    snap.restore({0: 3, 1: 3})
    assert len(m.book_log_records(0)) == mid[3] and len(m.book_log_records(1)) == mid[3]
    m.run()
    built = [SEEDS[3], SEEDS[3]] + SEEDS[2:]
    assert_oracle(m, "rmsc03", built)
    assert_streams(m, built)
    # a whole-handle reset lets the exchange log be switched; a restore brings back envs that have
    # popped events, so the switch is fixed again
    m.reset()
    snap.restore()
    with pytest.raises(mx.MxaError):
        m.set_exchange_log(False)
    # the log reallocated at another capacity: the snapshot's rows no longer fit the handle
    m.set_book_log(1 << 12)
    after_realloc = blocks(m)
    for call in (snap.save, snap.restore):
        with pytest.raises(mx.MxaError, match="mxa_set_book_log"):
            call()
    assert_blocks_equal(after_realloc, blocks(m), ALL, "refused")


# ---- GymKernel handles

RL_CUT, RL_MORE, RL_CAP = 10, 5, 60


def rl_actions(seed, steps, n, scale=0.02):
    a = np.random.RandomState(seed).uniform(0, 1, (steps, n, 3))
    a[..., 0] *= scale
    return a


def fork_streams():
    """fork(0)'s branches: four action streams [step][env][3] from one state, from no volume at all to
    the whole parent order in every step"""
    a = np.random.RandomState(31).uniform(0, 1, (RL_CAP, 4, 3))
    a[..., 0] *= np.array([0.0, 0.02, 0.3, 1.0])[None, :]
    return a


def assert_gym_equals_oracles(v, oras, tag):
    s = v.summary()
    for e, o in enumerate(oras):
        assert s["events"][e] == o.events and s["hash"][e] == o.hash, (tag, e)
        assert s["order_counter"][e] == o.order_counter, (tag, e)
        assert v.agents(e)[1:] == [tuple(x) for x in o.agents()][1:], (tag, e)


def test_gpu_snapshot_rl(mx):
    """6: rmsc03 + DummyRL x4: saved after 10 steps, 5 steps of actions A, restored (block, host
    obs / flags rows, order counter), then actions B to the end against fresh oracles fed the prefix
    and B"""
    n = len(RL_SEEDS)
    pre, A, B = rl_actions(17, RL_CUT, n), rl_actions(18, RL_MORE, n, 0.3), rl_actions(19, RL_CAP, n, 0.1)
    v = VecABIDESEnv(seeds=RL_SEEDS)
    v.set_parity_hash(True)
    oras = [pyoracle.OracleGymEnv(seed=s) for s in RL_SEEDS]
    alive = np.ones(n, dtype=bool)
    for i in range(RL_CUT):
        obs = _step_all(v, oras, alive, pre[i], "prefix %d" % i)
    assert alive.all()
    snap = v.snapshot()
    snap.save()
    saved, obs0, flags0 = gym_blocks(v), v.obs.copy(), v.flags.copy()
    oc0 = v.summary()["order_counter"].copy()
    assert (obs0 == obs).all() and flags0.all() and (oc0 > 0).all()
    for i in range(RL_MORE):
        v.step(A[i])
    s = v.summary()
    assert (s["order_counter"] > oc0).all() and not (v.obs == obs0).all()
    snap.restore()
    assert_blocks_equal(saved, gym_blocks(v), range(n), "restore")
    assert (v.obs == obs0).all() and (v.flags == flags0).all()
    assert (v.summary()["order_counter"] == oc0).all()
    assert_gym_equals_oracles(v, oras, "restore")
    for i in range(RL_CAP):
        _step_all(v, oras, alive, B[i], "B %d" % i)
        if not alive.any():
            break
    assert not alive.any()
    assert_gym_equals_oracles(v, oras, "end of B")

    # a partial restore puts back the restored envs' host rows only
    end_obs, end_flags = v.obs.copy(), v.flags.copy()
    snap.restore({1: 1})
    assert (v.obs[1] == obs0[1]).all() and v.flags[1] == flags0[1]
    for e in (0, 2, 3):
        assert (v.obs[e] == end_obs[e]).all() and v.flags[e] == end_flags[e], e


@pytest.mark.parametrize("seed,err_step", [(123456789, None), (4, 12)])
def test_gpu_snapshot_rl_fork(mx, seed, err_step):
    """6: fork(0) after the prefix and four different action streams: each env equals an oracle of
    env 0's seed fed the prefix and the env's own stream, step by step and at the end.  Seed
    123456789: four different whole episodes.  Seed 4: every branch ends in the reference's
    ValueError (get_observation on an empty book side) 13 steps after the fork, each with its own
    events and hash.
    The issue asks for a stream whose branch alone ends in that ValueError while its siblings go on.
    The CPU oracle gives none: over seeds 1..45,999 with this prefix, the streams (0, .5, .5),
    (1, 1, 0), (1, 0, 1), (0.3, .5, .5) and (0.05, .5, .5) constant for 40 steps, and 40 random
    streams on each of eleven seeds that raise after the prefix, every branch of a seed ended at
    the same step in the same way.  DummyRL's orders are passive bids at the first two bid levels,
    cancelled before each observation, so whether a book side is empty at an observation did not
    once depend on them."""
    n = 4
    seeds = [seed, 7, 11, 2024]
    pre = rl_actions(17, RL_CUT, n)
    v = VecABIDESEnv(seeds=seeds)
    v.set_parity_hash(True)
    for i in range(RL_CUT):
        obs, done, valid, err = v.step(pre[i])
        assert not done[0] and not err[0], i
    b0, obs0, flags0 = gym_blocks(v), v.obs.copy(), v.flags.copy()
    v.fork(0)
    b1 = gym_blocks(v)
    for e in range(n):
        assert np.array_equal(b1[e], b0[0]), e
        assert (v.obs[e] == obs0[0]).all() and v.flags[e] == flags0[0], e
    oras = [pyoracle.OracleGymEnv(seed=seed) for _ in range(n)]
    for o in oras:
        for i in range(RL_CUT):
            assert o.step(pre[i, 0])[1:] == (False, 0)
    assert_gym_equals_oracles(v, oras, "fork")
    streams = fork_streams()
    alive = np.ones(n, dtype=bool)
    ended_in_error = []
    for i in range(streams.shape[0]):
        was = alive.copy()
        _step_all(v, oras, alive, streams[i], "branch step %d" % i)
        s = v.summary()
        ended_in_error += [(int(e), i) for e in np.nonzero(was & ~alive)[0] if s["status"][e] == 2]
        if not alive.any():
            break
    assert not alive.any()
    assert ended_in_error == ([] if err_step is None else [(e, err_step) for e in range(n)])
    assert_gym_equals_oracles(v, oras, "end of the branches")
    assert len(set(v.summary()["hash"].tolist())) == n  # four different episodes from one state


def test_gpu_snapshot_replay(mx):
    """7: the replay handle (IBM 2003-01-14) x4 saved at 40 steps; 20 steps later env 1 alone goes
    back and replays its tape from there while the others step on"""
    from mxabides import tape
    tp = tape.Tape.load(os.path.join(os.path.dirname(__file__), "golden", "tape_IBM_2003-01-14.npz"))
    n, cut, more, cap = 4, 40, 20, 1200
    rs = np.random.RandomState(23)
    acts = np.stack([rs.uniform(0, 0.05, (cap, n)) * np.arange(1, n + 1), rs.uniform(0, 1, (cap, n)),
                     rs.uniform(0, 1, (cap, n))], 2)
    v = VecABIDESEnv(tp, n)
    v.set_parity_hash(True)
    oras = [pyoracle.OracleGymEnv(tp) for _ in range(n)]
    alive = np.ones(n, dtype=bool)
    for i in range(cut):
        _step_all(v, oras, alive, acts[i], "step %d" % i)
    snap = v.snapshot()
    snap.save()
    saved = gym_blocks(v)
    oc0 = v.summary()["order_counter"].copy()
    for i in range(cut, cut + more):
        _step_all(v, oras, alive, acts[i], "step %d" % i)
    assert alive.all()
    b1 = gym_blocks(v)
    snap.restore({1: 1})
    b2 = gym_blocks(v)
    assert_blocks_equal(b1, b2, [0, 2, 3], "restore, envs left out")
    assert_blocks_equal(saved, b2, [1], "restore")
    assert v.summary()["order_counter"][1] == oc0[1]
    oras[1] = pyoracle.OracleGymEnv(tp)  # env 1's oracle: the 40-step prefix again
    for i in range(cut):
        oras[1].step(acts[i, 1])
    steps = cut + more
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


def test_gpu_snapshot_refusals(mx):
    """8: every refusal is MXA_EINVAL with a message and leaves every block as it was"""
    EINVAL = -1
    m = mx.VecMarket("rmsc03", SEEDS[:4], book_log=1 << 16)
    other = mx.VecMarket("rmsc03", SEEDS[:4], book_log=1 << 16)
    m.set_parity_hash(True)
    m.run(chunk=2000, max_launches=1)
    L, h = m.L, m._h
    snap, small, theirs = m.snapshot(), m.snapshot(2), other.snapshot()
    snap.save([0, 1, -1, -1])
    assert snap.filled == 2
    before = blocks(m)
    i32 = lambda x: np.asarray(x, dtype=np.int32)

    def refused(rc, what):
        assert rc == EINVAL, (what, rc)
        msg = L.mxa_last_error(h).decode()
        assert msg and what in msg, (what, msg)
        assert_blocks_equal(before, blocks(m), range(4), what)

    out = ctypes.c_void_p()
    # null arguments, n_slots <= 0
    refused(L.mxa_snapshot_create(h, 4, None), "mxa_snapshot_create")
    refused(L.mxa_snapshot_create(h, 0, ctypes.byref(out)), "mxa_snapshot_create")
    refused(L.mxa_snapshot_create(h, -3, ctypes.byref(out)), "mxa_snapshot_create")
    assert not out
    refused(L.mxa_snapshot_save(h, None, None), "null")
    refused(L.mxa_snapshot_restore(h, None, None), "null")
    assert L.mxa_snapshot_save(None, snap._s, None) == EINVAL and L.mxa_snapshot_restore(None, snap._s, None) == EINVAL
    assert L.mxa_snapshot_create(None, 4, ctypes.byref(out)) == EINVAL
    o4 = np.zeros(4, dtype=np.int64)
    assert L.mxa_snapshot_info(None, o4.ctypes.data) == EINVAL and L.mxa_snapshot_info(snap._s, None) == EINVAL
    L.mxa_snapshot_destroy(None)
    # map entries outside -1 .. n_slots - 1
    for bad in ([0, 1, -2, -1], [0, 1, 4, -1]):
        refused(L.mxa_snapshot_save(h, snap._s, i32(bad).ctypes.data), "outside")
        refused(L.mxa_snapshot_restore(h, snap._s, i32(bad).ctypes.data), "outside")
    refused(L.mxa_snapshot_save(h, small._s, i32([0, 1, 2, -1]).ctypes.data), "outside")
    # the identity map with too few slots
    refused(L.mxa_snapshot_save(h, small._s, None), "n_slots >= n_envs")
    refused(L.mxa_snapshot_restore(h, small._s, None), "n_slots >= n_envs")
    # two envs saving to one slot
    refused(L.mxa_snapshot_save(h, snap._s, i32([2, -1, 2, -1]).ctypes.data), "two envs")
    # a slot never saved: slot 2 by name, slots 2 and 3 through the identity map, slot 0 of an empty bank
    refused(L.mxa_snapshot_restore(h, snap._s, i32([0, 0, 2, 1]).ctypes.data), "never saved")
    refused(L.mxa_snapshot_restore(h, snap._s, None), "never saved")
    refused(L.mxa_snapshot_restore(h, small._s, i32([0, -1, -1, -1]).ctypes.data), "never saved")
    # another handle's snapshot
    theirs.save()
    refused(L.mxa_snapshot_save(h, theirs._s, None), "another handle")
    refused(L.mxa_snapshot_restore(h, theirs._s, None), "another handle")
    assert (snap.filled, small.filled) == (2, 0)  # no refused save filled a slot
    # through the Python surface
    for call, arg in ((snap.save, [0, 1]), (snap.restore, {4: 0}), (snap.restore, {0: 3}), (small.save, None)):
        with pytest.raises((ValueError, mx.MxaError)):
            call(arg)
    assert_blocks_equal(before, blocks(m), range(4), "python")
    # the exchange-log switch differs from the one at create (other has not launched: the switch is free)
    other.set_exchange_log(True)
    with pytest.raises(mx.MxaError, match="exchange-log"):
        theirs.restore()
    other.set_exchange_log(False)
    theirs.restore()
    # the log reallocated (mxa_set_book_log): at another capacity, and switched off
    for cap in (8192, 0):
        other.set_book_log(cap)
        for call in (theirs.save, theirs.restore):
            with pytest.raises(mx.MxaError, match="mxa_set_book_log"):
                call()
    # what is accepted still works after all of it
    snap.restore([0, 0, 1, -1])
    b = blocks(m)
    assert np.array_equal(b[0], before[0]) and np.array_equal(b[1], before[0]) and np.array_equal(b[2], before[1])
    assert np.array_equal(b[3], before[3])
