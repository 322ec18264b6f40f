"""The stream classes on the device (csrc/mxa_config.h stream_class_of; DESIGN.md §4 "RNG streams";
include/mxa_streams.h): what the build kernel leaves in every agent's stream area after reset(),
read through mxa_read_raw at mxa_layout.h's offsets with no run, and the head streams' probe.

  full  block 0 is numpy's seeded state and block 1 its next twist, all 624 words of each
  head  block 1's first 64 words are numpy's first 64 outputs (tempered on the host)
  none  nothing past the seed word

Whatever is not written stays as mxa_create zeroed it, so a handle reset over other seeds ends
byte-identical to a fresh one (test_gpu_reset_is_a_function_of_the_seeds).

The guard.  A draw that leaves a head sets bit 1 of the stream's flag word (rs_head_guard), the bit
rng_maint reports as ERR_RNG_OVERRUN at its one fail() site; the probe shows the bit at the first
draw that consumes word `head_words` and never before.  No seed reaches it in a market:
randint(0, 100) rejects 28 of 128 masked words, so 64 rejections in a row have probability about
1e-42, and tests/env_error_cases.py says so for code 9.  Nothing here tries to provoke it."""

import numpy as np
import pytest

from golden_util import COMPOSITION_FIXTURES, load_composition

pytestmark = pytest.mark.gpu

MT_N, MT_M, RNG_BYTES, HEAD = 624, 397, 5120, 64
AG_EXCHANGE, AG_ZI, AG_NOISE, AG_VALUE, AG_POVMM, AG_MOMENTUM = 0, 1, 2, 3, 4, 5
HDR_LAUNCH_LOCAL = [(248, 280), (368 + 4 * 25, 368 + 4 * 28)]  # as tests/test_gpu_limit_inplace.py raw_state


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def temper(y):
    y = y.astype(np.uint32).copy()
    y ^= y >> 11
    y ^= (y << 7) & np.uint32(0x9d2c5680)
    y ^= (y << 15) & np.uint32(0xefc60000)
    y ^= y >> 18
    return y


def numpy_words(seed, n):
    """the first n raw 32-bit outputs of numpy.random.RandomState(seed)"""
    return np.frombuffer(np.random.RandomState(int(seed)).bytes(4 * n), dtype="<u4")


def numpy_blocks(seed):
    """(block 0: the seeded state, block 1: its next twist) of numpy.random.RandomState(seed)"""
    rs = np.random.RandomState(int(seed))
    b0 = rs.get_state()[1].copy()
    rs.bytes(4)
    st = rs.get_state()
    assert st[2] == 1
    return b0, st[1].copy()


def raw(h, env, offset, nbytes):
    """mxa_read_raw of any handle (a VecMarket's or a VecABIDESEnv's)"""
    buf = np.zeros(nbytes, dtype=np.uint8)
    h._check(h.L.mxa_read_raw(h._h, env, offset, nbytes, buf.ctypes.data), "mxa_read_raw")
    return buf


def stream(h, env, agent):
    """the 1280 words of agent's stream area"""
    o = np.zeros(8, dtype=np.int64)
    h._check(h.L.mxa_layout(h._h, o.ctypes.data), "mxa_layout")
    return raw(h, env, int(o[2]) + (4 + agent) * RNG_BYTES, RNG_BYTES).view(np.uint32)


def types(h, env):
    return [int(a.type) for a in h._agent_states(env)]


def reset_market(mx, config, seeds):
    if config == "rmsc03_rl":
        from mxabides.gym import VecABIDESEnv
        m = VecABIDESEnv(seeds=seeds)
    else:
        m = mx.VecMarket(config, seeds)
    m.reset()
    m._check(m.L.mxa_sync(m._h), "mxa_sync")
    return m


def check_heads(m, env):
    """every noise and momentum agent's head against numpy; how many were checked"""
    n = 0
    for a, t in enumerate(types(m, env)):
        if t not in (AG_NOISE, AG_MOMENTUM):
            continue
        w = stream(m, env, a)
        got, want = temper(w[MT_N:MT_N + HEAD]), numpy_words(w[0], HEAD)
        assert np.array_equal(got, want), (env, a, int(w[0]))
        n += 1
    return n


@pytest.mark.parametrize("config,n_envs,n_head", [("rmsc03", 2, 52), ("value_noise", 2, 100), ("rmsc03_rl", 2, 52),
                                                  ("cfg.rmsc03_n100_v20", 2, 102), ("random_fund_value", 1, 5000)])
def test_gpu_head_streams_are_numpys_first_outputs(mx, config, n_envs, n_head):
    if config.startswith("cfg."):
        from mxabides import composition as C
        name = config[4:]
        seed = next(s for n, s in COMPOSITION_FIXTURES if n == name)
        config = C.from_dict(load_composition(name, seed)[0]["composition"])
    m = reset_market(mx, config, [123456789, 7][:n_envs])
    for e in range(n_envs):
        assert check_heads(m, e) == n_head, e


def test_gpu_full_streams_are_numpys_state_and_next_twist(mx):
    """the parent's behaviour, pinned: rmsc03's value agents (51-60), sparse_zi_100's first and last ZI agent"""
    for config, agents, typ in (("rmsc03", range(51, 61), AG_VALUE), ("sparse_zi_100", (1, 100), AG_ZI)):
        m = reset_market(mx, config, [123456789, 7])
        assert m.n_agents == (64 if config == "rmsc03" else 101)
        for e in range(2):
            ag = types(m, e)
            for a in agents:
                assert ag[a] == typ, (config, a)
                w = stream(m, e, a)
                b0, b1 = numpy_blocks(w[0])
                assert np.array_equal(w[:MT_N], b0), (config, e, a)
                assert np.array_equal(w[MT_N:2 * MT_N], b1), (config, e, a)


def test_gpu_none_streams_hold_the_seed_alone(mx):
    m = reset_market(mx, "rmsc03", [123456789, 7])
    for e in range(2):
        ag = types(m, e)
        assert ag[0] == AG_EXCHANGE and ag[61] == AG_POVMM
        for a in (0, 61):
            w = stream(m, e, a)
            assert w[0] != 0 and not w[1:].any(), (e, a, np.nonzero(w[1:])[0][:8].tolist())


def raw_state(m):
    out = []
    for i in range(m.n_envs):
        b = m.raw(i, 0, m.env_bytes).copy()
        for lo, hi in HDR_LAUNCH_LOCAL:
            b[lo:hi] = 0
        out.append(b)
    return out


def records(m):
    s = m.summary()
    assert (s["status"] == 1).all(), s["err"]
    return [(int(s["events"][i]), int(s["hash"][i]), int(s["order_counter"][i]), int(s["last_trade"][i]),
             [(a["cash"], a["shares"], a["n_open"]) for a in m.agents(i)[1:]]) for i in range(m.n_envs)]


@pytest.mark.parametrize("config,n_envs", [("rmsc03", 4), ("value_noise", 2)])
def test_gpu_reset_is_a_function_of_the_seeds(mx, config, n_envs):
    """a handle reset three times over other seeds and then over S is a fresh handle built with S, byte
    for byte (the unwritten words of head and none streams are zero on both), and runs to the same end"""
    S = np.array([123456789, 1008, 7, 11][:n_envs], dtype=np.int64)
    old = mx.VecMarket(config, S + 1000)
    old.set_parity_hash(True)
    for k in (1, 2, 3):
        old.set_seeds((S * (k + 1) + 17 * k) & 0xFFFFFFFF)
        old.reset()
    old.set_seeds(S)
    old.reset()
    old.sync()
    new = mx.VecMarket(config, S)
    new.set_parity_hash(True)
    new.reset()
    new.sync()
    for e, (x, y) in enumerate(zip(raw_state(old), raw_state(new))):
        assert np.array_equal(x, y), (e, np.nonzero(x != y)[0][:16].tolist())
    old.run()
    new.run()
    assert records(old) == records(new)


# ---- the probe


def probe(mx, seed, hw, n):
    L = mx.load()
    out, state = np.zeros(n), np.zeros((n, 2), dtype=np.uint64)
    assert L.mxa_stream_head_probe(0, seed, hw, n, out.ctypes.data, state.ctypes.data) == 0
    return out.astype(np.int64), state[:, 0].astype(np.int64), state[:, 1].astype(np.int64)


def rejected(seed, n):
    """which of numpy's first n words randint(0, 100) rejects"""
    return (numpy_words(seed, n) & 127) > 99


def seed_where(hw, pattern):
    """the smallest seed whose words hw - len(pattern) .. hw - 1 are rejected as `pattern` says"""
    for seed in range(1, 100000):
        r = rejected(seed, hw)
        if list(r[hw - len(pattern):]) == list(pattern):
            return seed
    raise AssertionError("no seed")


@pytest.mark.parametrize("hw", [2, 3, 63, 64])
@pytest.mark.parametrize("case", ["plain", "boundary", "inside"])
def test_gpu_probe_draws_and_flags_as_numpy_to_the_heads_end(mx, hw, case):
    """plain: seed 123456789; boundary: word hw - 2 is accepted and word hw - 1 rejected, so that draw goes on to word hw;
    inside: word hw - 2 is rejected and word hw - 1 accepted, so that draw ends with exactly hw words"""
    seed = {"plain": 123456789, "boundary": seed_where(hw, [False, True]), "inside": seed_where(hw, [True, False])}[case]
    n = hw + 2
    val, pos, flag = probe(mx, seed, hw, n)
    rs = np.random.RandomState(seed)
    first_over = None
    for i in range(n):
        v = int(rs.randint(0, 100))
        p = MT_N + int(rs.get_state()[2])  # numpy's position inside block 1 after the draw
        if p <= MT_N + hw:  # every word of the draw inside the head
            assert first_over is None
            assert (int(val[i]), int(pos[i])) == (v, p), (i, seed)
            assert flag[i] & 2 == 0, (i, seed)
        else:
            first_over = i if first_over is None else first_over
            assert flag[i] & 2, (i, seed)  # set at the first draw that touches word hw, and it stays
    assert first_over is not None
    if case != "plain":
        assert first_over >= 1 and flag[first_over - 1] & 2 == 0
    if case == "inside":
        assert pos[first_over - 1] == MT_N + hw  # exactly head_words words consumed: clear
    if case == "boundary":
        assert pos[first_over - 1] < MT_N + hw and rejected(seed, hw)[hw - 1]


def test_gpu_probe_refuses_bad_arguments(mx):
    L = mx.load()
    out, state = np.zeros(4), np.zeros((4, 2), dtype=np.uint64)
    o, s = out.ctypes.data, state.ctypes.data
    for args in ((0, 1, 64, 4, None, s), (0, 1, 64, 4, o, None), (0, 1, 64, 0, o, s), (0, 1, 64, -1, o, s),
                 (0, 1, 1, 4, o, s), (0, 1, 0, 4, o, s), (0, 1, -3, 4, o, s), (0, 1, 65, 4, o, s)):
        assert L.mxa_stream_head_probe(*args) == -1, args
    assert not out.any() and not state.any()
    assert L.mxa_stream_head_probe(0, 1, 64, 4, o, s) == 0 and L.mxa_stream_head_probe(0, 1, 2, 4, o, s) == 0
