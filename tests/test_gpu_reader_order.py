"""The readers' ordering contract (include/mxa.h): every mxa_read_* is ordered after all work submitted
to the handle's stream before it, on the handle's own (non-blocking) stream and on a caller's, so a
read straight after an asynchronous launch or step returns what a read after mxa_sync returns.

Two handles of the same seeds advance in lockstep.  A is synchronised before it is read; B is read
with its launch still queued or running.  Each round starts B's reads with another reader (the first
read after the launch is the one that can overtake it), then compares every reader of every env.
Every comparison is exact and none depends on how long anything takes."""
import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process

from mxabides.gym import ACTION_SIZE, OBS_SIZE, VecABIDESEnv
from test_gpu_partial_reset import NS, OPEN, SEEDS

pytestmark = pytest.mark.gpu

POPS = 4096
TRACE_ROWS = 64
BOOK_LOG = 1 << 14  # records per env: small (a log that overflows does so on both handles alike)
LEVELS, N_BARS = 4, 4


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def rmsc03_pair(mx, caller_stream, book_log=0):
    """(A, B, B's stream): both created and reset before either launches"""
    a, b = (mx.VecMarket("rmsc03", SEEDS, trace_cap=TRACE_ROWS) for _ in range(2))
    stream = torch.cuda.Stream() if caller_stream else None
    if stream is not None:
        b.set_stream(stream.cuda_stream)
    for m in (a, b):
        m.set_parity_hash(True)
        if book_log:
            m.set_book_log(book_log)
    return a, b, stream


def advance(a, b):
    """A to its synced state, and only then B's launch: B's reads follow with nothing in between"""
    a.launch(POPS)
    a.sync()
    b.launch(POPS)


def assert_same(what, x, y):
    if isinstance(x, dict):
        assert x.keys() == y.keys(), what
        for k in x:
            assert np.array_equal(x[k], y[k]), (what, k, x[k], y[k])
    elif isinstance(x, np.ndarray):
        assert x.shape == y.shape and np.array_equal(x, y), (what, np.argwhere(x != y)[:8].tolist())
    else:
        assert x == y, what


@pytest.mark.parametrize("caller_stream", [False, True], ids=["own_stream", "callers_stream"])
def test_gpu_readers_follow_an_async_launch(mx, caller_stream):
    a, b, stream = rmsc03_pair(mx, caller_stream)
    readers = [("book 0", lambda m, e: m.book(e, 0)), ("book 1", lambda m, e: m.book(e, 1)),
               ("agents", lambda m, e: m.agents(e)), ("trace", lambda m, e: m.trace(e))]
    firsts = readers + [("summary", None)]
    for r, (first, read_first) in enumerate(firsts):
        advance(a, b)
        # B's first read after the launch: another reader each round
        got_first = b.summary() if read_first is None else read_first(b, 0)
        assert_same("round %d, %s first" % (r, first), got_first, a.summary() if read_first is None else read_first(a, 0))
        for e in range(b.n_envs):
            for name, read in readers:
                assert_same("round %d, env %d, %s" % (r, e, name), read(b, e), read(a, e))
        sa, sb = a.summary(), b.summary()
        assert_same("round %d, summary" % r, sb, sa)
        assert (sa["status"] != 2).all() and (sa["events"] > 0).all(), sa
        assert all(len(a.trace(e)) > 0 for e in range(a.n_envs))


@pytest.mark.parametrize("caller_stream", [False, True], ids=["own_stream", "callers_stream"])
def test_gpu_depth_and_bars_follow_an_async_launch(mx, caller_stream):
    a, b, stream = rmsc03_pair(mx, caller_stream, book_log=BOOK_LOG)
    depth = lambda m: m.depth(levels=LEVELS)
    bars = lambda m: m.bars(OPEN, NS, N_BARS)
    for r, first in enumerate((depth, bars)):
        advance(a, b)
        for k, (x, y) in enumerate(zip(first(b), first(a))):
            assert_same("round %d, first read, array %d" % (r, k), x, y)
        for name, read in (("depth", depth), ("bars", bars)):
            for k, (x, y) in enumerate(zip(read(b), read(a))):
                assert_same("round %d, %s, array %d" % (r, name, k), x, y)
        assert_same("round %d, summary" % r, b.summary(), a.summary())
    assert (a.summary()["events"] > 0).all()


def test_gpu_readers_follow_an_async_step():
    seeds = SEEDS[:2]
    a, b = VecABIDESEnv(seeds=seeds), VecABIDESEnv(seeds=seeds)
    n = a.n_envs
    rs = np.random.RandomState(29)
    acts = rs.uniform(0, 1, (4, n, ACTION_SIZE))
    acts[..., 0] *= 0.02
    d_act = torch.tensor(acts, dtype=torch.float64, device="cuda")
    d_obs = torch.zeros((2, n, OBS_SIZE), dtype=torch.float64, device="cuda")
    d_flags = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the tensors are ready before the handles' streams touch them

    def two_steps(v, which, i0):
        for i in (i0, i0 + 1):
            v.step_device(d_act[i].data_ptr(), d_obs[which].data_ptr(), d_flags[which].data_ptr())

    book = lambda v: [v.book(e, s) for e in range(n) for s in (0, 1)]
    agents = lambda v: [v.agents(e) for e in range(n)]
    for r, first in enumerate((book, agents)):
        two_steps(a, 0, 2 * r)
        a._check(a.L.mxa_sync(a._h), "mxa_sync")
        two_steps(b, 1, 2 * r)
        assert_same("round %d, first read" % r, first(b), first(a))
        assert_same("round %d, book" % r, book(b), book(a))
        assert_same("round %d, agents" % r, agents(b), agents(a))
        assert_same("round %d, summary" % r, b.summary(), a.summary())
    s = a.summary()
    assert (s["status"] != 2).all() and (s["events"] > 0).all(), s
