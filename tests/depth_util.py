"""Helpers of the book-depth tests (include/mxa_depth.h): the reference rows of a side as the host
readers return it, and the check of one mxa_write_depth call against them."""
import numpy as np

GUARD = 0x5A5A5A5A5A5A5A5A  # what the rows around the buffer hold
GARBAGE = -0x0123456789ABCDEF  # what the buffer holds before the call


def depth_ref(levels_list, k):
    """a side as Handle.book() / OracleEnv.book() return it (levels best-first, each a list of
    [oid, agent, qty, price]) -> ([k][2] int64 rows of (price, total quantity), zero past the count;
    the count = min(k, levels))"""
    rows = np.zeros((k, 2), dtype=np.int64)
    n = min(k, len(levels_list))
    for i in range(n):
        lvl = levels_list[i]
        assert lvl and all(o[3] == lvl[0][3] for o in lvl), "one price per level"
        rows[i] = (int(lvl[0][3]), sum(int(o[2]) for o in lvl))
    return rows, n


def refs_of(books, k):
    """[(bids, asks)] per env -> (rows [n][2][k][2] int64, counts [n][2] int32)"""
    rows = np.zeros((len(books), 2, k, 2), dtype=np.int64)
    counts = np.zeros((len(books), 2), dtype=np.int32)
    for e, sides in enumerate(books):
        for s in (0, 1):
            rows[e, s], counts[e, s] = depth_ref(sides[s], k)
    return rows, counts


def handle_books(h, envs=None):
    """[(bids, asks)] of every env through the handle's own host reader"""
    return [(h.book(e, 0), h.book(e, 1)) for e in (range(h.n_envs) if envs is None else envs)]


def device_depth(h, k, counts=True):
    """one write_depth into a torch buffer with a guard block of rows before and after and garbage
    inside: (rows [n][2][k][2], counts [n][2] or None) once the guards are seen intact"""
    import torch
    n = h.n_envs
    rows_n = n * 2 * k
    pad = 2 * k + 3  # rows of guard on either side
    buf = torch.full(((rows_n + 2 * pad) * 2,), GUARD, dtype=torch.int64, device="cuda")
    buf[2 * pad:2 * (pad + rows_n)] = GARBAGE
    cnt = torch.full((2 * n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt[8:8 + 2 * n] = -7
    torch.cuda.synchronize()
    h.write_depth(k, buf.data_ptr() + 16 * pad, cnt.data_ptr() + 32 if counts else 0)
    h._check(h.L.mxa_sync(h._h), "mxa_sync")
    torch.cuda.synchronize()
    b, c = buf.cpu().numpy(), cnt.cpu().numpy()
    assert (b[:2 * pad] == GUARD).all() and (b[2 * (pad + rows_n):] == GUARD).all(), "a write outside the depth array"
    assert (c[:8] == 0x5A5A5A5A).all() and (c[8 + 2 * n:] == 0x5A5A5A5A).all(), "a write outside the counts array"
    if not counts:
        assert (c[8:8 + 2 * n] == -7).all(), "counts written though the pointer was NULL"
    return b[2 * pad:2 * (pad + rows_n)].reshape(n, 2, k, 2), (c[8:8 + 2 * n].reshape(n, 2) if counts else None)


def check_depth(handle, k, refs, envs=None):
    """mxa_write_depth(k) of `handle` against refs = (rows, counts) as refs_of gives them (for `envs`,
    default all): rows and counts equal, the rows past the count zero (written by the kernel: the
    buffer held garbage), nothing written outside, and depth(k) / inside(env, k) agree with the
    device buffer.  Returns the device rows and counts."""
    rows, counts = device_depth(handle, k)
    envs = list(range(handle.n_envs)) if envs is None else list(envs)
    ref_rows, ref_counts = refs
    assert len(ref_rows) == len(envs)
    for i, e in enumerate(envs):
        for s in (0, 1):
            c = int(counts[e, s])
            assert c == int(ref_counts[i, s]), ("count", e, s, c, int(ref_counts[i, s]))
            assert (rows[e, s, c:] == 0).all(), ("rows past the count", e, s)
            assert np.array_equal(rows[e, s], ref_rows[i, s]), ("rows", e, s, rows[e, s, :c + 1].tolist(),
                                                                ref_rows[i, s, :c + 1].tolist())
    h_rows, h_counts = handle.depth(k)
    assert h_rows.dtype == np.int64 and h_rows.shape == (handle.n_envs, 2, k, 2)
    assert h_counts.dtype == np.int32 and h_counts.shape == (handle.n_envs, 2)
    assert np.array_equal(h_rows, rows) and np.array_equal(h_counts, counts)
    for e in envs[:2] + envs[-1:]:
        bids, asks = handle.inside(e, k)
        assert bids == [tuple(r) for r in rows[e, 0, :counts[e, 0]].tolist()]
        assert asks == [tuple(r) for r in rows[e, 1, :counts[e, 1]].tolist()]
    return rows, counts
