"""Handle: what every libmxa handle (include/mxa.h mxa_handle) offers whichever constructor made
it: the error check, the switches, the device-side writers and the readers.  VecMarket
(mxabides.market, Kernel.runner handles) and VecABIDESEnv (mxabides.gym, GymKernel handles) derive
from it; a subclass creates the handle into `self._h` and sets n_envs, n_agents and trace_cap."""
import ctypes

import numpy as np

from . import _lib


def seeds_u32(seeds):
    """per-env seeds as the C-ABI takes them: the reference's -s values modulo 2^32"""
    return np.ascontiguousarray(np.asarray(seeds, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)


class Handle:
    def __init__(self):
        self.L = _lib.load()
        self._h = ctypes.c_void_p()

    def _check(self, rc, what):
        if rc < 0:
            msg = self.L.mxa_last_error(self._h).decode() if self._h else ""
            raise _lib.MxaError("%s failed (%d): %s" % (what, rc, msg))
        return rc

    # ---- switches
    def set_parity_hash(self, on):
        """Per-pop parity hash (summary()["hash"]) on or off; market results are identical
        either way (include/mxa.h mxa_set_parity_hash)."""
        self._check(self.L.mxa_set_parity_hash(self._h, 1 if on else 0), "mxa_set_parity_hash")

    def set_stream(self, stream_ptr):
        """Run on an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream)."""
        self._check(self.L.mxa_set_stream(self._h, ctypes.c_void_p(stream_ptr) if stream_ptr else None),
                    "mxa_set_stream")

    # ---- device-side writers (asynchronous on the handle's stream)
    def write_results(self, device_ptr):
        """Per-env (events, hash, status, current_time) int64 rows into device memory."""
        self._check(self.L.mxa_write_results(self._h, ctypes.c_void_p(device_ptr)), "mxa_write_results")

    def write_records(self, device_ptr):
        """Per-env episode records [n][RECORD_WORDS] int64 into device memory (include/mxa.h
        mxa_write_records: events, hash, status, current_time, err, seed, last_trade, order_counter,
        cash, holdings, gain, 0), the rows bench.py all-gathers across ranks."""
        self._check(self.L.mxa_write_records(self._h, ctypes.c_void_p(device_ptr)), "mxa_write_records")

    def write_depth(self, levels, depth_ptr, counts_ptr=0):
        """Every env's top `levels` price levels into device memory, one kernel launch on the handle's
        stream (include/mxa_depth.h mxa_write_depth): depth_ptr -> [n_envs][2][levels][2] int64, side 0
        bids / 1 asks, row i = (price, total shares) of the i-th best level, (0, 0) from the count on;
        counts_ptr -> [n_envs][2] int32 or 0 for none.  Returns without synchronising."""
        self._check(self.L.mxa_write_depth(self._h, int(levels), ctypes.c_void_p(depth_ptr) if depth_ptr else None,
                                           ctypes.c_void_p(counts_ptr) if counts_ptr else None), "mxa_write_depth")

    # ---- readers
    def counters(self):
        """[n_envs][COUNTER_WORDS] int64 event-class counters since the last reset (kept by
        instrumented runs: parity hash on; include/mxa.h mxa_read_counters, mxabides.counters)"""
        out = np.zeros((self.n_envs, _lib.COUNTER_WORDS), dtype=np.int64)
        self._check(self.L.mxa_read_counters(self._h, out.ctypes.data), "mxa_read_counters")
        return out

    def inplace_groups(self):
        """[market-maker query groups, value-agent wakes, cancel / ladder groups, 0, value agents'
        resting orders with their acknowledgement (inside such a wake), 0] taken in place by
        the instrumented runs (parity hash on) of this configuration's handles since the last call
        (include/mxa.h mxa_read_inplace: read, then cleared).  The env blocks cannot tell: an in-place
        group leaves every observable of the queued sequence.  Words 6-8 and 9-11: the draws those
        runs took from the variate tables of the oracle stream and of the value agents' streams, as
        (hits, fills, serial fall-backs)"""
        out = np.zeros(_lib.INPLACE_WORDS, dtype=np.uint64)
        self._check(self.L.mxa_read_inplace(self._h, out.ctypes.data), "mxa_read_inplace")
        return out

    @property
    def last_kernel_ms(self):
        return self.L.mxa_last_kernel_ms(self._h)

    @property
    def resident_envs(self):
        """envs resident on the device at once (run / step kernel occupancy x CUs, at most n_envs;
        include/mxa.h mxa_resident_envs)"""
        return self._check(self.L.mxa_resident_envs(self._h), "mxa_resident_envs")

    def summary(self):
        """every mxa_env_summary field as an [n_envs] array"""
        arr = (_lib.EnvSummary * self.n_envs)()
        self._check(self.L.mxa_read_summary(self._h, arr), "mxa_read_summary")
        dt = {ctypes.c_int32: np.int32, ctypes.c_int64: np.int64, ctypes.c_uint64: np.uint64}
        return {k: np.array([getattr(a, k) for a in arr], dtype=dt[t]) for k, t in _lib.EnvSummary._fields_}

    def _agent_states(self, env):
        arr = (_lib.AgentState * self.n_agents)()
        self._check(self.L.mxa_read_agents(self._h, env, arr, self.n_agents), "mxa_read_agents")
        return arr

    def book(self, env, side):
        """OrderBook.bids (side 0) / asks (side 1): list of levels best-first, each a FIFO list of
        [order_id, agent_id, quantity, price]."""
        cap = 4096
        while True:  # mxa_read_book returns the side's order count; a replay book holds thousands
            buf = np.zeros((cap, 4), dtype=np.int64)
            n = self._check(self.L.mxa_read_book(self._h, env, side, buf.ctypes.data, cap), "mxa_read_book")
            if n <= cap:
                break
            cap = n
        levels = []
        for o in buf[:n].tolist():
            if levels and levels[-1][0][3] == o[3]:
                levels[-1].append(o)
            else:
                levels.append([o])
        return levels

    def depth(self, levels=10):
        """(np.int64 [n_envs, 2, levels, 2], np.int32 [n_envs, 2]): write_depth's rows and counts on the
        host (include/mxa_depth.h mxa_read_depth; synchronises the handle's stream)"""
        rows = np.empty((self.n_envs, 2, int(levels), 2), dtype=np.int64) if 1 <= int(levels) <= 1 << 20 else None
        counts = np.empty((self.n_envs, 2), dtype=np.int32)
        self._check(self.L.mxa_read_depth(self._h, int(levels), rows.ctypes.data if rows is not None else None,
                                          counts.ctypes.data), "mxa_read_depth")
        return rows, counts

    def inside(self, env, levels):
        """(OrderBook.getInsideBids(levels), OrderBook.getInsideAsks(levels)) of one env as the reference
        returns them (OrderBook.py:377-398): lists of (price, quantity) tuples, best level first, as many
        as the side has levels up to `levels`"""
        if not 0 <= int(env) < self.n_envs:
            raise IndexError("env %r outside 0 .. %d" % (env, self.n_envs - 1))
        rows, counts = self.depth(levels)
        return tuple([tuple(r) for r in rows[env, s, :counts[env, s]].tolist()] for s in (0, 1))

    def trace(self, env):
        """env's trace ring rows [n][10] int64 (none without a trace ring)"""
        buf = np.zeros((self.trace_cap, 10), dtype=np.int64)
        n = ctypes.c_int64()
        self._check(self.L.mxa_read_trace(self._h, env, buf.ctypes.data, self.trace_cap, ctypes.byref(n)),
                    "mxa_read_trace")
        return buf[:n.value]

    def snapshot(self, n_slots=None):
        """A Snapshot of n_slots slots (default: one per env) on this handle's device, to save envs
        into and restore or fork them from, mid-episode (include/mxa_snap.h)."""
        return Snapshot(self, self.n_envs if n_slots is None else n_slots)

    def close(self):
        if self._h:
            self.L.mxa_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Snapshot:
    """n_slots slots of device memory, each holding one env of `handle` whole: its block, its seed
    word and its book-update log rows (include/mxa_snap.h).  save() and restore() are one
    kernel launch each.  `slots` says which env goes with which slot: None (env e <-> slot e), a full
    [n_envs] map with -1 for the envs that take no part, or a dict {env: slot}.  On restore many envs
    may name one slot (a fork); on save each slot takes one env.  On a GymKernel handle a slot also
    keeps its env's host `obs` / `flags` rows, and restore() puts them back for the restored envs,
    as reset(mask=...) clears exactly the masked rows."""

    def __init__(self, handle, n_slots):
        self.handle = handle
        self.L = handle.L
        self._s = ctypes.c_void_p()
        handle._check(self.L.mxa_snapshot_create(handle._h, int(n_slots), ctypes.byref(self._s)), "mxa_snapshot_create")
        self._rows = {}  # slot -> (obs row, flags word) of a GymKernel handle

    def _info(self):
        o = np.zeros(4, dtype=np.int64)
        if self.L.mxa_snapshot_info(self._s, o.ctypes.data) < 0:
            raise _lib.MxaError("mxa_snapshot_info failed: the snapshot is closed")
        return o

    n_slots = property(lambda self: int(self._info()[0]))
    slot_bytes = property(lambda self: int(self._info()[1]))
    filled = property(lambda self: int(self._info()[2]))
    has_log = property(lambda self: bool(self._info()[3]))

    def _map(self, slots):
        """(the C-ABI's slot_of_env or None, [(env, slot)] of the envs taking part)"""
        n = self.handle.n_envs
        if slots is None:
            return None, [(e, e) for e in range(n)]
        if isinstance(slots, dict):
            m = np.full(n, -1, dtype=np.int32)
            for e, s in slots.items():
                if not 0 <= int(e) < n:
                    raise ValueError("slots: env %r outside 0 .. %d" % (e, n - 1))
                m[int(e)] = int(s)
        else:
            m = np.ascontiguousarray(np.asarray(slots, dtype=np.int64).reshape(-1), dtype=np.int32)
            if len(m) != n:
                raise ValueError("slots: one entry per env (-1: the env takes no part)")
        return m, [(e, int(s)) for e, s in enumerate(m) if s >= 0]

    def save(self, slots=None):
        h = self.handle
        m, pairs = self._map(slots)
        h._check(self.L.mxa_snapshot_save(h._h, self._s, m.ctypes.data if m is not None else None), "mxa_snapshot_save")
        if hasattr(h, "obs"):
            for e, s in pairs:
                self._rows[s] = (h.obs[e].copy(), h.flags[e].copy())

    def restore(self, slots=None):
        h = self.handle
        m, pairs = self._map(slots)
        h._check(self.L.mxa_snapshot_restore(h._h, self._s, m.ctypes.data if m is not None else None),
                 "mxa_snapshot_restore")
        h._finalized = False  # mxa_finalize's results are no part of a snapshot
        if hasattr(h, "obs"):
            for e, s in pairs:
                h.obs[e], h.flags[e] = self._rows[s]

    def close(self):
        if self._s:
            self.L.mxa_snapshot_destroy(self._s)
            self._s = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
