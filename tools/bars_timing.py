#!/usr/bin/env python3
"""Time of mxa_write_bars (include/mxa_bars.h) beside the host replay it replaces.

    python tools/bars_timing.py [--rounds 9] [--out profiles/bars/timing.json]

Two shapes, one process: rmsc03 x 4096 after the whole episode with 900 one-second bars from 09:30, and
the IBM 2003-01-14 replay runner x 64 after the whole tape with 390 one-minute bars.  The handle runs on
a torch side stream and the call is timed between torch.cuda events on that stream (HIP events); each
figure is the median of `rounds` after one warm-up call.  Beside it:
  (a) the only way to the same series before mxa_write_bars: book_log_records + rows_from_records per
      env, wall time, for 8 envs of the same handle, SCALED to the batch (x n_envs / 8) and marked so;
  (b) the bytes the kernel has to touch divided by the time: the 16-byte records it consumes (status
      word 1 of every env) and the env headers' two count words read, the bars and status words written;
  (c) the counts that bound a serial replay: records consumed and book-changing records (the sum of
      word 11) per env, and the time per record of the longest env."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-optimal-execution_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libmxa loads: one HIP runtime per process)

import mxabides  # noqa: E402
from mxabides import booklog, tape  # noqa: E402

S = 10**9
HOST_ENVS = 8


def time_write(h, stream, t0, dt, n_bars, rounds):
    bars = torch.empty((h.n_envs, n_bars, 12), dtype=torch.int64, device="cuda")
    status = torch.empty((h.n_envs, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for r in range(rounds + 1):  # call 0 warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h.write_bars(t0, dt, n_bars, bars.data_ptr(), status.data_ptr())
        e1.record(stream)
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), bars.cpu().numpy(), status.cpu().numpy()


def host_replay(h):
    t0 = time.perf_counter()
    rows = [booklog.rows_from_records(h.book_log_records(e)) for e in range(HOST_ENVS)]
    return time.perf_counter() - t0, rows


def check(rows, bars, t0, dt, n_bars):
    """the timed call's volume per bar is the host replay's executed quantity per bar"""
    for e, flat in enumerate(rows):
        want = np.zeros(n_bars, dtype=np.int64)
        for t, xq, _, _, _ in booklog.iter_rows(flat):
            if t0 <= t < t0 + n_bars * dt:
                want[(t - t0) // dt] += xq
        assert np.array_equal(bars[e, :, 8], want), e


def case(name, h, stream, t0, dt, n_bars, rounds):
    out = {"shape": name, "n_envs": h.n_envs, "n_bars": n_bars, "dt_ns": dt}
    host_s, rows = host_replay(h)
    out["host_replay_s_8_envs"] = host_s
    out["host_replay_s_scaled_to_batch"] = host_s * h.n_envs / HOST_ENVS
    out["host_replay_is_scaled"] = True
    ms, lo, hi, bars, status = time_write(h, stream, t0, dt, n_bars, rounds)
    check(rows, bars, t0, dt, n_bars)
    assert (status[:, 0] == 0).all(), status[:, 0]
    read = int(status[:, 1].astype(np.int64).sum()) * 16 + 8 * h.n_envs
    written = bars.nbytes + status.nbytes
    book = bars[:, :, 11].sum(axis=1)
    out.update({"ms": ms, "ms_min": lo, "ms_max": hi, "bytes_read": read, "bytes_written": written,
                "GBps": (read + written) / (ms * 1e-3) / 1e9, "host_replay_scaled_over_kernel": out["host_replay_s_scaled_to_batch"] * 1e3 / ms,
                "records_consumed_mean": float(status[:, 1].mean()), "records_consumed_max": int(status[:, 1].max()),
                "book_records_mean": float(book.mean()), "book_records_max": int(book.max()),
                "ns_per_record_of_longest_env": ms * 1e6 / max(1, int(status[:, 1].max())),
                "peak_levels": [int(status[:, 2].max()), int(status[:, 3].max())]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "build_id": mxabides.build_id(), "rounds": a.rounds, "cases": []}
    m = mxabides.VecMarket("rmsc03", list(range(1, 4097)), book_log=1 << 17)
    m.set_parity_hash(False)
    m.set_stream(stream.cuda_stream)
    m.run()
    assert (m.summary()["status"] == 1).all()
    res["cases"].append(case("rmsc03 x4096, whole episode, 900 one-second bars", m, stream, booklog.MKT_OPEN_NS, S, 900, a.rounds))
    m.close()
    tp = tape.Tape.load(os.path.join(ROOT, "tests", "golden", "tape_IBM_2003-01-14.npz"))
    r = mxabides.VecMarket("marketreplay_runner", np.zeros(64, dtype=np.int64), tape=tp, symbol=tp.symbol, book_log=1 << 20)
    r.set_parity_hash(False)
    r.set_stream(stream.cuda_stream)
    r.run()
    assert (r.summary()["status"] == 1).all()
    res["cases"].append(case("IBM 2003-01-14 replay runner x64, whole tape, 390 one-minute bars", r, stream, booklog.MKT_OPEN_NS,
                             60 * S, 390, a.rounds))
    r.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
