#!/usr/bin/env python3
"""Time of mxa_write_depth (include/mxa_depth.h) beside the host loop it replaces.

    python tools/depth_timing.py [--rounds 9] [--out profiles/depth/timing.json]

Two shapes, one process: rmsc03 x 4096 after 15,000 pops (the slot book) and the GymKernel replay of
IBM 2003-01-14 x 512 after 100 steps (the price ladder), each with k = 10 and k = 64.  The handle runs
on a torch side stream and the call is timed between torch.cuda events on that stream (HIP events);
each figure is the median of `rounds` after one warm-up call.  Beside it:
  (a) the only way to the same numbers before mxa_write_depth: Handle.book(env, side) for every env
      and both sides on the same handle, wall time, once;
  (b) the bytes the kernel has to touch divided by the time.  Slot book: the book section of every
      env block (32-byte slots, of which the kernel loads 16) plus the rows and counts written.
      Ladder: per (env, side) the 4-byte level counts of the price span the top k levels cover,
      rounded up to the 256 levels of one round trip, the 8-byte quantity of each row, the header's
      16 bytes, plus the rows and counts written."""
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
from mxabides import tape  # noqa: E402
from mxabides.gym import VecABIDESEnv  # noqa: E402

KS = (10, 64)


def time_write(h, stream, k, rounds):
    n = h.n_envs
    rows = torch.empty((n, 2, k, 2), dtype=torch.int64, device="cuda")
    counts = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for r in range(rounds + 1):  # call 0 warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h.write_depth(k, rows.data_ptr(), counts.data_ptr())
        e1.record(stream)
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), rows.cpu().numpy(), counts.cpu().numpy()


def book_loop(h):
    t0 = time.perf_counter()
    books = [(h.book(e, 0), h.book(e, 1)) for e in range(h.n_envs)]
    return time.perf_counter() - t0, books


def check(books, k, rows, counts):
    """the timed call's output is the host loop's"""
    for e, sides in enumerate(books):
        for s in (0, 1):
            want = [(lv[0][3], sum(o[2] for o in lv)) for lv in sides[s][:k]]
            assert counts[e, s] == len(want) and [tuple(r) for r in rows[e, s, :len(want)].tolist()] == want, (e, s)


def ladder_bytes(rows, counts, k):
    total = 0
    for e in range(len(rows)):
        for s in (0, 1):
            c = int(counts[e, s])
            span = abs(int(rows[e, s, c - 1, 0]) - int(rows[e, s, 0, 0])) + 1 if c else 0
            total += 16 + -(-span // 256) * 256 * 4 + c * 8
    return total


def case(name, h, stream, slot_bytes, rounds):
    out = {"shape": name, "n_envs": h.n_envs}
    out["book_loop_s"], books = book_loop(h)
    out["mean_levels"] = float(np.mean([len(side) for b in books for side in b]))
    for k in KS:
        ms, lo, hi, rows, counts = time_write(h, stream, k, rounds)
        check(books, k, rows, counts)
        written = rows.nbytes + counts.nbytes
        read = slot_bytes * h.n_envs if slot_bytes else ladder_bytes(rows, counts, k)
        out["k%d" % k] = {"ms": ms, "ms_min": lo, "ms_max": hi, "bytes_read": read, "bytes_written": written,
                          "TBps": (read + written) / (ms * 1e-3) / 1e12, "book_loop_over_kernel": out["book_loop_s"] * 1e3 / ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "build_id": mxabides.build_id(), "rounds": a.rounds, "cases": []}
    m = mxabides.VecMarket("rmsc03", list(range(1, 4097)))
    m.set_parity_hash(False)
    m.set_stream(stream.cuda_stream)
    m.run(chunk=5000, max_launches=3)
    lay = m.layout()
    res["cases"].append(case("rmsc03 x4096 after 15,000 pops", m, stream, lay["tx"] - lay["book"], a.rounds))
    m.close()
    tp = tape.Tape.load(os.path.join(ROOT, "tests", "golden", "tape_IBM_2003-01-14.npz"))
    v = VecABIDESEnv(tp, 512)
    v.set_parity_hash(False)
    v.set_stream(stream.cuda_stream)
    acts = np.tile(np.array([0.01, 0.5, 0.5]), (512, 1))
    for _ in range(100):
        v.step(acts)
    res["cases"].append(case("IBM 2003-01-14 replay x512 after 100 steps", v, stream, 0, a.rounds))
    v.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
