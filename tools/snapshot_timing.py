#!/usr/bin/env python3
"""Rate of the env-state snapshot kernel (include/mxa_snap.h) against one device-to-device
hipMemcpyAsync of the same byte count in the same process.

    python tools/snapshot_timing.py [--rounds 9] [--out profiles/snapshot/timing.json]

For rmsc03 x 4096 and random_fund_value x 64, mid-episode: identity save, identity restore and a fork
of one slot into every env, each with 4 and with 8 16-byte loads in flight per lane
(MXA_SNAPSHOT_LOADS), timed by the handle's HIP events (mxa_last_kernel_ms); the memcpy between
torch.cuda events on torch's stream.  The runs alternate; each figure is the median of `rounds`, the
memcpy's min and max are its run-to-run spread.  Bytes moved = 2 x the bytes copied (read + write);
the fork reads one slot, so its rate counts the bytes written only."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-optimal-execution_amd"))

import torch  # noqa: E402  (before libmxa loads: one HIP runtime per process)

import mxabides  # noqa: E402

CASES = [("rmsc03", 4096, 5000), ("random_fund_value", 64, 5000)]


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            pass
    raise SystemExit("libamdhip64.so not found")


def time_memcpy(hip, dst, src, nbytes):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream()
    e0.record(stream)
    rc = hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(nbytes),
                            3, ctypes.c_void_p(stream.cuda_stream))  # 3: hipMemcpyDeviceToDevice
    assert rc == 0, rc
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def case(hip, cfg, n_envs, pops, rounds):
    m = mxabides.VecMarket(cfg, list(range(1, n_envs + 1)))
    m.set_parity_hash(False)
    m.run(chunk=pops, max_launches=1)
    nbytes = m.env_bytes * n_envs
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    snaps = {}
    for loads in (4, 8):
        os.environ["MXA_SNAPSHOT_LOADS"] = str(loads)
        snaps[loads] = (m.snapshot(), m.snapshot(1))
        snaps[loads][0].save()
        snaps[loads][1].save({0: 0})
    os.environ.pop("MXA_SNAPSHOT_LOADS")
    t = {"memcpy": []}
    fork_map = {e: 0 for e in range(n_envs)}
    for r in range(rounds + 1):  # round 0 warms up
        row = {"memcpy": time_memcpy(hip, dst, src, nbytes)}
        for loads, (full, one) in snaps.items():
            full.save()
            row["save_%d" % loads] = m.last_kernel_ms
            full.restore()
            row["restore_%d" % loads] = m.last_kernel_ms
            one.restore(fork_map)
            row["fork_%d" % loads] = m.last_kernel_ms
            full.restore()  # every env its own state again
        if r:
            for k, v in row.items():
                t.setdefault(k, []).append(v)
    out = {"config": cfg, "n_envs": n_envs, "env_bytes": m.env_bytes, "bytes": nbytes, "rounds": rounds,
           "memcpy_ms_min": min(t["memcpy"]), "memcpy_ms_max": max(t["memcpy"])}
    for k, v in t.items():
        ms = statistics.median(v)
        out[k + "_ms"] = ms
        out[k + "_TBps"] = (1 if k.startswith("fork") else 2) * nbytes / (ms * 1e-3) / 1e12
    for full, one in snaps.values():
        full.close()
        one.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    hip = hip_runtime()
    res = {"device": torch.cuda.get_device_name(0), "build_id": mxabides.build_id(),
           "cases": [case(hip, *c, a.rounds) for c in CASES]}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
