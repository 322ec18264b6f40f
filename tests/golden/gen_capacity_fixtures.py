#!/usr/bin/env python3
"""The tight compositions of tests/test_gpu_capacity_edges.py: cap_<name>.json, settings only.

Each is a base script's own composition (oracle/pyoracle.config_defaults) with other agent counts
and a queue_capacity / book_capacity that the oracle's peak of pending events / resting orders
straddles over the seed pool (arange(N) * 7919 + 3): some envs end exactly full, some need one
slot more.  The capacities are fixed points of the engine's rounding (include/mxa.h
mxa_config_capacities).  __graft_entry__.compositions() picks the files up, so build() compiles
their engines.  No reference run is involved: the oracle is the checker at test time.

Usage: python tests/golden/gen_capacity_fixtures.py [--peaks]   (--peaks: print the oracle's peaks)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ZI95 = [14, 14, 13, 13, 13, 14, 14]
# name -> (base, ZI counts per strategy group or None, queue_capacity, book_capacity, pool size)
CAPACITY_COMPOSITIONS = {
    "cap_zi95_q": ("sparse_zi_100", ZI95, 192, 128, 2048),
    "cap_zi95_b": ("sparse_zi_100", ZI95, 256, 64, 2048),
    "cap_zi95_qb": ("sparse_zi_100", ZI95, 192, 64, 2048),
    "cap_zi384_q": ("sparse_zi_1000", [60, 54, 54, 54, 54, 54, 54], 768, 0, 512),
    "cap_zi767_q": ("sparse_zi_1000", [114, 109, 109, 109, 109, 109, 108], 1536, 0, 512),
    "cap_rmsc03_q": ("rmsc03", None, 128, 0, 2048),
}


def composition(base, counts, q, b):
    """the fields of mxabides.composition.to_dict"""
    import pyoracle
    c = pyoracle.config_defaults(base)
    if counts is not None:
        assert c.n_zi_groups == len(counts)
        for g, k in enumerate(counts):
            c.zi_count[g] = k
    c.queue_capacity, c.book_capacity = q, b
    d = {}
    for k, _ in c._fields_:
        v = getattr(c, k)
        if k == "mm":
            d[k] = {n: getattr(v, n) for n, _ in v._fields_}
        elif k in ("zi_count", "zi_r_min", "zi_r_max", "zi_eta"):
            d[k] = list(v)
        else:
            d[k] = v
    return c, d


def main():
    import numpy as np
    import pyoracle
    for name, (base, counts, q, b, n) in CAPACITY_COMPOSITIONS.items():
        c, d = composition(base, counts, q, b)
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump({"composition": d}, f, indent=0)
            f.write("\n")
        if "--peaks" in sys.argv:
            seeds = ((np.arange(n, dtype=np.int64) * 7919 + 3) & 0xFFFFFFFF).astype(np.uint32)
            st = pyoracle.run_batch_config(c, seeds, os.cpu_count() or 1, stats=True)[4]
            for col, what, cap in ((0, "pending", q), (1, "resting", b)):
                p = st[:, col]
                print("%s %s %d..%d, capacity %d: %d below, %d at, %d one over, %d further over" %
                      (name, what, p.min(), p.max(), cap, (p < cap).sum(), (p == cap).sum(), (p == cap + 1).sum(),
                       (p > cap + 1).sum()))


if __name__ == "__main__":
    main()
