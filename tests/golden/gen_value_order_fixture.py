#!/usr/bin/env python3
"""The tight composition of tests/test_gpu_value_order_inplace.py: cap_rmsc03_b.json, settings only.

rmsc03's own composition (oracle/pyoracle.config_defaults) with 18 value agents and the smallest
book a composition allows (64 resting orders; queue 192).  Over that test file's eight seeds the
oracle's peaks of resting orders are 61..65: one env ends exactly full, one needs a slot more, and
the order that finds the book full is a value agent's resting LIMIT_ORDER directly behind its wake
group.  The capacities are fixed points of the engine's rounding (include/mxa.h
mxa_config_capacities).  __graft_entry__.compositions() picks the file up with the other
cap_*.json, so build() compiles its engine.  The oracle is the checker at test time.

Usage: python tests/golden/gen_value_order_fixture.py [--peaks]   (--peaks: print the oracle's peaks)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_capacity_fixtures import composition  # noqa: E402  (also puts oracle/ on sys.path)

NAME, BASE, N_VALUE, QUEUE, BOOK = "cap_rmsc03_b", "rmsc03", 18, 192, 64
SEEDS = [123456789, 1008, 7, 11, 2, 3, 5, 13]  # tests/test_gpu_limit_inplace.py


def main():
    d = composition(BASE, None, QUEUE, BOOK)[1]
    d["n_value"] = N_VALUE
    with open(os.path.join(HERE, NAME + ".json"), "w") as f:
        json.dump({"composition": d}, f, indent=0)
        f.write("\n")
    if "--peaks" in sys.argv:
        import numpy as np
        import pyoracle
        c = pyoracle.config_defaults(BASE)
        c.n_value, c.queue_capacity, c.book_capacity = N_VALUE, QUEUE, BOOK
        st = pyoracle.run_batch_config(c, np.array(SEEDS, dtype=np.uint32), os.cpu_count() or 1, stats=True)[4]
        print("%s resting %s, capacity %d" % (NAME, st[:, 1].tolist(), BOOK))


if __name__ == "__main__":
    main()
