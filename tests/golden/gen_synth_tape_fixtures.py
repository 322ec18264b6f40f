#!/usr/bin/env python3
"""Reference fixtures of the crafted replay tapes (tests/synth_tapes.py).

CONTAINER-ONLY TEST INFRASTRUCTURE, like gen_fixtures.py: it runs the *reference* (read-only) and
never runs on the GPU machine.  Nothing under tests/ imports it.

For each reference-checked tape it writes the tape as a LOBSTER message CSV (our own data) into a
temporary working directory, asserts that mxabides.tape.load_lobster reads the builder's arrays
back exactly (the host ingestion path), and runs the reference on that CSV:

  runner tapes   gen_fixtures.py "run marketreplay:<T>:<date> 1 <out> --full" (config/marketreplay.py)
  gym tapes      gen_mr_fixtures.py (ABIDESEnv, one episode) / gen_episodes_fixtures.py (several
                 episodes in one process), their LOBSTEROrdersProcessor pointed at the CSV

Outputs: tests/golden/synth_<name>.json, .npz, _summary.json (runner tapes) and
tape_<T>_<date>.npz.  A gym fixture keeps per episode the actions, every step's observation,
done flag and event count, the trace head, the whole-episode hash, and the
final books as order counts and digests (a skip tape's book holds 3,600 orders).  The .npz files
are written with fixed zip timestamps, so a second run reproduces every file byte for byte.

Usage: python tests/golden/gen_synth_tape_fixtures.py [name ...]
       python tests/golden/gen_synth_tape_fixtures.py --gym-child NAME CSV   (internal)
"""
import hashlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "marl-optimal-execution_amd")):
    sys.path.insert(0, p)
import synth_tapes as S  # noqa: E402
from mxabides import tape as T  # noqa: E402

GYM_SEED, GYM_ACTION_SEED = 789, 1


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed zip timestamp (byte-for-byte reproducible)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)


def save_tape(tp):
    save_npz(os.path.join(HERE, "tape_%s_%s.npz" % (tp.symbol, tp.date)), t=tp.t, oid=tp.oid, price=tp.price,
             size=tp.size, buy=tp.buy, symbol=np.array(tp.symbol), date=np.array(tp.date))


def write_csv(tp, wd):
    """the tape as LOBSTER's <T>_<date>_34200000_57600000_message_1.csv: seconds after midnight
    (whole milliseconds), event type 1, id, size, price in 1e-4 $, 1 / -1"""
    assert (tp.t % S.NS_MS == 0).all(), "reference-checked tapes keep whole milliseconds"
    d = os.path.join(wd, "data", "lobster", "LOBSTER_SampleFile_%s_%s_1" % (tp.symbol, tp.date))
    os.makedirs(d)
    path = os.path.join(d, "%s_%s_34200000_57600000_message_1.csv" % (tp.symbol, tp.date))
    with open(path, "w") as f:
        for t, oid, price, size, buy in zip(tp.t, tp.oid, tp.price, tp.size, tp.buy):
            ms = int(t) // S.NS_MS
            f.write("%d.%03d,1,%d,%d,%d,%d\n" % (ms // 1000, ms % 1000, oid, size, price * 100, 1 if buy else -1))
    back = T.load_lobster(path, tp.date)
    for k in ("t", "oid", "price", "size", "buy"):
        assert (getattr(back, k) == getattr(tp, k)).all(), (tp.symbol, k)
    assert back.symbol == tp.symbol and back.date == tp.date
    return path


def run_runner(name):
    tp, _ = S.RUNNER_TAPES[name]()
    wd = tempfile.mkdtemp(prefix="synth_")
    write_csv(tp, wd)
    out = os.path.join(HERE, "synth_" + name)
    subprocess.check_call([sys.executable, os.path.join(HERE, "gen_fixtures.py"), "run",
                           "marketreplay:%s:%s" % (tp.symbol, tp.date), "1", out, "--full"], cwd=wd,
                          env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    trace = np.load(out + ".npz")["trace"]
    save_npz(out + ".npz", trace=trace)
    for f in (out + ".json", out + "_summary.json"):  # one line each
        with open(f) as fh:
            d = json.load(fh)
        with open(f, "w") as fh:
            json.dump(d, fh, separators=(",", ":"))
    save_tape(tp)
    shutil.rmtree(wd)
    print(name, "records", len(tp), "events", len(trace))


TRACE_HEAD = 2000  # records kept verbatim; the hash covers every pop


def book_digest(levels):
    """sha256 over a side's levels ([[id, agent, quantity, price], ...] per level, best first, FIFO)"""
    return hashlib.sha256(json.dumps(levels, separators=(",", ":")).encode()).hexdigest()


def compact_episode(ep, actions, trace, sfx):
    """the per-step records as arrays: observation [steps][9] (NaN rows where the step returned
    none), done flags and ttl_messages, beside the actions and the trace head"""
    obs = np.full((len(ep["steps"]), 9), np.nan)
    for i, st in enumerate(ep["steps"]):
        if st["obs"]:
            obs[i] = st["obs"]
    return {"actions" + sfx: actions, "trace" + sfx: trace[:TRACE_HEAD], "obs" + sfx: obs,
            "done" + sfx: np.array([st["done"] for st in ep["steps"]], dtype=np.int8),
            "events" + sfx: np.array([st["events"] for st in ep["steps"]], dtype=np.int64)}


def episode_record(ep):
    """what stays in the JSON: counts, hashes, both books as (orders, digest), the agents' holdings"""
    return {"events": ep["events"], "hash": ep["hash"],
            "order_id_counter_start": ep.get("order_id_counter_start", 0), "order_id_counter": ep["order_id_counter"],
            "bids": [sum(len(lv) for lv in ep["bids"]), book_digest(ep["bids"])],
            "asks": [sum(len(lv) for lv in ep["asks"]), book_digest(ep["asks"])],
            "agents": [{"id": a["id"], "holdings": a["holdings"], "n_open": len(a["open_orders"])} for a in ep["agents"]]}


def gym_child(name, csv):
    """one reference process: gen_mr_fixtures / gen_episodes_fixtures with the processor reading csv"""
    sys.path.insert(0, HERE)
    import gen_mr_fixtures as M
    M.install_stubs()
    from agent.examples import MarketReplayAgent as MRA
    orig = MRA.LOBSTEROrdersProcessor.__init__

    def init(self, symbol, date_, start_time, end_time, orders_file_path, processed_orders_folder_path):
        orig(self, symbol, date_, start_time, end_time, csv, processed_orders_folder_path)

    MRA.LOBSTEROrdersProcessor.__init__ = init
    tp, _ = S.GYM_TAPES[name]()
    episodes = S.GYM_EPISODES.get(name, 1)
    if episodes == 1:
        sys.argv = ["gen_mr_fixtures.py", tp.symbol, tp.date, str(GYM_SEED), str(GYM_ACTION_SEED)]
        M.main()
        base = os.path.join(HERE, "mr_%s_%s_%d_%d" % (tp.symbol, tp.date, GYM_SEED, GYM_ACTION_SEED))
    else:
        import gen_episodes_fixtures as E
        E.run_mr(tp.symbol, tp.date, GYM_SEED, GYM_ACTION_SEED, episodes)
        base = os.path.join(HERE, "eps_mr_%s_%s_%d_%d" % (tp.symbol, tp.date, GYM_SEED, GYM_ACTION_SEED))
    with open(base + ".json") as f:
        d = json.load(f)
    z = np.load(base + ".npz")
    eps = d["episodes"] if episodes > 1 else [d]
    arrays, small = {}, []
    for k, ep in enumerate(eps, start=1):
        sfx = "_%d" % k
        arrays.update(compact_episode(ep, z["actions" + (sfx if episodes > 1 else "")],
                                      z["trace" + (sfx if episodes > 1 else "")], sfx))
        small.append(episode_record(ep))
    out = os.path.join(HERE, "synth_" + name)
    with open(out + ".json", "w") as f:
        json.dump({"ticker": tp.symbol, "date": tp.date, "seed": GYM_SEED, "action_seed": GYM_ACTION_SEED,
                   "episodes": small}, f, separators=(",", ":"))
    save_npz(out + ".npz", **arrays)
    os.remove(base + ".json")
    os.remove(base + ".npz")


def run_gym(name):
    tp, _ = S.GYM_TAPES[name]()
    wd = tempfile.mkdtemp(prefix="synth_")
    csv = write_csv(tp, wd)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--gym-child", name, csv], cwd=wd,
                          env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    save_tape(tp)
    shutil.rmtree(wd)
    print(name, "records", len(tp))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--gym-child":
        return gym_child(sys.argv[2], sys.argv[3])
    names = sys.argv[1:] or list(S.RUNNER_TAPES) + list(S.GYM_TAPES)
    for n in names:
        run_runner(n) if n in S.RUNNER_TAPES else run_gym(n)


if __name__ == "__main__":
    main()
