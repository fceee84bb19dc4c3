"""get_node_names / answer.names: the device call (das_node_names, a gather
over the resident name heap, names.hip) against the host loop it replaces
(DAS_NAME_FETCH=0: one get_node_name per handle) on a synthetic KB of
"Concept n<i>" nodes.

Each path runs in a fresh child process and is forced (NAME_FETCH_MIN = 0 on
the device, DAS_NAME_FETCH=0 on the host), so the figures do not depend on
where HipDB switches between them.  Per size -- a few small ones for the
crossover, then 10^3, 10^5 and 10^6 random ids, and one answer column of 10^6
rows -- the figure is the median wall time of the repeated calls after a first
one, whose names are checked against the handles they hash to.  The host
child measures twice: as loaded (every handle is a device lookup and every
name a device read) and after prefetch() (host mirrors); without the mirrors
it stops at --host-max ids.  The device child then times
the kernels alone with the library's per-kernel events, in a pass of its own,
and reports the copy kernel's name bytes (read + written) against the rate of
a plain copy.  GPU box:

    python tools/name_fetch_bench.py [--nodes 10000000] [--out profiles/name_fetch.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SMALL = [1, 2, 4, 8, 16, 32, 64, 256]
SIZES = [1000, 100_000, 1_000_000]
COLUMN_ROWS = 1_000_000
HBM_PEAK_COPY = 6.29e12         # bytes/s, measured float4 copy


def timed(fn, reps):
    """Median wall time in ms of `reps` calls (the caller has made a first one)."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 4)


def child(args):
    import numpy as np
    from name_search_bench import numbered_kb
    from das_amd import _lib, name_search
    from das_amd.database.hip_db import HipDB, Relation
    from das_amd.pattern_matcher import pattern_matcher as PM
    db = HipDB(device=0)
    db.NAME_FETCH_MIN = 0
    t0 = time.perf_counter()
    db.load_arrays(numbered_kb(args.nodes))
    db.ctx.sync()
    out = {"mode": args.mode, "nodes": args.nodes, "load_s": round(time.perf_counter() - t0, 3)}
    tid = db.type_id["Concept"]
    t0 = time.perf_counter()
    all_ids = db.ctx.match_node_names(tid, name_search.ACCEPT_ALL, cap=args.nodes)[0]      # (builds the heap)
    out["heap_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert all_ids.size == args.nodes
    rng = np.random.default_rng(1)
    picks = {n: all_ids[rng.integers(0, all_ids.size, n)] for n in SMALL + SIZES}
    column = all_ids[rng.permutation(all_ids.size)[:COLUMN_ROWS]]         # distinct: an answer's rows are a set

    def answer(ids):
        t = db.ctx.table_from_host(_lib.TABLE_ORDERED, [PM._vid("V1")], np.ascontiguousarray(ids).reshape(1, -1))
        a = PM.PatternMatchingAnswer()
        a._set(db, Relation([t]))
        return a

    def check(names, ids, aligned=True):
        # "Concept n<i>": spot checks against the handles the names hash to (an answer's rows: in any order)
        assert len(names) == len(ids)
        among = None if aligned else set(ids.tolist())
        for k in (0, len(names) // 2, len(names) - 1):
            i = int(db.ids_of([db.get_node_handle("Concept", names[k])])[0])
            assert i == int(ids[k]) if aligned else i in among, (k, names[k])

    def measure(limit, reps_of):
        rec = {}
        for n in SMALL + SIZES:
            if n > limit:
                rec[str(n)] = None
                continue
            ids = picks[n]
            names = db.get_node_names(ids)
            check(names, ids)
            rec[str(n)] = {"median_ms": timed(lambda: db.get_node_names(ids), reps_of(n)), "reps": reps_of(n)}
            print(f"[{args.mode}] {n} ids: {rec[str(n)]}", file=sys.stderr, flush=True)
        rows = min(COLUMN_ROWS, limit)
        ans = answer(column[:rows])
        check(ans.names("V1"), column[:rows], aligned=False)
        # a fresh answer per call: the host definition builds its Assignment objects each time, as a query does
        rec["column"] = {"rows": rows, "reps": reps_of(rows),
                         "median_ms": timed(lambda: answer(column[:rows]).names("V1"), reps_of(rows))}
        print(f"[{args.mode}] column: {rec['column']}", file=sys.stderr, flush=True)
        return rec

    if args.mode == "device":
        out["ids"] = measure(COLUMN_ROWS, lambda n: args.reps)
        # kernel times: HIP events, a pass of their own
        db.ctx.prof_enable(True)
        db.ctx.prof_only("k_name_locate|k_name_copy")
        out["kernels"] = {}
        for n in SIZES:
            off, data, kind = db.ctx.node_names(ids=picks[n])
            name_bytes = int(off[-1])
            db.ctx.prof_reset()
            for _ in range(args.reps):
                db.ctx.node_names(ids=picks[n])
            st = db.ctx.prof_stats()
            cp, lc = st["k_name_copy"], st["k_name_locate"]
            ms = cp["ms"] / cp["launches"]
            out["kernels"][str(n)] = {
                "name_bytes": name_bytes, "copy_ms": round(ms, 5), "copy_algorithmic_bytes": cp["bytes"] / cp["launches"],
                "copy_fraction_of_plain_copy": round(2.0 * name_bytes / (ms * 1e-3) / HBM_PEAK_COPY, 5),
                "locate_ms": round(lc["ms"] / lc["launches"], 5)}
        db.ctx.prof_enable(False)
        assert db._mirror is None
    else:
        out["as_loaded"] = measure(args.host_max, lambda n: 1 if n >= 10_000 else 3)
        t0 = time.perf_counter()
        db.prefetch()
        out["prefetch_s"] = round(time.perf_counter() - t0, 3)
        out["prefetched"] = measure(COLUMN_ROWS, lambda n: 1 if n >= 10_000 else 5)
    out["path"] = dict(db.name_fetch_stats)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9, help="timed calls per size on the device path")
    ap.add_argument("--host-max", type=int, default=1_000_000,
                    help="largest fetch of the host loop without prefetch() (about 0.1 ms per name there: "
                         "10^6 names and a 10^6-row column take some 7 minutes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "name_fetch.json"))
    ap.add_argument("--mode", choices=["device", "host"], help=argparse.SUPPRESS)      # child process
    args = ap.parse_args()
    if args.mode:
        return child(args)
    rec = {"tool": "tools/name_fetch_bench.py", "nodes": args.nodes, "sizes": SMALL + SIZES,
           "column_rows": COLUMN_ROWS, "plain_copy_Bps": HBM_PEAK_COPY}
    for mode in ("device", "host"):
        env = dict(os.environ, DAS_NAME_FETCH="1" if mode == "device" else "0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--nodes", str(args.nodes),
                            "--reps", str(args.reps), "--host-max", str(args.host_max)], env=env,
                           stdout=subprocess.PIPE, text=True, check=True)
        rec[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec[mode]["path"][mode] > 0 and rec[mode]["path"]["host" if mode == "device" else "device"] == 0
    # the smallest size from which the device call is never slower than the host loop
    for flavour in ("as_loaded", "prefetched"):
        cross = None
        for n in reversed(SMALL + SIZES):
            h, d = rec["host"][flavour][str(n)], rec["device"]["ids"][str(n)]
            if h is None:
                continue
            if d["median_ms"] > h["median_ms"]:
                break
            cross = n
        rec[f"device_not_slower_from_{flavour}"] = cross
    for n in SMALL + SIZES + ["column"]:
        d = rec["device"]["ids"][str(n)]
        h0, h1 = rec["host"]["as_loaded"][str(n)], rec["host"]["prefetched"][str(n)]
        print(f"{n}: device {d['median_ms']} ms; host loop {h0 and h0['median_ms']} ms as loaded, "
              f"{h1 and h1['median_ms']} ms prefetched")
    for n, k in rec["device"]["kernels"].items():
        print(f"{n} ids: copy kernel {k['copy_ms']} ms for {k['name_bytes']} name bytes = "
              f"{100 * k['copy_fraction_of_plain_copy']:.2f}% of a plain copy; locate {k['locate_ms']} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
