"""get_matched_node_name: the device path (DFA matcher over the resident name
heap, names.hip) against the host path (DAS_NAME_SEARCH=0: `re.search` over a
host copy of the names) on a synthetic KB of "Concept n<i>" nodes.

Each path runs in a fresh child process.  Per pattern: the first call (on the
first pattern it also builds the name heap, or copies the atoms to the host)
is reported apart; the figure is the median wall time of the repeated calls
after it.  The device child then times the matcher kernel alone with the
library's per-kernel events and reports its fraction of the HBM peak:
(heap bytes + offsets + flags of the type) / kernel time.  GPU box:

    python tools/name_search_bench.py [--nodes 10000000] [--out profiles/name_search.json]
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

PATTERNS = ["CoA", r"^n\d+7$", "^n1234567$"]
HBM_PEAK_SPEC = 8.0e12          # bytes/s, MI355X HBM3E (spec)
HBM_PEAK_COPY = 6.29e12         # bytes/s, measured float4 copy


def numbered_kb(n_nodes):
    """n_nodes terminals "Concept n<i>" and a handful of links (a normal build)."""
    import numpy as np
    from das_amd import synthetic
    from das_amd.loader import AtomArrays
    leaves, names = synthetic.powerlaw_leaves(n_nodes, 1)            # types T0, Concept
    n_types = len(names)
    k = min(4, n_nodes // 2)
    child = np.array([[0, n_types + 2 * i, n_types + 2 * i + 1] for i in range(k)], dtype=np.uint32).reshape(-1)
    return AtomArrays(*leaves, np.arange(k + 1, dtype=np.uint64) * 3, child, np.ones(k, np.uint8),
                      np.full(k, -1, np.int32), np.array([0, k], dtype=np.uint64), names)


def child(args):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    t0 = time.perf_counter()
    db.load_arrays(numbered_kb(args.nodes))
    db.ctx.sync()
    out = {"mode": args.mode, "nodes": args.nodes, "load_s": round(time.perf_counter() - t0, 3), "patterns": {}}
    bytes_before = int(db.ctx.stats().device_bytes)
    for p in PATTERNS:
        t0 = time.perf_counter()
        n = len(db.get_matched_node_name("Concept", p))
        first = time.perf_counter() - t0
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            db.get_matched_node_name("Concept", p)
            ts.append(time.perf_counter() - t0)
        out["patterns"][p] = {"matches": n, "first_call_ms": round(first * 1e3, 3),
                              "median_ms": round(statistics.median(ts) * 1e3, 3), "reps": args.reps}
        print(f"[{args.mode}] {p!r}: {out['patterns'][p]}", file=sys.stderr, flush=True)
    out["path"] = dict(db.name_search_stats)
    if args.mode == "device":
        tid = db.type_id["Concept"]
        n_nodes, n_bytes, ascii_only = db.ctx.node_name_stats(tid)
        out["heap_device_bytes"] = int(db.ctx.stats().device_bytes) - bytes_before
        out["name_bytes"], out["ascii_only"] = n_bytes, ascii_only
        algorithmic = n_bytes + 8 * (n_nodes + 1) + n_nodes
        db.ctx.prof_enable(True)
        db.ctx.prof_only("k_name_match")
        for p in PATTERNS:
            db.ctx.prof_reset()
            for _ in range(args.reps):
                db.get_matched_node_name("Concept", p)
            st = db.ctx.prof_stats()["k_name_match"]
            ms = st["ms"] / st["launches"]
            assert abs(st["bytes"] / st["launches"] - algorithmic) < 1
            out["patterns"][p].update(kernel_ms=round(ms, 4), kernel_bytes=algorithmic,
                                      hbm_fraction_of_spec=round(algorithmic / (ms * 1e-3) / HBM_PEAK_SPEC, 4),
                                      hbm_fraction_of_copy=round(algorithmic / (ms * 1e-3) / HBM_PEAK_COPY, 4))
        db.ctx.prof_enable(False)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15, help="timed calls per pattern on the device path")
    ap.add_argument("--host-reps", type=int, default=3, help="timed calls per pattern on the host path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "name_search.json"))
    ap.add_argument("--mode", choices=["device", "host"], help=argparse.SUPPRESS)      # child process
    args = ap.parse_args()
    if args.mode:
        return child(args)
    rec = {"tool": "tools/name_search_bench.py", "nodes": args.nodes, "patterns": PATTERNS,
           "hbm_peak_spec_Bps": HBM_PEAK_SPEC, "hbm_peak_copy_Bps": HBM_PEAK_COPY}
    for mode, reps in (("device", args.reps), ("host", args.host_reps)):
        env = dict(os.environ, DAS_NAME_SEARCH="1" if mode == "device" else "0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--nodes", str(args.nodes),
                            "--reps", str(reps)], env=env, stdout=subprocess.PIPE, text=True, check=True)
        rec[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec[mode]["path"][mode] > 0 and rec[mode]["path"]["host" if mode == "device" else "device"] == 0
    for p in PATTERNS:
        d, h = rec["device"]["patterns"][p], rec["host"]["patterns"][p]
        assert d["matches"] == h["matches"], p
        print(f"{p!r}: {d['matches']} matches; device {d['median_ms']} ms (kernel {d['kernel_ms']} ms, "
              f"{100 * d['hbm_fraction_of_spec']:.1f}% of HBM peak), host {h['median_ms']} ms; "
              f"first call device {d['first_call_ms']} ms, host {h['first_call_ms']} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
