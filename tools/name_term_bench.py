"""NameMatch inside queries (das_scan_node_names, das_table_name_filter;
names.hip), two measurements, each path in a fresh child process, the figure
the median wall time of the repeated calls after a checked first call, kernel
times from the library's per-kernel events in a pass of their own.

cut-over: das_table_name_filter forced to `walk` and to `flags` on the KB of
profiles/name_search.json (10^7 "Concept n<i>" nodes), over one-column tables
of 10^3 .. 10^8 random node ids.  Reports the smallest measured row count from
which `flags` is never slower (null: there is none).

query: on a FlyBase-shaped KB (synthetic.flybase_kb) the one-call query

    And([NameMatch(v2, Verbatim, p), Link(Execution, [gene_uniquename, v1, v2]),
         Link(Execution, [gene_map_table_recombination_loc, v2, v3])])

against the notebook's loop -- get_matched_node_name, then per name
get_node_name and the two Link queries -- which runs unchanged without the
term.  Patterns that match 1, 10^2 and 10^4 names.  GPU box:

    python tools/name_term_bench.py [--out profiles/name_term.json]
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

FILTER_PATTERNS = [r"^n\d+7$", "CoA", "^n1234567$"]
QUERY_PATTERNS = [r"^FBgn0001234$", r"^FBgn00012\d\d$", r"^FBgn001\d\d\d\d$"]
S_UNIQ, S_LOC = "Schema:gene_uniquename", "Schema:gene_map_table_recombination_loc"
FILTER_SCOPES = ["k_name_filter", "k_name_filter_flags", "k_name_match"]


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 4)


def child_filter(args):
    import numpy as np
    from das_amd import _lib
    from das_amd.database.hip_db import HipDB
    from tools.name_search_bench import numbered_kb
    db = HipDB(device=0)
    db.load_arrays(numbered_kb(args.nodes))
    tid = db.type_id["Concept"]
    n_nodes, n_bytes, ascii_only = db.ctx.node_name_stats(tid)
    ids, _ = db.ctx.match_node_names(tid, db._name_dfa("", ascii_only))
    lut = np.zeros(int(ids.max()) + 1, dtype=bool)
    mode_id = {"walk": _lib.NAME_FILTER_WALK, "flags": _lib.NAME_FILTER_FLAGS}[args.mode]
    rng = np.random.default_rng(1)
    out = {"mode": args.mode, "nodes": n_nodes, "name_bytes": n_bytes, "sizes": {}}
    rows = 1000
    while rows <= args.max_rows:
        vals = ids[rng.integers(0, ids.size, rows)]
        table = db.ctx.table_from_host(_lib.TABLE_ORDERED, [0], vals.reshape(1, -1))
        reps = args.reps if rows <= 10 ** 6 else max(3, args.reps // 3)
        rec = out["sizes"][str(rows)] = {}
        for p in FILTER_PATTERNS:
            dfa = db._name_dfa(p, ascii_only)
            hits, _ = db.ctx.match_node_names(tid, dfa)
            lut[:] = False
            lut[hits] = True
            kept = int(lut[vals].sum())
            assert db.ctx.table_name_filter(table, 0, tid, dfa, mode_id).nrows == kept, (p, rows)
            r = {"kept": kept, "reps": reps,
                 "median_ms": _median_ms(lambda: db.ctx.table_name_filter(table, 0, tid, dfa, mode_id).free(), reps)}
            db.ctx.prof_enable(True)
            db.ctx.prof_only("|".join(FILTER_SCOPES))
            db.ctx.prof_reset()
            for _ in range(reps):
                db.ctx.table_name_filter(table, 0, tid, dfa, mode_id).free()
            st = db.ctx.prof_stats()
            db.ctx.prof_enable(False)
            for k in FILTER_SCOPES:
                if k in st and st[k]["launches"]:
                    ms = st[k]["ms"] / st[k]["launches"]
                    b = st[k]["bytes"] / st[k]["launches"]
                    r[k] = {"kernel_ms": round(ms, 4), "algorithmic_bytes": int(b),
                            "achieved_GBps": round(b / (ms * 1e-3) / 1e9, 2) if ms > 0 else None}
            rec[p] = r
            print(f"[{args.mode}] rows {rows} {p!r}: {r}", file=sys.stderr, flush=True)
        table.free()
        rows *= 10
    print(json.dumps(out), flush=True)


def _flybase_db(args):
    from das_amd import synthetic
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(synthetic.flybase_kb(n_genes=args.genes, n_schema=6, rows_per_schema=50_000))
    return db


def child_query(args):
    from das_amd.pattern_matcher import pattern_matcher as pm
    db = _flybase_db(args)
    out = {"mode": "query", "genes": args.genes, "patterns": {}}

    def expr(p):
        return pm.And([pm.NameMatch("v2", "Verbatim", p),
                       pm.Link("Execution", [pm.Node("Schema", S_UNIQ), pm.Variable("v1"), pm.Variable("v2")], True),
                       pm.Link("Execution", [pm.Node("Schema", S_LOC), pm.Variable("v2"), pm.Variable("v3")], True)])

    def run(p, rows):
        ans = pm.PatternMatchingAnswer()
        assert expr(p).matched(db, ans)
        return len(ans.assignments) if rows else ans.count()

    for p in QUERY_PATTERNS:
        n = run(p, True)
        assert n == run(p, False)
        r = {"rows": n, "reps": args.reps, "median_ms": _median_ms(lambda: run(p, False), args.reps),
             "median_ms_rows_read": _median_ms(lambda: run(p, True), args.reps)}
        db.ctx.prof_enable(True)
        db.ctx.prof_only(None)
        db.ctx.prof_reset()
        for _ in range(args.reps):
            run(p, False)
        st = db.ctx.prof_stats()
        db.ctx.prof_enable(False)
        r["kernels_ms"] = round(sum(v["ms"] for v in st.values()) / args.reps, 4)
        r["kernels"] = {k: round(v["ms"] / args.reps, 4) for k, v in sorted(st.items()) if v["launches"]}
        r["kernel_share_of_call"] = round(r["kernels_ms"] / r["median_ms"], 3)
        out["patterns"][p] = r
        print(f"[query] {p!r}: rows {n} {r['median_ms']} ms (rows read {r['median_ms_rows_read']} ms), "
              f"kernels {r['kernels_ms']} ms", file=sys.stderr, flush=True)
    out["path"] = dict(db.name_term_stats)
    print(json.dumps(out), flush=True)


def child_loop(args):
    """QueryFlyBase.ipynb's cell, as it runs without the term."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    db = _flybase_db(args)
    out = {"mode": "loop", "genes": args.genes, "patterns": {}}

    def run(p):
        n = 0
        for h in db.get_matched_node_name("Verbatim", p):
            name = db.get_node_name(h)
            a1, a2 = pm.PatternMatchingAnswer(), pm.PatternMatchingAnswer()
            q1 = pm.Link("Execution", [pm.Node("Schema", S_UNIQ), pm.Variable("v1"), pm.Node("Verbatim", name)], True)
            q2 = pm.Link("Execution", [pm.Node("Schema", S_LOC), pm.Node("Verbatim", name), pm.Variable("v3")], True)
            if q1.matched(db, a1) and q2.matched(db, a2):
                n += len(a1.assignments) * len(a2.assignments)
        return n

    for p in QUERY_PATTERNS:
        n = run(p)
        reps = args.reps if n <= 1000 else 1
        out["patterns"][p] = {"rows": n, "reps": reps, "median_ms": _median_ms(lambda: run(p), reps)}
        print(f"[loop] {p!r}: {out['patterns'][p]}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def cut_over(walk, flags):
    """The smallest measured row count from which flags is never slower, over
    every pattern and every larger measured size; None: there is none."""
    sizes = sorted(int(s) for s in walk["sizes"])
    best = None
    for s in reversed(sizes):
        if all(flags["sizes"][str(s)][p]["median_ms"] <= walk["sizes"][str(s)][p]["median_ms"]
               for p in FILTER_PATTERNS):
            best = s
        else:
            break
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--max-rows", type=int, default=100_000_000)
    ap.add_argument("--genes", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "name_term.json"))
    ap.add_argument("--mode", choices=["walk", "flags", "query", "loop"], help=argparse.SUPPRESS)   # child process
    args = ap.parse_args()
    if args.mode:
        return {"walk": child_filter, "flags": child_filter, "query": child_query, "loop": child_loop}[args.mode](args)
    rec = {"tool": "tools/name_term_bench.py", "nodes": args.nodes, "genes": args.genes,
           "filter_patterns": FILTER_PATTERNS, "query_patterns": QUERY_PATTERNS}
    for mode in ("walk", "flags", "query", "loop"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--nodes", str(args.nodes),
                            "--max-rows", str(args.max_rows), "--genes", str(args.genes), "--reps", str(args.reps)],
                           stdout=subprocess.PIPE, text=True, check=True)
        rec[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    rows = cut_over(rec["walk"], rec["flags"])
    rec["flags_never_slower_from_rows"] = rows
    rec["flags_never_slower_from_rows_per_node"] = None if rows is None else rows / rec["walk"]["nodes"]
    assert rec["query"]["path"]["device"] > 0 and rec["query"]["path"]["host"] == 0
    for p in QUERY_PATTERNS:
        q, l = rec["query"]["patterns"][p], rec["loop"]["patterns"][p]
        assert q["rows"] == l["rows"], p
        print(f"{p!r}: {q['rows']} rows; one query {q['median_ms']} ms ({q['median_ms_rows_read']} ms with the rows "
              f"read; kernels {q['kernels_ms']} ms), loop {l['median_ms']} ms")
    print(f"flags never slower from {rows} rows")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
