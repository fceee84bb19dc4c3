"""answer.value_counts: the device call (das_group_counts, group.hip) on the
bench's own KBs, against the host definition it replaces and against the cost
of writing the rows it leaves unwritten.

(a) crossover: answers of 1 .. 2^18 rows (the first rows of the bio KB's
    Member scan, grouped by process) through the device path and through DAS_GROUP=0 (the host Counter
    over Assignment objects, built afresh per call as a query does), in the
    same process; the smallest size from which the device call is never slower.
(b) bio Q6 (bench.py's QUERY_3, a deferred cross product) grouped by each of
    its variables, device only, beside the time the same process takes to
    settle the product (the k_cartesian scope): the cost avoided.
(c) the FlyBase uniquename x recombination_loc index join in both
    DAS_DEFER_JOIN modes, grouped by each variable.
(d) the two strategies against each other (DAS_GROUP_DIRECT=1 / =0): 4096 and
    2^22 rows of uniform keys over ranges from the LDS tile (4096 bins) and
    one past it (global atomics) to 2^26 bins.

Per case the figure is the median wall time of the repeated calls after a
first one.  GPU box:

    python tools/group_bench.py [--out profiles/group_counts.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [1, 4, 16, 64, 256, 1024, 4096, 16384, 65536, 262144]


def timed(fn, reps):
    """Median wall time in ms of `reps` calls (the caller has made a first one)."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 4)


def ask(bench, pm, db, spec):
    ans = pm.PatternMatchingAnswer()
    assert bench.build_expr(pm, spec).matched(db, ans)
    return ans


def variables(pm, ans):
    return sorted({pm._var_name(v) for t in ans._rel.tables for v in t.vars})


def grouped(db, pm, ans, reps):
    """Per variable of the answer: groups, the device call's time, the largest count."""
    out = {}
    for v in variables(pm, ans):
        before = dict(db.group_stats)
        vc = ans.value_counts(v)
        assert vc.ids is not None and vc.total == ans.count()
        out[v] = {"groups": len(vc), "max_count": int(vc.counts.max()) if len(vc) else 0,
                  "median_ms": timed(lambda: ans.value_counts(v), reps),
                  "unwritten": db.group_stats["unwritten"] - before["unwritten"],
                  "settled": db.group_stats["settled"] - before["settled"]}
        print(f"  {v}: {out[v]}", file=sys.stderr, flush=True)
    return out


def settle_ms(db, ans, scope):
    """Settles the answer's tables (das_table_column); the scope's recorded ms."""
    from das_amd import _lib
    db.ctx.prof_enable(True)
    db.ctx.prof_reset()
    t0 = time.perf_counter()
    for t in ans._rel.tables:
        p = ctypes.c_void_p()
        _lib.check(_lib.lib().das_table_column(t.h, 0, ctypes.byref(p)))
    db.ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    st = {k: v for k, v in db.ctx.prof_stats().items() if k.startswith(scope)}
    db.ctx.prof_enable(False)
    db.ctx.prof_reset()
    return {"wall_ms": round(wall, 3), "kernel_ms": round(sum(v["ms"] for v in st.values()), 3),
            "launches": sum(v["launches"] for v in st.values()), "bytes": sum(v["bytes"] for v in st.values())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genes", type=int, default=200_000)
    ap.add_argument("--bps", type=int, default=50_000)
    ap.add_argument("--members", type=int, default=20_000_000)
    ap.add_argument("--inheritance", type=int, default=100_000)
    ap.add_argument("--fb-genes", type=int, default=300_000)
    ap.add_argument("--fb-schema", type=int, default=60)
    ap.add_argument("--fb-rows", type=int, default=450_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=262144, help="largest answer the host definition is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_counts.json"))
    args = ap.parse_args()

    import numpy as np
    import bench
    from das_amd import _lib, synthetic
    from das_amd.database.hip_db import HipDB, Relation
    from das_amd.pattern_matcher import pattern_matcher as pm

    rec = {"tool": "tools/group_bench.py", "reps": args.reps,
           "bio": {"genes": args.genes, "bps": args.bps, "members": args.members, "inheritance": args.inheritance},
           "flybase": {"genes": args.fb_genes, "schemas": args.fb_schema, "rows": args.fb_rows}}
    for k in ("DAS_GROUP", "DAS_GROUP_DIRECT", "DAS_DEFER_JOIN", "DAS_DEFER_PRODUCT"):
        os.environ.pop(k, None)

    # ---- bio -------------------------------------------------------------------------------------------
    db = HipDB(device=0)
    db.GROUP_MIN = 0
    db.load_arrays(synthetic.bio_full_kb(args.genes, args.bps, args.members, args.inheritance))
    specs = dict((name[:2], q) for name, q in bench.bio_specs(np.arange(args.genes)))

    # (a) the crossover, on slices of the Member scan's process column
    scan = ask(bench, pm, db, specs["Q1"])
    t, = scan._rel.tables
    rows_ab = t.fetch(0, SIZES[-1])                  # both columns: an answer's rows are distinct
    ab_vars, var = list(t.vars), pm._vid("V_bp")

    def answer(n):
        a = pm.PatternMatchingAnswer()
        a._set(db, Relation([db.ctx.table_from_host(_lib.TABLE_ORDERED, ab_vars, np.ascontiguousarray(rows_ab[:, :n]))]))
        return a

    cross = {}
    for n in [s for s in SIZES if s <= rows_ab.shape[1]]:
        os.environ.pop("DAS_GROUP", None)
        dev = answer(n).value_counts("V_bp")
        d_ms = timed(lambda: answer(n).value_counts("V_bp"), args.reps)
        h_ms = None
        if n <= args.host_max:
            os.environ["DAS_GROUP"] = "0"
            host = answer(n).value_counts("V_bp")
            assert host.ids is None and host.as_dict() == dev.as_dict()
            h_ms = timed(lambda: answer(n).value_counts("V_bp"), 1 if n >= 65536 else 3)
            os.environ.pop("DAS_GROUP")
        cross[str(n)] = {"groups": len(dev), "device_ms": d_ms, "host_ms": h_ms}
        print(f"[a] {n} rows: {cross[str(n)]}", file=sys.stderr, flush=True)
    rec["crossover"] = cross
    first = None
    for n in reversed([int(k) for k in cross]):
        c = cross[str(n)]
        if c["host_ms"] is None:
            continue
        if c["device_ms"] > c["host_ms"]:
            break
        first = n
    rec["device_not_slower_from_rows"] = first
    del scan, t

    # (d) the two strategies against each other: uniform keys over a bounded range, few rows and many
    rng = np.random.default_rng(3)
    rec["strategies"] = {}
    for rows in (4096, 1 << 22):
        for bits in (12, 13, 16, 20, 22, 24, 26):
            span = (1 << bits) + (1 if bits == 13 else 0) - (4096 if bits == 13 else 0)    # 13: 4097, one past the LDS tile
            keys = rng.integers(0, span, rows).astype(np.uint32).reshape(1, -1)
            tab = db.ctx.table_from_host(_lib.TABLE_ORDERED, [var], keys)
            tab.set_bounds([0], [span - 1])
            r = {}
            for mode, name in (("1", "direct_ms"), ("0", "sorted_ms")):
                os.environ["DAS_GROUP_DIRECT"] = mode
                got = db.ctx.group_counts([tab], [0], cap=rows)
                assert int(got[1].sum()) == rows
                r[name] = timed(lambda: db.ctx.group_counts([tab], [0], cap=rows), args.reps)
            os.environ.pop("DAS_GROUP_DIRECT")
            rec["strategies"][f"rows_{rows}_range_{span}"] = r
            print(f"[d] {rows} rows, range {span}: {r}", file=sys.stderr, flush=True)
            del tab

    # (b) Q6 by each variable, and the settle it avoids
    print("[b] bio Q6", file=sys.stderr, flush=True)
    q6 = ask(bench, pm, db, specs["Q6"])
    rec["q6"] = {"rows": q6.count(), "tables": len(q6._rel.tables), "by": grouped(db, pm, q6, args.reps)}
    rec["q6"]["settle"] = settle_ms(db, q6, "k_cartesian")
    print(f"  settle: {rec['q6']['settle']}", file=sys.stderr, flush=True)
    del q6, db

    # ---- flybase ---------------------------------------------------------------------------------------
    db = HipDB(device=0)
    db.GROUP_MIN = 0
    db.load_arrays(synthetic.flybase_kb(args.fb_genes, args.fb_schema, args.fb_rows))
    fj = dict((name[:2], q) for name, q in bench.flybase_specs())["FJ"]
    rec["flybase_join"] = {}
    for defer in ("1", "0"):
        os.environ["DAS_DEFER_JOIN"] = defer
        print(f"[c] FlyBase FJ, DAS_DEFER_JOIN={defer}", file=sys.stderr, flush=True)
        ans = ask(bench, pm, db, fj)
        rec["flybase_join"][f"defer_{defer}"] = {"rows": ans.count(), "by": grouped(db, pm, ans, args.reps)}
        if defer == "1":
            rec["flybase_join"]["defer_1"]["settle"] = settle_ms(db, ans, "k_dj_write")
        del ans
    os.environ.pop("DAS_DEFER_JOIN")
    rec["path"] = dict(db.group_stats)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: rec[k] for k in ("device_not_slower_from_rows",)}))


if __name__ == "__main__":
    main()
