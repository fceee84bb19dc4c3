"""das.query()'s text: the device call (das_table_rows_text, rows_text.hip)
against the path it replaces, on the bench's bio KB.

(a) crossover: das.query() wall time on answers of 1 .. 2^22 rows -- the first
    rows of the Member scan as a two-variable answer, and the same rows bound
    to six variables -- through the device path and through DAS_QUERY_TEXT=0
    (the parent commit's path: fetch, handle strings, a set of Assignment
    objects, repr of each), in the same process.  Per size: the median of the
    repeated calls after a first one, and the host path's fastest and slowest
    call (its run-to-run spread); the smallest size from which the device path
    was never slower than the host path's fastest call.
(b) bio Q6 (bench.py's QUERY_3, a deferred cross product) streamed by
    answer.iter_text at a fixed chunk size: the first chunks, rows and bytes
    per second, no k_cartesian launch.
(c) the kernel alone: k_rows_text's recorded time and algorithmic bytes on
    the 2^22-row answers, beside the card's 16-byte store ceiling
    (das_box_store_bw).

GPU box:

    python tools/query_text_bench.py [--out profiles/query_text.json]
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [4 ** k for k in range(12)]          # 1 .. 2^22


def times(fn, reps):
    """Wall times in ms of `reps` calls (the caller has made a first one)."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genes", type=int, default=200_000)
    ap.add_argument("--bps", type=int, default=50_000)
    ap.add_argument("--members", type=int, default=20_000_000)
    ap.add_argument("--inheritance", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=SIZES[-1], help="largest answer the host path is timed on")
    ap.add_argument("--chunk-rows", type=int, default=1 << 20)
    ap.add_argument("--chunks", type=int, default=16, help="chunks of Q6 that (b) streams")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_text.json"))
    args = ap.parse_args()

    import numpy as np
    import bench
    from das_amd import _lib, synthetic
    from das_amd.database.hip_db import HipDB, Relation
    from das_amd.distributed_atom_space import DistributedAtomSpace
    from das_amd.pattern_matcher import pattern_matcher as pm

    class Rows(pm.LogicalExpression):
        """A query whose answer is the given device tables."""

        def __init__(self, tables):
            self.tables = tables

        def matched(self, db, answer):
            answer._set(db, Relation(self.tables))
            return True

    rec = {"tool": "tools/query_text_bench.py", "reps": args.reps,
           "bio": {"genes": args.genes, "bps": args.bps, "members": args.members, "inheritance": args.inheritance}}
    for k in ("DAS_QUERY_TEXT", "DAS_DEFER_JOIN", "DAS_DEFER_PRODUCT"):
        os.environ.pop(k, None)

    db = HipDB(device=0)
    db.QUERY_TEXT_MIN = 0
    db.load_arrays(synthetic.bio_full_kb(args.genes, args.bps, args.members, args.inheritance))
    das = DistributedAtomSpace(db=db)
    specs = dict((name[:2], q) for name, q in bench.bio_specs(np.arange(args.genes)))

    # (a) the crossover, on the first rows of the Member scan
    scan = pm.PatternMatchingAnswer()
    assert bench.build_expr(pm, specs["Q1"]).matched(db, scan)
    t, = scan._rel.tables
    rows2 = t.fetch(0, SIZES[-1])
    sizes = [n for n in SIZES if n <= rows2.shape[1]]
    shapes = {"two_variables": (sorted(t.vars), [0, 1]),
              "six_variables": (sorted(pm._vid(f"V_{i}") for i in range(6)), [0, 1, 0, 1, 0, 1])}
    del scan, t
    rec["crossover"], rec["device_not_slower_from_rows"] = {}, {}
    for shape, (var_ids, src) in shapes.items():
        cross = {}
        for n in sizes:
            cols = np.ascontiguousarray(rows2[src, :n])
            query = Rows([db.ctx.table_from_host(_lib.TABLE_ORDERED, var_ids, cols)])
            os.environ.pop("DAS_QUERY_TEXT", None)
            before = dict(db.query_text_stats)
            dev = das.query(query)
            assert db.query_text_stats["device"] == before["device"] + 1
            d = times(lambda: das.query(query), args.reps if n <= 1 << 20 else 3)
            c = {"bytes": len(dev), "device_ms": round(statistics.median(d), 4)}
            if n <= args.host_max:
                os.environ["DAS_QUERY_TEXT"] = "0"
                host = das.query(query)
                assert len(host) == len(dev) and (n > 1 or host == dev)
                h = times(lambda: das.query(query), 5 if n <= 4096 else 3 if n <= 65536 else 1)
                c.update(host_ms=round(statistics.median(h), 4), host_ms_min=round(min(h), 4),
                         host_ms_max=round(max(h), 4))
                os.environ.pop("DAS_QUERY_TEXT")
                del host
            del dev
            cross[str(n)] = c
            print(f"[a] {shape} {n} rows: {c}", file=sys.stderr, flush=True)
        rec["crossover"][shape] = cross
        first = None
        for n in reversed(sizes):
            c = cross[str(n)]
            if "host_ms" not in c:
                continue
            if c["device_ms"] > c["host_ms_min"]:
                break
            first = n
        rec["device_not_slower_from_rows"][shape] = first

    # (c) the kernel alone, beside the card's store ceiling
    rec["store_ceiling_gbps"] = round(db.ctx.box_store_bw(), 1)
    rec["kernel"] = {}
    n = sizes[-1]
    for shape, (var_ids, src) in shapes.items():
        tab = db.ctx.table_from_host(_lib.TABLE_ORDERED, var_ids, np.ascontiguousarray(rows2[src, :n]))
        lits = pm.row_literals(pm._var_name(v) for v in var_ids)
        out = np.empty(_lib.rows_text_size(lits, pm.ROW_SEP, n), dtype=np.uint8)
        db.ctx.rows_text(tab, lits, pm.ROW_SEP, out=out)
        db.ctx.prof_enable(True)
        db.ctx.prof_reset()
        wall = times(lambda: db.ctx.rows_text(tab, lits, pm.ROW_SEP, out=out), args.reps)
        db.ctx.sync()
        st = {k: v for k, v in db.ctx.prof_stats().items() if k.startswith("k_rows_text")}
        db.ctx.prof_enable(False)
        db.ctx.prof_reset()
        launches = max(sum(v["launches"] for v in st.values()), 1)
        ms = sum(v["ms"] for v in st.values()) / launches
        nbytes = sum(v["bytes"] for v in st.values()) / launches
        k = {"rows": n, "text_bytes": int(out.size), "algorithmic_bytes": nbytes, "kernel_ms": round(ms, 4),
             "gbps": round(nbytes / ms / 1e6, 1) if ms else None, "call_ms": round(statistics.median(wall), 3)}
        k["share_of_store_ceiling"] = round(k["gbps"] / rec["store_ceiling_gbps"], 3) if ms else None
        rec["kernel"][shape] = k
        print(f"[c] {shape}: {k}", file=sys.stderr, flush=True)
        del tab, out
    del rows2

    # (b) Q6 streamed: a deferred product, never written
    q6 = pm.PatternMatchingAnswer()
    assert bench.build_expr(pm, specs["Q6"]).matched(db, q6)
    db.ctx.prof_enable(True)
    db.ctx.prof_reset()
    t0 = time.perf_counter()
    got_bytes = got_pieces = 0
    for piece in itertools.islice(q6.iter_text(chunk_rows=args.chunk_rows), args.chunks + 1):
        got_bytes += len(piece)
        got_pieces += 1
    wall = time.perf_counter() - t0
    db.ctx.sync()
    st = db.ctx.prof_stats()
    db.ctx.prof_enable(False)
    rows = min(q6.count(), (got_pieces - 1) * args.chunk_rows)
    rec["q6_iter_text"] = {
        "rows_of_answer": q6.count(), "tables": len(q6._rel.tables), "chunk_rows": args.chunk_rows,
        "chunks": got_pieces - 1, "rows": rows, "characters": got_bytes, "wall_ms": round(wall * 1e3, 2),
        "rows_per_s": round(rows / wall), "characters_per_s": round(got_bytes / wall),
        "k_cartesian_launches": sum(v["launches"] for k, v in st.items() if k.startswith("k_cartesian")),
        "k_rows_text_launches": sum(v["launches"] for k, v in st.items() if k.startswith("k_rows_text"))}
    print(f"[b] {rec['q6_iter_text']}", file=sys.stderr, flush=True)
    rec["path"] = dict(db.query_text_stats)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: rec[k] for k in ("device_not_slower_from_rows", "store_ceiling_gbps")}))


if __name__ == "__main__":
    main()
