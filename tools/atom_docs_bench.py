"""ATOM_INFO / JSON outputs in bulk: the device calls (das_atoms_json renders
the text, das_links_outgoing feeds the documents; docs.hip) against the
per-atom host walk they replace (DAS_ATOM_DOCS=0: the parent commit's
get_atom_as_deep_representation / get_atom_as_dict per handle) on the
FlyBase-shaped KB of the bench.

Each path runs in a fresh child process and is forced (ATOM_DOCS_MIN* = 0 on
the device, DAS_ATOM_DOCS=0 on the host), so the figures do not depend on
where HipDB switches between them.  Workloads, each as JSON and as ATOM_INFO:
the links of get_links('Execution', targets=[schema, '*', '*']) for one schema
node, one node alone, and random link sets of 1 .. 10^5.  The figure is the
median wall time of the calls after a first one, which is checked against the
host walk (the whole text up to 1000 links, 64 sampled documents above).  The host child
measures twice, as loaded and after prefetch(), under a time budget per
workload: where the walk does not finish, the rows done and their time are
reported and the total is marked extrapolated.  The device child then times
the kernels alone with the library's per-kernel events, in a pass of their
own, and reports the write kernels' text bytes against the box's 16-byte
store ceiling (das_box_store_bw).  GPU box:

    python tools/atom_docs_bench.py [--fb-genes 300000] [--out profiles/atom_docs.json]
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

SIZES = [1, 2, 4, 8, 16, 64, 1000, 100_000]
SCHEMA = "Schema:gene_uniquename"
CHUNK = 256                     # handles per call of the budgeted host walk
KERNELS = "doc_arity_scan|k_doc_expand|k_doc_measure|doc_root_scan|k_doc_roots|k_doc_write"


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
    from das_amd import synthetic
    from das_amd.database.hip_db import HipDB
    from das_amd.distributed_atom_space import DistributedAtomSpace, QueryOutputFormat as F
    db = HipDB(device=0)
    db.ATOM_DOCS_MIN = db.ATOM_DOCS_MIN_PREFETCHED = db.ATOM_DOCS_MIN_NODES = 0
    t0 = time.perf_counter()
    arrays = synthetic.flybase_kb(args.fb_genes, args.fb_schema, args.fb_rows)
    db.load_arrays(arrays)
    db.ctx.sync()
    out = {"mode": args.mode, "links": int(arrays.n_expr), "load_s": round(time.perf_counter() - t0, 3)}
    print(f"[{args.mode}] loaded {out['links']} links in {out['load_s']} s", file=sys.stderr, flush=True)
    das = DistributedAtomSpace(db=db)
    schema = das.get_node("Schema", SCHEMA)
    t0 = time.perf_counter()
    rows = das.get_links("Execution", targets=[schema, "*", "*"])
    out["schema_rows"] = len(rows)
    out["schema_match_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    # random link sets: random atom ids that are links
    rng = np.random.default_rng(1)
    n_atoms = int(db.ctx.stats().n_atoms)
    cand = rng.integers(0, n_atoms, 8 * max(SIZES)).astype(np.uint32)
    cand = cand[db.ctx.atoms_info(cand)[1] == 2]
    assert cand.size >= max(SIZES)
    picks = {n: db.hex_of(cand[:n]) for n in SIZES}
    # (one node alone: the walk's cheapest case, one device round trip)
    workloads = [("schema", rows), ("node", [das.get_node("Verbatim", "FBgn0000003")])] + \
        [(str(n), picks[n]) for n in SIZES]

    def check(handles, text, infos):
        k = list(range(len(handles))) if len(handles) <= 1000 else rng.integers(0, len(handles), 64).tolist()
        if len(handles) <= 1000:
            assert text == db.atoms_json_host(handles)
        else:
            docs = json.loads(text)
            assert len(docs) == len(handles)
            for i in k:
                assert docs[i] == db.get_atom_as_deep_representation(handles[i])
        assert len(infos) == len(handles)
        for i in k[:64]:
            assert infos[i] == db.get_atom_as_dict(handles[i])

    def walk(fn, handles, budget):
        """The host walk in chunks under a time budget: (rows done, seconds)."""
        t0, done = time.perf_counter(), 0
        while done < len(handles) and time.perf_counter() - t0 < budget:
            fn(handles[done:done + CHUNK])
            done += CHUNK
        return min(done, len(handles)), time.perf_counter() - t0

    if args.mode == "device":
        rec = {}
        for name, handles in workloads:
            text, infos = db.atoms_json(handles), db.get_atoms_as_dicts(handles)
            check(handles, text, infos)
            reps = args.reps if len(handles) <= 1000 else 3
            rec[name] = {"rows": len(handles), "text_bytes": len(text), "reps": reps,
                         "json_ms": timed(lambda: db.atoms_json(handles), reps),
                         "atom_info_ms": timed(lambda: db.get_atoms_as_dicts(handles), reps)}
            print(f"[device] {name}: {rec[name]}", file=sys.stderr, flush=True)
        rec["schema"]["facade_json_ms"] = timed(
            lambda: das.get_links("Execution", targets=[schema, "*", "*"], output_format=F.JSON), 3)
        rec["schema"]["facade_atom_info_ms"] = timed(
            lambda: das.get_links("Execution", targets=[schema, "*", "*"], output_format=F.ATOM_INFO), 3)
        out["calls"] = rec
        # kernel times: HIP events, a pass of their own (the C call alone: no handle resolution, no decode)
        out["store16_nt_GBps"] = round(db.ctx.box_store_bw(), 1)
        tj, toff = db._type_json_texts()
        db.ctx.prof_enable(True)
        db.ctx.prof_only(KERNELS)
        out["kernels"] = {}
        for name, handles in workloads:
            if len(handles) < 1000:
                continue
            ids = db.ids_of(handles).astype(np.uint32)
            buf = np.empty(rec[name]["text_bytes"], dtype=np.uint8)
            db.ctx.atoms_json(tj, toff, ids=ids, out=buf)
            db.ctx.prof_reset()
            t_call = timed(lambda: db.ctx.atoms_json(tj, toff, ids=ids, out=buf), args.reps)
            st = db.ctx.prof_stats()
            per = {k: round(v["ms"] / args.reps, 5) for k, v in st.items()}
            write_ms = st["k_doc_write"]["ms"] / args.reps
            out["kernels"][name] = {
                "text_bytes": rec[name]["text_bytes"], "c_call_ms": t_call, "kernel_ms_per_call": per,
                # the rest of HipDB.atoms_json: handles to ids (cached after the first call), bytes to str
                "ids_of_ms": timed(lambda: db.ids_of(handles), 3),
                "decode_ms": timed(lambda: str(buf.data, "ascii"), 3),
                "launches_per_call": sum(v["launches"] for v in st.values()) / args.reps,
                "write_ms": round(write_ms, 5),
                "write_GBps": round(rec[name]["text_bytes"] / (write_ms * 1e-3) / 1e9, 2)}
            print(f"[device] kernels {name}: {out['kernels'][name]}", file=sys.stderr, flush=True)
        db.ctx.prof_enable(False)
    else:
        def measure():
            rec = {}
            for name, handles in workloads:
                r = {"rows": len(handles)}
                for what, fn in (("json", db.atoms_json), ("atom_info", db.get_atoms_as_dicts)):
                    done, secs = walk(fn, handles, args.host_budget)
                    r[what] = {"rows_done": done, "seconds": round(secs, 4), "extrapolated": done < len(handles),
                               "total_ms": round(secs / max(done, 1) * len(handles) * 1e3, 4)}
                    if done == len(handles) and secs < 1.0:      # short enough to repeat: the median of whole calls
                        r[what]["total_ms"] = timed(lambda: fn(handles), 5)
                rec[name] = r
                print(f"[host] {name}: {r}", file=sys.stderr, flush=True)
            return rec
        out["as_loaded"] = measure()
        t0 = time.perf_counter()
        db.prefetch()
        out["prefetch_s"] = round(time.perf_counter() - t0, 3)
        out["prefetched"] = measure()
    out["path"] = dict(db.atom_docs_stats)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fb-genes", type=int, default=300_000)
    ap.add_argument("--fb-schema", type=int, default=60)
    ap.add_argument("--fb-rows", type=int, default=450_000)
    ap.add_argument("--reps", type=int, default=9, help="timed calls per workload on the device path")
    ap.add_argument("--host-budget", type=float, default=60.0,
                    help="seconds the host walk gets per workload, format and flavour")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atom_docs.json"))
    ap.add_argument("--mode", choices=["device", "host"], help=argparse.SUPPRESS)      # child process
    args = ap.parse_args()
    if args.mode:
        return child(args)
    rec = {"tool": "tools/atom_docs_bench.py", "sizes": SIZES, "schema": SCHEMA, "host_budget_s": args.host_budget,
           "kb": f"flybase_kb({args.fb_genes}, {args.fb_schema}, {args.fb_rows})"}
    for mode in ("device", "host"):
        env = dict(os.environ, DAS_ATOM_DOCS="1" if mode == "device" else "0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--fb-genes", str(args.fb_genes),
                            "--fb-schema", str(args.fb_schema), "--fb-rows", str(args.fb_rows), "--reps",
                            str(args.reps), "--host-budget", str(args.host_budget)], env=env,
                           stdout=subprocess.PIPE, text=True, check=True)
        rec[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec[mode]["path"][mode] > 0 and rec[mode]["path"]["host" if mode == "device" else "device"] == 0
    # the smallest size from which the device call is never slower than the host walk, either format
    for flavour in ("as_loaded", "prefetched"):
        cross = None
        for n in reversed(SIZES):
            d, h = rec["device"]["calls"][str(n)], rec["host"][flavour][str(n)]
            if d["json_ms"] > h["json"]["total_ms"] or d["atom_info_ms"] > h["atom_info"]["total_ms"]:
                break
            cross = n
        rec[f"device_not_slower_from_{flavour}"] = cross
    for name in ["schema", "node"] + [str(n) for n in SIZES]:
        d = rec["device"]["calls"][name]
        for what, key in (("JSON", "json"), ("ATOM_INFO", "atom_info")):
            h0, h1 = rec["host"]["as_loaded"][name][key], rec["host"]["prefetched"][name][key]
            print(f"{name} ({d['rows']} atoms) {what}: device {d[key + '_ms']} ms; host walk {h0['total_ms']} ms as "
                  f"loaded{' (extrapolated)' if h0['extrapolated'] else ''}, {h1['total_ms']} ms prefetched"
                  f"{' (extrapolated)' if h1['extrapolated'] else ''}")
    for name, k in rec["device"]["kernels"].items():
        print(f"{name}: write kernels {k['write_ms']} ms for {k['text_bytes']} text bytes = {k['write_GBps']} GB/s "
              f"(16-byte store ceiling {rec['device']['store16_nt_GBps']} GB/s); C call {k['c_call_ms']} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
