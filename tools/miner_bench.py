"""SimplePatternMiner's halo walk and template counts: the device path
(das_halo_expand / das_pattern_counts, miner.hip) against the per-call host
loops (DAS_MINER=0: miner.halo_host / miner.pattern_counts_host, what a
caller ran before) on the bench's FlyBase-shaped KB.

Seed: one gene node, as the notebook.  Halo at length 2, then pattern_counts
over level 0 plus every 100th link (1 %) of level 1.  Each path runs in a
fresh child process on its own HipDB.  The host loops get a time budget
(--host-budget seconds per step); a step that does not finish is extrapolated
per link from the part it did (the record says so: "extrapolated").  The
notebook's own figures: halo ms/query = elapsed / sum over templates of
(links + 1), here 5 per expanded atom + the links found; counts ms/query =
elapsed / (8 * links).  The device child also times every kernel with the
library's events and reports its algorithmic bytes against the HBM peak, and
the launches and read-backs per level from das_counters.  GPU box:

    python tools/miner_bench.py [--fb-genes 300000] [--out profiles/miner.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_SPEC = 8.0e12          # bytes/s, MI355X HBM3E (spec)
LENGTH = 2
MINER_KERNELS = ("k_halo_seed_bits", "k_halo_mark_links", "k_halo_mark_targets", "k_bits_count", "k_bits_emit",
                 "k_pc_templates", "k_pc_flags", "k_pc_emit", "k_pc_resolve", "k_pc_scan", "k_pc_finish")


def halo_queries(atoms_expanded, links_found):
    return 5 * atoms_expanded + links_found


def child(args):
    import numpy as np
    from das_amd import _lib, miner, synthetic
    from das_amd.database.hip_db import HipDB
    from das_amd.expression_hasher import ExpressionHasher as EH
    db = HipDB(device=0)
    t0 = time.perf_counter()
    arrays = synthetic.flybase_kb(args.fb_genes, args.fb_schema, args.fb_rows)
    db.load_arrays(arrays)
    db.ctx.sync()
    out = {"mode": args.mode, "links": int(arrays.n_expr), "load_s": round(time.perf_counter() - t0, 3)}
    seed = [EH.terminal_hash("gene", f"g{7 % args.fb_genes}")]
    warm = [EH.terminal_hash("gene", f"g{7926 % args.fb_genes}")]
    log = lambda m: print(f"[{args.mode}] {m}", file=sys.stderr, flush=True)      # noqa: E731
    if args.mode == "device":
        wh = db.halo(warm, LENGTH)                                                 # first call: allocations
        db.pattern_counts(wh.level(0))
        db.ctx.sync()
        c0 = _lib.counters()
        t0 = time.perf_counter()
        halo = db.halo(seed, LENGTH)
        sizes = [len(halo.level(lv)) for lv in range(LENGTH)]
        db.ctx.sync()
        t_halo = time.perf_counter() - t0
        c1 = _lib.counters()
        sample = np.concatenate([halo.links[0], halo.links[1][::100]])
        t0 = time.perf_counter()
        pc = db.pattern_counts(sample)
        t_pc = time.perf_counter() - t0
        c2 = _lib.counters()
        t0 = time.perf_counter()
        pc_all = db.pattern_counts(halo.level(1))                                  # a whole level, read in place
        t_all = time.perf_counter() - t0
        expanded = [len(seed)] + [len(halo.atoms[lv]) for lv in range(LENGTH - 1)]
        out.update(
            halo={"seconds": round(t_halo, 6), "links_per_level": sizes, "atoms_expanded": expanded,
                  "universe_size": halo.universe_size,
                  "ms_per_query": round(1e3 * t_halo / halo_queries(sum(expanded), sum(sizes)), 6),
                  # the whole call, seed step included (two fills, the seeds' bits, one
                  # compaction, one read-back), over the number of levels
                  "launches": c1[0] - c0[0], "readbacks": c1[1] - c0[1],
                  "launches_per_level": round((c1[0] - c0[0]) / LENGTH, 1),
                  "readbacks_per_level": round((c1[1] - c0[1]) / LENGTH, 1)},
            counts={"seconds": round(t_pc, 6), "links": int(sample.size), "templates": len(pc),
                    "matched": int(pc.count.sum()), "ms_per_query": round(1e3 * t_pc / (8 * max(sample.size, 1)), 6),
                    "launches": c2[0] - c1[0], "readbacks": c2[1] - c1[1]},
            counts_whole_level_1={"seconds": round(t_all, 6), "links": sizes[1], "templates": len(pc_all)})
        out["sample_ids"] = sample.tolist()
        out["counts_digest"] = [len(pc), int(pc.count.sum())]
        # per-kernel times (events) of one more run of both steps
        db.ctx.prof_enable(True)
        db.ctx.prof_reset()
        h2 = db.halo(seed, LENGTH)
        db.pattern_counts(sample)
        db.pattern_counts(h2.level(1))
        db.ctx.sync()
        ks = {}
        for name, st in db.ctx.prof_stats().items():
            if st["launches"] and (name in MINER_KERNELS or name.startswith(("k_scan", "k_radix", "k_gather_u32"))):
                ms = st["ms"]
                ks[name] = {"launches": int(st["launches"]), "ms": round(ms, 4), "bytes": st["bytes"],
                            "hbm_fraction_of_spec": round(st["bytes"] / (ms * 1e-3) / HBM_PEAK_SPEC, 4) if ms else None}
        out["kernels"] = ks
        db.ctx.prof_enable(False)
    else:
        os.environ["DAS_MINER"] = "0"
        want = json.loads(args.expect)
        t0 = time.perf_counter()
        halo = miner.halo_host(db, seed, LENGTH, budget_s=args.host_budget)
        t_halo = time.perf_counter() - t0
        sizes = [len(x) for x in halo.links]
        rec = {"seconds_measured": round(t_halo, 3), "links_per_level": sizes, "stopped": halo.stopped}
        if halo.stopped is None:
            assert sizes == want["links_per_level"], (sizes, want)
            total = t_halo
        else:
            # the part done, scaled to the whole of the step it stopped in (the
            # get_link_targets calls of the level's links, or the probes of its atoms)
            st = halo.stopped
            total = t_halo * max(st["of"], 1) / max(st["done"], 1)
            rec["extrapolated"] = f"stopped in level {st['level']} {st['phase']} after {st['done']} of {st['of']}; " \
                                  "seconds = measured * of / done (later steps not counted: a lower bound)"
        rec["seconds"] = round(total, 3)
        rec["ms_per_query"] = round(1e3 * total / halo_queries(sum(want["atoms_expanded"]),
                                                               sum(want["links_per_level"])), 6)
        out["halo"] = rec
        log(f"halo {rec}")
        sample = np.asarray(want["sample_ids"], dtype=np.uint32)
        t0 = time.perf_counter()
        pc = miner.pattern_counts_host(db, sample, budget_s=args.host_budget)
        t_pc = time.perf_counter() - t0
        rec = {"seconds_measured": round(t_pc, 3), "links": int(sample.size), "stopped": pc.stopped}
        if pc.stopped is None:
            assert [len(pc), int(pc.count.sum())] == want["counts_digest"], (len(pc), want["counts_digest"])
            total = t_pc
        else:
            total = t_pc * pc.stopped["of"] / max(pc.stopped["done"], 1)
            rec["extrapolated"] = f"{pc.stopped['done']} of {pc.stopped['of']} links counted; seconds = measured * of / done"
        rec["seconds"] = round(total, 3)
        rec["ms_per_query"] = round(1e3 * total / (8 * max(sample.size, 1)), 6)
        out["counts"] = rec
        log(f"counts {rec}")
    out["path"] = dict(db.miner_stats)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fb-genes", type=int, default=300_000)
    ap.add_argument("--fb-schema", type=int, default=60)
    ap.add_argument("--fb-rows", type=int, default=450_000)
    ap.add_argument("--host-budget", type=float, default=60.0, help="seconds per host step before extrapolating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miner.json"))
    ap.add_argument("--mode", choices=["device", "host"], help=argparse.SUPPRESS)      # child process
    ap.add_argument("--expect", default="{}", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.mode:
        return child(args)
    rec = {"tool": "tools/miner_bench.py", "kb": "synthetic.flybase_kb", "genes": args.fb_genes,
           "schemas": args.fb_schema, "rows_per_schema": args.fb_rows, "halo_length": LENGTH,
           "seed": "gene g7", "hbm_peak_spec_Bps": HBM_PEAK_SPEC, "host_budget_s": args.host_budget}
    base = [sys.executable, os.path.abspath(__file__), "--fb-genes", str(args.fb_genes), "--fb-schema",
            str(args.fb_schema), "--fb-rows", str(args.fb_rows), "--host-budget", str(args.host_budget)]
    env = {k: v for k, v in os.environ.items() if k != "DAS_MINER"}
    r = subprocess.run(base + ["--mode", "device"], env=env, stdout=subprocess.PIPE, text=True, check=True)
    dev = json.loads(r.stdout.strip().splitlines()[-1])
    expect = {"links_per_level": dev["halo"]["links_per_level"], "atoms_expanded": dev["halo"]["atoms_expanded"],
              "sample_ids": dev.pop("sample_ids"), "counts_digest": dev.pop("counts_digest")}
    r = subprocess.run(base + ["--mode", "host", "--expect", json.dumps(expect)], env=dict(env, DAS_MINER="0"),
                       stdout=subprocess.PIPE, text=True, check=True)
    host = json.loads(r.stdout.strip().splitlines()[-1])
    assert dev["path"]["host"] == 0 and dev["path"]["device"] > 0
    rec["device"], rec["host"] = dev, host
    for step in ("halo", "counts"):
        d, h = dev[step], host[step]
        print(f"{step}: device {d['seconds']} s ({d['ms_per_query']} ms/query), host {h['seconds']} s "
              f"({h['ms_per_query']} ms/query{', extrapolated' if 'extrapolated' in h else ''})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
