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
elapsed / (8 * links).

Third step, the mining loop (cells c34c1d24 / efac9ac6): over the templates of
that sample, 1,000 random 3-grams drawn as the notebook draws them (first
term among the level-0 templates; each other term: a halo level by roulette
over DEPTH_WEIGTH = [1, 1], then a template of that level, drawn again while
that (template, level) is in the combination; fixed seed), count and
I-surprisingness of each: the device path is one
miner.isurprisingness call (das_conjunction_counts: one call for the triples,
one for their merged pairs); the host path is the per-query loop
(miner.conjunction_counts_host, one matched() per triple and per pair) under
the same budget.  The device child also counts a batch of 10^5 random pairs.
The record states launches and read-backs per call.

Fourth step, "exhaustive": the notebook's last cell (efac9ac6) for NGRAM 3
over the same templates -- every level-0 template with every pair of templates
-- as one db.mine call (das_mine_combinations: the pair matrix, the partner
lists, tiles of enumerated triples counted, scored and cut to the best 16).
The baseline is the only way there was before: the host enumerates the same
(unpruned) space and scores it in batches through miner.isurprisingness on
the same HipDB (miner.mine_host; the counting itself is das_conjunction_counts),
under --host-budget; if it does not finish it is extrapolated per row from
the part done, and the record says so.  Both run in the device child.

--steps names the steps to measure (default: all four).  With fewer, the
halo host loop is not run unless asked for, and the steps measured replace
those of the record already at --out, whose other steps stay as they are;
"steps_measured_last" then says which ones the last run wrote.

The device child also times every kernel with the
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
                 "k_pc_templates", "k_pc_flags", "k_pc_emit", "k_pc_resolve", "k_pc_scan", "k_pc_finish",
                 "k_cj_resolve", "k_cj_plan", "k_cj_count", "k_mx_pair_rows", "k_mx_partners", "k_mx_enum",
                 "k_mx_score", "k_mx_emit", "k_mx_keys", "k_mx_take")
MX_TOP, MX_BATCH = 16, 1 << 17
NGRAM, EPOCHS, PAIR_BATCH, MINING_SEED = 3, 1000, 100_000, 20240229
STEPS = ("halo", "counts", "mining", "exhaustive")


def halo_queries(atoms_expanded, links_found):
    return 5 * atoms_expanded + links_found


def draw_ngrams(np, level_rows):
    """Cell c34c1d24's draw over template rows: level_rows[lv] = the rows of
    the templates of halo level lv (a template of both levels is in both).
    The first term is a level-0 row; each other term takes a level by
    roulette over equal weights (build_roulette([1, 1]) = [0.5, 1]), then a
    row of that level, again while (row, level) is in the combination."""
    rng = np.random.default_rng(MINING_SEED)
    roulette = [0.5, 1.0]
    combos = np.empty((EPOCHS, NGRAM), dtype=np.uint32)
    for e in range(EPOCHS):
        picked = [(int(level_rows[0][rng.integers(len(level_rows[0]))]), 0)]
        while len(picked) < NGRAM:
            r = rng.random()
            level = next(lv for lv, w in enumerate(roulette) if r <= w)
            term = (int(level_rows[level][rng.integers(len(level_rows[level]))]), level)
            if term not in picked:
                picked.append(term)
        combos[e] = [row for row, _ in picked]
    return combos


def level_rows(np, db, pc, links_per_level):
    """Per halo level the rows of `pc` that are templates of its links."""
    key = lambda q: list(zip(q.arity.tolist(), q.type_id.tolist(),                          # noqa: E731
                             *(q.targets[:, p].tolist() for p in range(3))))
    at = {k: i for i, k in enumerate(key(pc))}
    return [np.asarray([at[k] for k in key(db.pattern_counts(links))], dtype=np.int64) for links in links_per_level]


def exhaustive_step(args, np, _lib, miner, db, pc, basics, universe, log):
    """db.mine over (basics x pairs of all templates) and its baseline, the
    host enumeration scored through miner.isurprisingness on the same HipDB."""
    db.mine(pc, basics[:1], universe, ngram=2, top=1)                              # first call: allocations
    db.ctx.sync()
    c0 = _lib.counters()
    t0 = time.perf_counter()
    res = db.mine(pc, basics, universe, ngram=NGRAM, top=MX_TOP, max_combinations=2 ** 62)
    t_dev = time.perf_counter() - t0
    c1 = _lib.counters()
    assert db.mine_stats["host"] == 0
    dev = {"ngram": NGRAM, "templates": len(pc), "basics": len(basics), "top": MX_TOP,
           "searched": res.searched, "scored": res.scored, "tiles": res.tiles, "seconds": round(t_dev, 6),
           "us_per_combination_scored": round(1e6 * t_dev / max(res.scored, 1), 5),
           "us_per_combination_searched": round(1e6 * t_dev / max(res.searched, 1), 7),
           "launches": c1[0] - c0[0], "readbacks": c1[1] - c0[1], "rows": len(res),
           "best": {"combo": res.combos[0].tolist(), "count": int(res.count[0]), "value": float(res.value[0])}
           if len(res) else None}
    log(f"exhaustive {dev}")
    t0 = time.perf_counter()
    base = miner.mine_host(db, pc, basics, universe, ngram=NGRAM, top=MX_TOP, max_combinations=2 ** 62,
                           batch=MX_BATCH, budget_s=args.host_budget)
    t_base = time.perf_counter() - t0
    rec = {"how": "miner.mine_host: itertools enumeration of the whole space, miner.isurprisingness "
                  f"(das_conjunction_counts) per batch of {MX_BATCH} rows, on the same HipDB",
           "searched": base.searched, "budget_s": args.host_budget, "seconds_measured": round(t_base, 3),
           "stopped": base.stopped}
    if base.stopped is None:
        assert base.combos.tolist() == res.combos.tolist() and base.value.tolist() == res.value.tolist()
        total = t_base
    else:
        done = max(base.stopped["done"], 1)
        total = t_base * base.stopped["of"] / done
        rec["extrapolated"] = f"{base.stopped['done']} of {base.stopped['of']} rows scored; " \
                              "seconds = measured * of / done"
        rec["us_per_combination_measured"] = round(1e6 * t_base / done, 4)
    rec["seconds"] = round(total, 3)
    log(f"exhaustive baseline {rec}")
    return {"exhaustive": dev, "exhaustive_baseline": rec}


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
        # the mining loop over the sample's templates
        rows = level_rows(np, db, pc, [halo.links[0], halo.links[1][::100]])
        combos = draw_ngrams(np, rows)
        universe = halo.universe_size
        miner.isurprisingness(db, pc, combos[:8], universe)                        # first call: allocations
        db.ctx.sync()
        s0, c3 = dict(db.conjunction_stats), _lib.counters()
        t0 = time.perf_counter()
        res = miner.isurprisingness(db, pc, combos, universe)
        t_is = time.perf_counter() - t0
        c4, s1 = _lib.counters(), dict(db.conjunction_stats)
        pairs = np.random.default_rng(MINING_SEED + 1).integers(len(pc), size=(PAIR_BATCH, 2)).astype(np.uint32)
        t0 = time.perf_counter()
        pair_counts = db.conjunction_counts(pc, pairs)
        t_pairs = time.perf_counter() - t0
        c5 = _lib.counters()
        queries = len(combos) + len(miner.sub_combinations(combos)[2][0])
        out["mining"] = {"ngram": NGRAM, "combinations": len(combos), "templates": len(pc),
                         "templates_per_level": [len(r) for r in rows],
                         "queries": queries, "seconds": round(t_is, 6),
                         "ms_per_query": round(1e3 * t_is / queries, 6),
                         "launches": c4[0] - c3[0], "readbacks": c4[1] - c3[1],
                         "conjunction_calls": 2, "nonzero": int((res.count > 0).sum()),
                         "count_sum": int(res.count.sum()),
                         "best_isurprisingness": float(np.nanmax(res.value)),
                         "on_device": s1["device"] - s0["device"], "on_host": s1["host"] - s0["host"]}
        out["pair_batch"] = {"combinations": PAIR_BATCH, "seconds": round(t_pairs, 6),
                             "us_per_combination": round(1e6 * t_pairs / PAIR_BATCH, 4),
                             "launches": c5[0] - c4[0], "readbacks": c5[1] - c4[1],
                             "nonzero": int((pair_counts > 0).sum()), "count_sum": int(pair_counts.sum())}
        out["mining_combos"] = combos.tolist()
        out["mining_digest"] = [int(res.count.sum()), int((res.count > 0).sum())]
        if "exhaustive" in args.steps:
            out.update(exhaustive_step(args, np, _lib, miner, db, pc, rows[0].tolist(), universe, log))
        # per-kernel times (events) of one more run of the steps
        db.ctx.prof_enable(True)
        db.ctx.prof_reset()
        h2 = db.halo(seed, LENGTH)
        db.pattern_counts(sample)
        db.pattern_counts(h2.level(1))
        miner.isurprisingness(db, pc, combos, universe)
        db.conjunction_counts(pc, pairs)
        db.ctx.sync()
        ks = {}
        for name, st in db.ctx.prof_stats().items():
            if st["launches"] and (name in MINER_KERNELS or name.startswith(("k_scan", "k_radix", "k_gather_u32"))):
                ms = st["ms"]
                ks[name] = {"launches": int(st["launches"]), "ms": round(ms, 4), "bytes": st["bytes"],
                            "hbm_fraction_of_spec": round(st["bytes"] / (ms * 1e-3) / HBM_PEAK_SPEC, 4) if ms else None}
        out["kernels"] = ks
        if "exhaustive" in args.steps:
            # one more db.mine under the events, its kernels apart: it shares the counting kernels with the mining step
            db.ctx.prof_reset()
            db.mine(pc, rows[0].tolist(), universe, ngram=NGRAM, top=MX_TOP, max_combinations=2 ** 62)
            db.ctx.sync()
            mx = {name: {"launches": int(st["launches"]), "ms": round(st["ms"], 4), "bytes": st["bytes"]}
                  for name, st in db.ctx.prof_stats().items() if st["launches"]}
            out["exhaustive"]["kernels"] = mx
            out["exhaustive"]["kernel_ms"] = round(sum(r["ms"] for r in mx.values()), 4)
        db.ctx.prof_enable(False)
    else:
        os.environ["DAS_MINER"] = "0"
        want = json.loads(args.expect)
        t0 = time.perf_counter()
        halo = miner.halo_host(db, seed, LENGTH if "halo" in args.steps else 0, budget_s=args.host_budget)
        t_halo = time.perf_counter() - t0
        sizes = [len(x) for x in halo.links]
        rec = {"seconds_measured": round(t_halo, 3), "links_per_level": sizes, "stopped": halo.stopped}
        if halo.stopped is None:
            assert "halo" not in args.steps or sizes == want["links_per_level"], (sizes, want)
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
        # the mining loop: one matched() per triple and per merged pair
        combos = np.asarray(want["mining_combos"], dtype=np.uint32)
        sub = miner.sub_combinations(combos)[2][0]
        assert not pc.stopped, "the sample's templates are needed whole"
        c0 = _lib.counters()
        t0 = time.perf_counter()
        full = miner.conjunction_counts_host(db, pc, combos, budget_s=args.host_budget)
        t_full = time.perf_counter() - t0
        c1 = _lib.counters()
        done = full.stopped["done"] if full.stopped else len(combos)
        rec = {"combinations": len(combos), "queries": len(combos) + len(sub), "seconds_measured": round(t_full, 3),
               "stopped": full.stopped, "launches_per_query": round((c1[0] - c0[0]) / max(done, 1), 1),
               "readbacks_per_query": round((c1[1] - c0[1]) / max(done, 1), 1)}
        if full.stopped is None:
            assert [int(full.sum()), int((full > 0).sum())] == want["mining_digest"], want["mining_digest"]
            t0 = time.perf_counter()
            part = miner.conjunction_counts_host(db, pc, sub, budget_s=args.host_budget)
            t_sub = time.perf_counter() - t0
            rec["seconds_measured"] = round(t_full + t_sub, 3)
            total = t_full + (t_sub if part.stopped is None else t_sub * part.stopped["of"] / max(part.stopped["done"], 1))
            if part.stopped is not None:
                rec["extrapolated"] = f"every triple counted; {part.stopped['done']} of {part.stopped['of']} pairs " \
                                      "counted, their seconds = measured * of / done"
        else:
            total = t_full * rec["queries"] / max(done, 1)
            rec["extrapolated"] = f"{done} of {len(combos)} triples counted, no pair; seconds = measured * queries / done"
        rec["seconds"] = round(total, 3)
        rec["ms_per_query"] = round(1e3 * total / rec["queries"], 6)
        out["mining"] = rec
        log(f"mining {rec}")
    out["path"] = dict(db.miner_stats)
    out["conjunction_path"] = dict(db.conjunction_stats)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fb-genes", type=int, default=300_000)
    ap.add_argument("--fb-schema", type=int, default=60)
    ap.add_argument("--fb-rows", type=int, default=450_000)
    ap.add_argument("--host-budget", type=float, default=60.0, help="seconds per host step before extrapolating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miner.json"))
    ap.add_argument("--steps", default=",".join(STEPS), help="comma-separated: " + ", ".join(STEPS))
    ap.add_argument("--mode", choices=["device", "host"], help=argparse.SUPPRESS)      # child process
    ap.add_argument("--expect", default="{}", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.steps = [x for x in args.steps.split(",") if x]
    assert args.steps and set(args.steps) <= set(STEPS), args.steps
    if args.mode:
        return child(args)
    rec = {"tool": "tools/miner_bench.py", "kb": "synthetic.flybase_kb", "genes": args.fb_genes,
           "schemas": args.fb_schema, "rows_per_schema": args.fb_rows, "halo_length": LENGTH,
           "seed": "gene g7", "hbm_peak_spec_Bps": HBM_PEAK_SPEC, "host_budget_s": args.host_budget}
    base = [sys.executable, os.path.abspath(__file__), "--fb-genes", str(args.fb_genes), "--fb-schema",
            str(args.fb_schema), "--fb-rows", str(args.fb_rows), "--host-budget", str(args.host_budget),
            "--steps", ",".join(args.steps)]
    env = {k: v for k, v in os.environ.items() if k != "DAS_MINER"}
    r = subprocess.run(base + ["--mode", "device"], env=env, stdout=subprocess.PIPE, text=True, check=True)
    dev = json.loads(r.stdout.strip().splitlines()[-1])
    expect = {"links_per_level": dev["halo"]["links_per_level"], "atoms_expanded": dev["halo"]["atoms_expanded"],
              "sample_ids": dev.pop("sample_ids"), "counts_digest": dev.pop("counts_digest"),
              "mining_combos": dev.pop("mining_combos"), "mining_digest": dev.pop("mining_digest")}
    host_steps = [x for x in args.steps if x != "exhaustive"]          # (its baseline ran in the device child)
    host = {}
    if host_steps:
        r = subprocess.run(base + ["--mode", "host", "--expect", json.dumps(expect)], env=dict(env, DAS_MINER="0"),
                           stdout=subprocess.PIPE, text=True, check=True)
        host = json.loads(r.stdout.strip().splitlines()[-1])
        assert host["conjunction_path"]["device"] == 0
    assert dev["path"]["host"] == 0 and dev["path"]["device"] > 0
    assert dev["mining"]["on_device"] > 0
    if set(args.steps) != set(STEPS) and os.path.exists(args.out):
        # only the steps asked for are taken from this run; the record's other steps stay
        with open(args.out) as f:
            old = json.load(f)
        same_kb = all(old.get(k) == rec[k] for k in ("kb", "genes", "schemas", "rows_per_schema", "halo_length", "seed"))
        assert same_kb, "the record at --out is of another KB: measure all steps"
        keep = {"halo": ("halo",), "counts": ("counts", "counts_whole_level_1"),
                "mining": ("mining", "pair_batch", "conjunction_path"),
                "exhaustive": ("exhaustive", "exhaustive_baseline")}
        names = {"halo": ("k_halo", "k_bits"), "counts": ("k_pc_",), "mining": ("k_cj_",), "exhaustive": ("k_mx_",)}
        for side, new in (("device", dev), ("host", host)):
            for step in args.steps:
                for k in keep[step]:
                    if k in new:
                        old[side][k] = new[k]
        for name, row in dev["kernels"].items():
            if name.startswith(tuple(p for step in args.steps for p in names[step])):
                old["device"]["kernels"][name] = row
        dev, host, rec = old["device"], old["host"], old
    rec["steps_measured_last"] = args.steps
    rec["device"], rec["host"] = dev, host
    if "exhaustive" in args.steps:
        d, h = dev["exhaustive"], dev["exhaustive_baseline"]
        print(f"exhaustive: device {d['seconds']} s ({d['scored']} of {d['searched']} combinations scored, "
              f"{d['tiles']} tiles), host enumeration {h['seconds']} s{', extrapolated' if 'extrapolated' in h else ''}")
    for step in host_steps:
        d, h = dev[step], host[step]
        print(f"{step}: device {d['seconds']} s ({d['ms_per_query']} ms/query), host {h['seconds']} s "
              f"({h['ms_per_query']} ms/query{', extrapolated' if 'extrapolated' in h else ''})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
