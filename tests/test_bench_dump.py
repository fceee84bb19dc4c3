"""bench.py's plain / --full split and --dump-outputs: a plain run switches
off everything beside the headline's timed steps; the dump of a step's
answers is the same from run to run, holds the oracle's rows (as the leading
48 bits of each handle, sorted) and the order-independent checksum of the
whole answer, and a sampled table keeps a fixed subset of its rows."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1")
    assert not a.full and a.no_cpu_baseline and a.no_materialise and a.no_extras
    assert a.detail is None and a.dump_outputs is None
    assert (a.steps, a.warmup, a.workload) == (3, 1, "all")


def test_full_run_keeps_every_measurement(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--full")
    assert a.full and not (a.no_cpu_baseline or a.no_materialise or a.no_extras)
    assert a.detail.endswith("bench_detail.json")
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--detail", "x.json", "--dump-outputs", "d")
    assert a.no_cpu_baseline and not a.no_extras and a.detail == "x.json" and a.dump_outputs == "d"


def test_dump_outputs_is_for_query_workloads(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--workload", "build", "--dump-outputs", "d")


@pytest.mark.gpu
def test_dump_outputs_holds_the_oracles_rows(golden, tmp_path, monkeypatch):
    from das_amd import loader
    from das_amd.database.hip_db import HipDB
    from das_amd.pattern_matcher import pattern_matcher as pm
    from oracle import das_oracle as O
    from tests import checksum as CK
    d = golden("kb_animals.json")
    db = HipDB(device=0)
    db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    inh = lambda a, b: bench._L("Inheritance", bench._V(a), bench._V(b))  # noqa: E731
    specs = [("one link", inh("V2", "V1")), ("two hops", ["And", [inh("V1", "V2"), inh("V2", "V3")]])]
    names = [n for n, _ in specs]

    def run(sub):
        answers = []
        for _, s in specs:
            ans = pm.PatternMatchingAnswer()
            assert bench.build_expr(pm, s).matched(db, ans)
            answers.append(ans)
        bench.dump_outputs(str(tmp_path / sub), db, pm, names, [a.count() for a in answers], answers)
        with open(tmp_path / sub / "index.json") as f:
            index = json.load(f)
        files = sorted(f[:-4] for f in os.listdir(tmp_path / sub) if f.endswith(".npy"))
        assert files == sorted(index)
        return {f: np.load(tmp_path / sub / (f + ".npy")) for f in files}, index

    def same(x, y):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k].dtype == np.float64 and np.array_equal(x[k], y[k]), k

    a, index = run("a")
    same(a, run("b")[0])
    odb = O.RedisMongoSemantics(O.KB.from_tables(d["nodes"], d["links"]))
    for q, (name, spec) in enumerate(specs):
        maps = [dict((v, h) for v, h in r[1]) for r in O.evaluate(spec, odb)["rows"]]
        assert len(maps) > 4 and a["counts"][q] == len(maps)
        cols = sorted(maps[0])
        assert index[f"q{q}_rows0"]["columns"] == cols and index[f"q{q}_rows0"]["sample"] == "every row"
        want = sorted([float(int(m[v][:12], 16)) for v in cols] for m in maps)
        assert a[f"q{q}_rows0"].tolist() == want
        ck = CK.rows_checksum(maps)
        assert a[f"q{q}_checksum"].tolist() == [float((ck >> (16 * i)) & 0xFFFF) for i in range(4)]
    # a table above DUMP_SAMPLE_ROWS: a fixed subset of its rows, the checksum still of the whole answer
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 2)
    c, cindex = run("c")
    same(c, run("d")[0])
    for q in range(len(specs)):
        full = {tuple(r) for r in a[f"q{q}_rows0"].tolist()}
        kept = [tuple(r) for r in c[f"q{q}_rows0"].tolist()]
        assert kept == sorted(kept) and set(kept) <= full and len(kept) < len(full)
        assert cindex[f"q{q}_rows0"]["sample"].startswith("1 row in ")
        assert np.array_equal(c[f"q{q}_checksum"], a[f"q{q}_checksum"]) and c["counts"][q] == a["counts"][q]
