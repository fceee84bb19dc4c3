"""The exhaustive cell of notebooks/SimplePatternMiner.ipynb (efac9ac6) as
one call, host side: miner.mine_host against a literal restatement of the
cell with every count asked of the oracle, the argument checks, and the
64-bit unranking the device enumeration uses (das_amd/csrc/mx_unrank.h, built
into a stand-alone host program).  No GPU."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bench
from das_amd import miner
from das_amd.database.db_interface import UNORDERED_LINK_TYPES, WILDCARD
from oracle import das_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def test_unranking_header_on_the_host(tmp_path):
    """unrank(rank(i, j, s), s) == (i, j): every pair of s in {2, 3, 4, 65,
    1000}; the first and last rank of every row of s in {2^16 + 1, 2^31 - 1,
    2^32 - 1} (ranks beyond 2^53: the floating seed alone is wrong there)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "mx_unrank_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Werror", "-o", exe,
                    os.path.join(HERE, "native", "mx_unrank_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    small = sum(s * (s - 1) // 2 for s in (2, 3, 4, 65, 1000))
    large = sum(2 * (s - 1) for s in (2 ** 16 + 1, 2 ** 31 - 1, 2 ** 32 - 1))
    assert r.stdout.split() == ["ok", str(small + large)]


# ---------------------------------------------------------------------------
# the animals fixture over the oracle
# ---------------------------------------------------------------------------

class OracleMinerDB(bench.OracleFacade):
    """The oracle facade with the one bulk call miner.isurprisingness looks
    for: compute_count of each combination, asked of the oracle's And (the
    package's own patterns evaluate on a HipDB only)."""

    def __init__(self, odb, kb):
        super().__init__(odb)
        self.kb = kb
        self.calls = 0

    def conjunction_counts(self, pc, combos):
        self.calls += 1
        out = []
        for combo in miner.check_combos(combos, len(pc)).tolist():
            expr = _spec(self.kb, pc.template(combo[0]))
            for t in combo[1:]:
                expr = ["And", [expr, _spec(self.kb, pc.template(t))]]
            r = O.evaluate(expr, self.db)
            out.append(r["n"] if r["matched"] else 0)
        return np.array(out, dtype=np.uint64)


@pytest.fixture(scope="module")
def animals():
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    kb = O.KB.from_tables(d["nodes"], d["links"])
    odb = O.RedisMongoSemantics(kb)
    das = OracleMinerDB(odb, kb)
    seeds = [h for h, t, n in d["nodes"] if n in ("mammal", "human")]
    halo = miner.halo_host(das, seeds, 2)
    pcs = [miner.pattern_counts_host(das, halo.link_handles(lv)) for lv in range(2)]
    # the notebook's all_patterns: the levels' templates merged by handle; pattern_handles[0]: level 0's
    pc = miner.pattern_counts_host(das, halo.link_handles(0) + halo.link_handles(1))
    level0 = {pcs[0].handle(i) for i in range(len(pcs[0]))}
    basics = [i for i in range(len(pc)) if pc.handle(i) in level0]
    return kb, odb, das, pc, basics, halo.universe_size


def _spec(kb, template):
    k = itertools.count(1)
    return ["Link", template[0], template[0] not in UNORDERED_LINK_TYPES,
            [["Var", f"V{next(k)}"] if h == WILDCARD else ["Node", *kb.nodes[h]] for h in template[1:]]]


class Notebook:
    """Cell efac9ac6 with compute_isurprisingness (cell 3fa7b2ec) beside it;
    compute_count is the oracle's answer to the composite pattern."""

    def __init__(self, kb, odb, pc, universe_size):
        self.kb, self.odb, self.pc, self.universe_size = kb, odb, pc, universe_size
        self.specs = [_spec(kb, pc.template(i)) for i in range(len(pc))]
        self.asked = {}

    def compute_count(self, terms):
        """And([And([t0, t1]), t2]) .. of build_composite_pattern"""
        if terms not in self.asked:
            expr = self.specs[terms[0]]
            for t in terms[1:]:
                expr = ["And", [expr, self.specs[t]]]
            r = O.evaluate(expr, self.odb)
            self.asked[terms] = r["n"] if r["matched"] else 0
        return self.asked[terms]

    def prob(self, count):
        return count / self.universe_size

    def compute_isurprisingness(self, count, terms, counts, normalized):
        prob, cc = self.prob, self.compute_count
        if len(terms) == 2:
            subset_probs = [prob(counts[0]) * prob(counts[1])]
        else:
            subset_probs = [
                prob(counts[0]) * prob(counts[1]) * prob(counts[2]),
                prob(cc((terms[0], terms[1]))) * prob(counts[2]),
                prob(cc((terms[0], terms[2]))) * prob(counts[1]),
                prob(cc((terms[1], terms[2]))) * prob(counts[0]),
            ]
        p = prob(count)
        isurprisingness = max([p - max(subset_probs), min(subset_probs) - p])
        return isurprisingness / p if normalized else isurprisingness

    def exhaustive(self, basics, all_patterns, ngram, support, normalized):
        higher_isurprisingness = 0
        best = None
        for basic in basics:
            for combination in itertools.combinations(all_patterns, ngram - 1):
                if basic in combination:
                    continue
                terms = (basic, *combination)
                counts = [int(self.pc.count[t]) for t in terms]
                count = self.compute_count(terms)
                if count >= support:
                    isurprisingness = self.compute_isurprisingness(count, terms, counts, normalized)
                    if isurprisingness > higher_isurprisingness:
                        higher_isurprisingness = isurprisingness
                        best = (terms, count, isurprisingness)
        return best


# (normalized with support 0 divides by zero in the notebook: its cell cannot run there)
@pytest.mark.parametrize("ngram,support,normalized", [(2, 0, False), (3, 0, False), (2, 1, True), (3, 1, True),
                                                      (3, 2, False)])
def test_mine_host_is_the_notebooks_exhaustive_cell(animals, ngram, support, normalized):
    kb, odb, das, pc, basics, universe = animals
    assert len(basics) >= 4 and len(pc) > len(basics) and universe > 0
    basics = basics[:4]
    candidates = list(range(len(pc)))[::max(1, len(pc) // 14)] if ngram == 3 else list(range(len(pc)))
    nb = Notebook(kb, odb, pc, universe)
    want = nb.exhaustive(basics, candidates, ngram, support, normalized)
    got = miner.mine_host(das, pc, basics, universe, ngram=ngram, support=support, normalized=normalized, top=1,
                          candidates=candidates)
    assert want is not None and len(got) == 1
    terms, count, value = want
    assert tuple(got.combos[0].tolist()) == terms and int(got.count[0]) == count
    assert got.value[0] == value                                         # the same operations in the same order
    assert got.searched == got.scored == sum(
        1 for b in basics for c in itertools.combinations(candidates, ngram - 1) if b not in c)
    # the whole list: every reported row is a row of the space, ordered by value, ties by enumeration order
    full = miner.mine_host(das, pc, basics, universe, ngram=ngram, support=support, normalized=normalized,
                           top=miner.MINE_MAX_TOP, candidates=candidates, batch=37)
    space = [(b, *c) for b in basics for c in itertools.combinations(sorted(candidates), ngram - 1) if b not in c]
    rank = {row: i for i, row in enumerate(space)}
    rows = [tuple(r) for r in full.combos.tolist()]
    assert rows[0] == terms and len(set(rows)) == len(rows) and set(rows) <= set(rank)
    keys = [(-v, rank[r]) for r, v in zip(rows, full.value.tolist())]
    assert keys == sorted(keys) and (full.value > 0).all() and (full.count >= support).all()
    scored = {row: nb.compute_isurprisingness(nb.compute_count(row), row, [int(pc.count[t]) for t in row], normalized)
              for row in space if nb.compute_count(row) >= max(support, 1 if normalized else 0)}
    assert {r for r, v in scored.items() if v > 0} == set(rows)
    assert [scored[r] for r in rows] == full.value.tolist()
    # pattern(i) is the composite pattern the notebook would print
    assert repr(got.pattern(0)) == repr(miner.build_composite_pattern([pc.pattern(t) for t in terms]))


def test_mine_facade_runs_the_host_loop(animals):
    from das_amd.distributed_atom_space import DistributedAtomSpace
    kb, odb, das, pc, basics, universe = animals
    got = miner.mine(das, pc, basics[:2], universe, ngram=2, top=3)
    want = miner.mine_host(das, pc, basics[:2], universe, ngram=2, top=3)
    assert got.combos.tolist() == want.combos.tolist() and got.value.tolist() == want.value.tolist()
    assert hasattr(DistributedAtomSpace, "mine")


def test_max_combinations_and_bad_arguments(animals):
    kb, odb, das, pc, basics, universe = animals
    m = len(pc)
    searched = miner.search_space_size(np.array(basics[:3]), np.arange(m), 3)
    assert searched == 3 * (m - 1) * (m - 2) // 2
    with pytest.raises(ValueError, match=str(searched)):
        miner.mine_host(das, pc, basics[:3], universe, max_combinations=searched - 1)
    for kw in (dict(ngram=4), dict(ngram=1), dict(top=0), dict(top=miner.MINE_MAX_TOP + 1), dict(support=-1),
               dict(candidates=[0, 0]), dict(candidates=[m]), dict(candidates=[-1])):
        with pytest.raises(ValueError):
            miner.mine_host(das, pc, basics[:1], universe, **kw)
    for bad in ([0, 0], [m], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            miner.mine_host(das, pc, bad, universe)
    with pytest.raises(ValueError):
        miner.mine_host(das, pc, basics[:1], 0)
    # nothing to search is an empty answer, not an error
    empty = miner.mine_host(das, pc, [], universe)
    assert len(empty) == 0 and empty.searched == 0 and empty.combos.shape == (0, 3)
    assert len(miner.mine_host(das, pc, basics[:1], universe, candidates=[])) == 0
