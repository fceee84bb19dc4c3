"""answer.value_counts on the device (das_group_counts): the
rows of an answer per value of one variable, counted from resolved tables and
from the three unresolved forms without writing their rows.

The reference is value_counts_host -- a Counter over the answer's Assignment
objects -- on the same query's answer, computed once per query and shared, or
a closed form where the answer is too large to build.  DAS_GROUP_DIRECT=0|1
forces the sorted / the direct strategy; launch counts (k_cartesian,
k_dj_write*, k_project / k_copy_*) show that no rows were written.

The KB.  R<n> (n in ROWS) holds n links (a_i, c_{i % 7}); E<n> (n in RANGES)
holds one link (k<n>_i, z) for every node of type K<n>, which has n nodes --
ids are clustered by named type, so E<n>'s first column has a bound range of
exactly n ids: the LDS tile's bin count, one below, one above.  P130 / Q70
(130 and 70 distinct links, values repeated on three of the four columns)
are the factors of the small product.  M, I<n>, U<n> have the shape
tests/test_gpu_deferred_join.py documents: M's 11000 links (g, b) with the
hubs b_0 and g_5, I<n> the reverse fold's probe (b_51 .. b_63 without a
partner: count 0), U<n> the forward fold's (g_9000 and up without one).  A
second KB holds the two 70000-row factors of the large product."""
import json
import os
from collections import Counter

import numpy as np
import pytest

from tests.util import build

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LDS_BINS = 4096                      # kGroupLdsBins (das_amd/csrc/group_plan.h)
ROWS = (63, 64, 65, 1023, 1024, 1025)
RANGES = (LDS_BINS - 1, LDS_BINS, LDS_BINS + 1)
PROBES = (2049, 2177)                # kIjSmall + 1; one more than that plus an expansion unit of 128 rows
N_G = 5 * PROBES[-1] + 8
BIG = 70000
STRATEGIES = ["0", "1"]


def _arrays():
    from das_amd import loader
    b = loader.AtomBuilder()
    node = lambda name, t="Concept": b.terminal(t, name, True)  # noqa: E731
    a = [node(f"a{i}") for i in range(ROWS[-1])]
    c = [node(f"c{i}") for i in range(7)]
    z = node("z")
    for n in ROWS:
        for i in range(n):
            b.expr(f"R{n}", [a[i], c[i % 7]])
    for n in RANGES:
        for i in range(n):
            b.expr(f"E{n}", [node(f"k{n}_{i}", f"K{n}"), z])
    for i in range(130):
        b.expr("P130", [a[i % 65], c[i // 65]])
    for i in range(70):
        b.expr("Q70", [a[100 + i % 9], a[200 + i]])
    g = [node(f"g{i}") for i in range(N_G)]
    bp = [node(f"b{i}") for i in range(64)]
    x = [node(f"x{i}") for i in range(2000)]
    p = [node(f"p{i}") for i in range(PROBES[-1])]
    hub = node("hub")
    for i in range(6000):
        b.expr("M", [g[i], bp[0]])
    for i in range(3000):
        b.expr("M", [g[i], bp[1 + i % 50]])
    for j in range(2000):
        b.expr("M", [g[5], x[j]])
    for n in PROBES:
        for i in range(n):
            b.expr(f"I{n}", [bp[i % 64], p[i]])
            b.expr(f"U{n}", [g[5 * i], hub])
    return b.finish()


def _big_arrays():
    from das_amd import loader
    b = loader.AtomBuilder()
    node = lambda name: b.terminal("Concept", name, True)  # noqa: E731
    hp, hq = node("hp"), node("hq")
    for i in range(BIG):
        b.expr("PB", [node(f"p{i}"), hp])
        b.expr("QB", [node(f"q{i}"), hq])
    return b.finish()


@pytest.fixture(autouse=True)
def no_row_floor(monkeypatch):
    """Every answer takes the device path whatever its size: no test depends
    on where HipDB.GROUP_MIN puts the switch to the host Counter."""
    from das_amd.database.hip_db import HipDB
    monkeypatch.setattr(HipDB, "GROUP_MIN", 0)


@pytest.fixture(scope="module")
def arrays():
    return _arrays()


@pytest.fixture(scope="module")
def kb(arrays):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(arrays)
    return db


@pytest.fixture(scope="module")
def big():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(_big_arrays())
    return db


def V(x):
    return ["Var", x]


def L(name, *targets):
    return ["Link", name, True, list(targets)]


HUB = ["Node", "Concept", "hub"]
M_SCAN = L("M", V("Vg"), V("Vb"))
JOIN_ENV = {"DAS_FUSED": "0", "DAS_REV_IJ": "1", "DAS_IJ_MID": "0"}


def ask(db, spec, monkeypatch, **env):
    """The query's answer, still holding its device relation."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    monkeypatch.setenv("DAS_FUSED", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ans = pm.PatternMatchingAnswer()
    assert build(spec).matched(db, ans)
    assert ans._rel is not None and ans._rel.tables
    return ans


_HOST = {}


def host_counts(db, key, ans, variable):
    """value_counts_host of the query `key` names, computed once (it builds
    the answer's Assignment objects, which settles `ans`: call it last)."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    k = (key, variable)
    if k not in _HOST:
        _HOST[k] = dict(pm.value_counts_host(db, ans, variable))
    return _HOST[k]


def device_counts(db, ans, variable, monkeypatch, direct=None):
    """ans.value_counts on the device path, checked for its own invariants."""
    if direct is None:
        monkeypatch.delenv("DAS_GROUP_DIRECT", raising=False)
    else:
        monkeypatch.setenv("DAS_GROUP_DIRECT", direct)
    monkeypatch.delenv("DAS_GROUP", raising=False)
    before = dict(db.group_stats)
    vc = ans.value_counts(variable)
    assert db.group_stats["device"] == before["device"] + 1 and db.group_stats["host"] == before["host"]
    assert vc.ids.dtype == np.uint32 and vc.counts.dtype == np.uint64
    assert np.all(vc.ids[1:] > vc.ids[:-1]) and np.all(vc.counts > 0)
    assert vc.total == ans.count()
    return vc


class Prof:
    """Launches recorded between enter and read(): (row-writing launches --
    k_cartesian*, k_dj_write* --, k_project + k_copy_*)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.prof_enable(True)
        self.ctx.prof_reset()
        return self

    def read(self):
        self.ctx.sync()
        st = self.ctx.prof_stats()
        w = sum(v["launches"] for k, v in st.items() if k.startswith(("k_dj_write", "k_cartesian")))
        c = sum(v["launches"] for k, v in st.items() if k.startswith(("k_project", "k_copy_")))
        self.ctx.prof_reset()
        return w, c

    def group_scopes(self):
        self.ctx.sync()
        return {k for k, v in self.ctx.prof_stats().items() if k.startswith("k_group") and v["launches"]}

    def __exit__(self, *exc):
        self.ctx.prof_enable(False)
        self.ctx.prof_reset()


# ---- 1. resolved tables, both strategies ------------------------------------

@pytest.mark.parametrize("direct", STRATEGIES, ids=["sorted", "direct"])
@pytest.mark.parametrize("n", ROWS)
def test_gpu_scan_rows(kb, monkeypatch, n, direct):
    ans = ask(kb, L(f"R{n}", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    assert ans.count() == n
    got = {v: device_counts(kb, ans, v, monkeypatch, direct).as_dict() for v in ("Va", "Vc")}
    for v in ("Va", "Vc"):
        assert got[v] == host_counts(kb, ("R", n), ans, v)
    assert len(got["Va"]) == n and len(got["Vc"]) == 7           # every row a distinct key; seven keys


@pytest.mark.parametrize("direct", STRATEGIES + [None], ids=["sorted", "direct", "rule"])
@pytest.mark.parametrize("n", RANGES)
def test_gpu_range_at_the_lds_tile(kb, monkeypatch, n, direct):
    """Key ranges of one bin less than the LDS tile, the tile, and one more
    (global atomics); the second column is one key holding every row."""
    ans = ask(kb, L(f"E{n}", V("Vk"), V("Vz")), monkeypatch, DAS_DEFER_JOIN="0")
    t, = ans._rel.tables
    lo, hi = t.bounds()
    assert sorted(h - l + 1 for l, h in zip(lo, hi)) == [1, n]   # the typed column's bound range is n ids
    with Prof(kb.ctx) as p:
        vk = device_counts(kb, ans, "Vk", monkeypatch, direct)
        scopes = p.group_scopes()
    if direct != "0":
        assert ("k_group_accum<true>" in scopes) == (n <= LDS_BINS)
        assert ("k_group_accum<false>" in scopes) == (n > LDS_BINS)
    else:
        assert "k_group_runs" in scopes and not any(s.startswith("k_group_accum") for s in scopes)
    vz = device_counts(kb, ans, "Vz", monkeypatch, direct)
    assert len(vk) == n and np.all(vk.counts == 1) and int(vk.ids[-1]) - int(vk.ids[0]) + 1 == n
    assert vz.counts.tolist() == [n]
    assert vk.as_dict() == host_counts(kb, ("E", n), ans, "Vk")
    assert vz.as_dict() == host_counts(kb, ("E", n), ans, "Vz")


@pytest.mark.parametrize("direct", STRATEGIES, ids=["sorted", "direct"])
def test_gpu_unknown_bounds(kb, monkeypatch, direct):
    """A host table without das_table_set_bounds: counters over [0, n_atoms)."""
    monkeypatch.setenv("DAS_GROUP_DIRECT", direct)
    rng = np.random.default_rng(7)
    n_atoms = sum(kb.count_atoms())
    cols = np.stack([rng.integers(0, n_atoms, 5000), rng.integers(3, 9, 5000)]).astype(np.uint32)
    cols[0, :1500] = n_atoms - 1                                 # a hub at the last id
    t = kb.ctx.table_from_host(0, (1, 2), cols)
    assert t.bounds() == ([0, 0], [0xFFFFFFFF, 0xFFFFFFFF])
    for c in (0, 1):
        ids, counts, stats = kb.ctx.group_counts([t], [c])
        want_ids, want_counts = np.unique(cols[c], return_counts=True)
        assert np.array_equal(ids, want_ids) and np.array_equal(counts, want_counts.astype(np.uint64))
        assert stats == (0, 0)


# ---- 2. several tables in one answer ----------------------------------------

@pytest.mark.parametrize("direct", STRATEGIES, ids=["sorted", "direct"])
def test_gpu_counts_add_across_tables(kb, monkeypatch, direct):
    spec = ["Or", [L("R65", V("Va"), V("Vc")), L("R1023", V("Va"), V("Vd"))]]
    ans = ask(kb, spec, monkeypatch, DAS_DEFER_JOIN="0")
    assert sorted(len(t.vars) for t in ans._rel.tables) == [2, 2] and ans.count() == 65 + 1023
    va = device_counts(kb, ans, "Va", monkeypatch, direct)
    assert sorted(Counter(va.counts.tolist()).items()) == [(1, 1023 - 65), (2, 65)]
    with pytest.raises(KeyError):
        ans.value_counts("Vc")                                  # the second table does not bind it
    with pytest.raises(KeyError):
        ans.value_counts("Vd")
    assert va.as_dict() == host_counts(kb, "or", ans, "Va")


# ---- 3. deferred products ---------------------------------------------------

PRODUCT = ["And", [L("P130", V("V1"), V("V2")), L("Q70", V("V3"), V("V4"))]]


@pytest.mark.parametrize("direct", STRATEGIES, ids=["sorted", "direct"])
def test_gpu_small_product(kb, monkeypatch, direct):
    eager = ask(kb, PRODUCT, monkeypatch, DAS_DEFER_PRODUCT="0")
    with Prof(kb.ctx) as p:
        ans = ask(kb, PRODUCT, monkeypatch, DAS_DEFER_PRODUCT="1")
        assert ans.count() == eager.count() == 130 * 70 and p.read()[0] == 0
        before = dict(kb.group_stats)
        got = {v: device_counts(kb, ans, v, monkeypatch, direct).as_dict() for v in ("V1", "V2", "V3", "V4")}
        assert p.read()[0] == 0                                  # the product was not written
        assert kb.group_stats["unwritten"] == before["unwritten"] + 4
        assert kb.group_stats["settled"] == before["settled"]
    for v in got:
        assert got[v] == device_counts(kb, eager, v, monkeypatch, direct).as_dict()
        assert got[v] == host_counts(kb, "product", ans, v)
    assert len(got["V1"]) == 65 and len(got["V2"]) == 2 and len(got["V3"]) == 9 and len(got["V4"]) == 70


@pytest.mark.parametrize("direct", STRATEGIES, ids=["sorted", "direct"])
def test_gpu_large_product_is_not_written(big, monkeypatch, direct):
    """70000 x 70000 rows: one count of 4.9e9 (above 2^32), from the factors."""
    spec = ["And", [L("PB", V("V1"), V("V2")), L("QB", V("V3"), V("V4"))]]
    monkeypatch.delenv("DAS_DEFER_PRODUCT", raising=False)
    with Prof(big.ctx) as p:
        ans = ask(big, spec, monkeypatch)
        assert ans.count() == BIG * BIG and p.read()[0] == 0
        for _ in range(2):                                       # the second call: still unresolved
            before = dict(big.group_stats)
            hubs = [device_counts(big, ans, v, monkeypatch, direct) for v in ("V2", "V4")]
            each = [device_counts(big, ans, v, monkeypatch, direct) for v in ("V1", "V3")]
            assert p.read()[0] == 0                              # no k_cartesian launch
            assert big.group_stats["unwritten"] == before["unwritten"] + 4
            assert big.group_stats["settled"] == before["settled"]
    for vc, name in zip(hubs, ("hp", "hq")):
        assert vc.counts.tolist() == [BIG * BIG] and vc.total == ans.count() == 4900000000
        assert vc.names() == [name]
    for vc in each:
        assert len(vc) == BIG and np.all(vc.counts == BIG) and vc.total == ans.count()


# ---- 4. deferred index joins ------------------------------------------------

def reverse_spec(n):
    return ["And", [M_SCAN, L(f"I{n}", V("Vb"), V("Vp"))]]


def forward_spec(n):
    return ["And", [L(f"U{n}", V("Vg"), HUB), M_SCAN]]


# fold -> (spec, a probe-side variable, the variable the expansion reads from the index)
FOLDS = {"reverse": (reverse_spec, "Vb", "Vg"), "forward": (forward_spec, "Vg", "Vb")}


@pytest.mark.parametrize("direct", STRATEGIES, ids=["sorted", "direct"])
@pytest.mark.parametrize("balanced", ["0", "1"], ids=["units", "balanced"])
@pytest.mark.parametrize("n", PROBES)
@pytest.mark.parametrize("fold", sorted(FOLDS))
def test_gpu_deferred_join(kb, monkeypatch, fold, n, balanced, direct):
    make, probe_var, fresh_var = FOLDS[fold]
    env = dict(JOIN_ENV, DAS_DJ_BALANCED=balanced)
    eager = ask(kb, make(n), monkeypatch, DAS_DEFER_JOIN="0", **env)
    with Prof(kb.ctx) as p:
        ans = ask(kb, make(n), monkeypatch, DAS_DEFER_JOIN="1", **env)
        assert p.read()[0] == 0 and ans.count() == eager.count() > n
        before = dict(kb.group_stats)
        by_probe = device_counts(kb, ans, probe_var, monkeypatch, direct)
        assert p.read()[0] == 0                                  # no expansion write
        assert kb.group_stats["unwritten"] == before["unwritten"] + 1
        assert kb.group_stats["settled"] == before["settled"]
        by_fresh = device_counts(kb, ans, fresh_var, monkeypatch, direct)
        assert p.read()[0] == 1                                  # the one write
        assert kb.group_stats["settled"] == before["settled"] + 1
        again = device_counts(kb, ans, probe_var, monkeypatch, direct)
        assert p.read()[0] == 0 and kb.group_stats["settled"] == before["settled"] + 1
    assert again.as_dict() == by_probe.as_dict()
    assert by_probe.as_dict() == device_counts(kb, eager, probe_var, monkeypatch, direct).as_dict()
    assert by_fresh.as_dict() == device_counts(kb, eager, fresh_var, monkeypatch, direct).as_dict()
    assert by_probe.as_dict() == host_counts(kb, (fold, n), ans, probe_var)
    assert by_fresh.as_dict() == host_counts(kb, (fold, n), ans, fresh_var)
    if fold == "reverse":
        # b_51 .. b_63 have probe rows and no partner in M: count 0, absent
        assert sorted(by_probe.names()) == sorted(f"b{i}" for i in range(51))


# ---- 5. scan views ----------------------------------------------------------

def test_gpu_scan_view_is_counted_in_place(arrays, monkeypatch):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(arrays)
    with Prof(db.ctx) as p:
        ans = ask(db, M_SCAN, monkeypatch, DAS_DEFER_JOIN="1")
        assert ans.count() == 11000 and p.read() == (0, 0)
        before = dict(db.group_stats)
        got = {v: device_counts(db, ans, v, monkeypatch).as_dict() for v in ("Vg", "Vb")}
        assert p.read() == (0, 0)                                # no write, no copy of the view
        assert db.group_stats["unwritten"] == before["unwritten"] + 2
        for direct in STRATEGIES:
            for v in got:
                assert device_counts(db, ans, v, monkeypatch, direct).as_dict() == got[v]
        p.read()
        # the index is rebuilt under the view: the registry settles it (the same
        # arrays give the same ids)
        db.load_arrays(arrays)
        assert p.read()[1] >= 2
        before = dict(db.group_stats)
        for v in got:
            assert device_counts(db, ans, v, monkeypatch).as_dict() == got[v]
        assert db.group_stats["unwritten"] == before["unwritten"]
    for v in got:
        assert got[v] == host_counts(db, "view", ans, v)
    assert max(got["Vb"].values()) == 6000 and max(got["Vg"].values()) == 2002


# ---- 6. matched_many and the facade -----------------------------------------

def _animals():
    from das_amd import loader
    from das_amd.distributed_atom_space import DistributedAtomSpace
    from das_amd.database.hip_db import HipDB
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    db = HipDB(device=0)
    db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    return DistributedAtomSpace(db=db), db


def test_gpu_facade_and_matched_many(monkeypatch):
    from das_amd.pattern_matcher import pattern_matcher as pm
    monkeypatch.delenv("DAS_GROUP", raising=False)
    das, db = _animals()
    query = build(["And", [L("Inheritance", V("V1"), V("V2")), L("Inheritance", V("V2"), V("V"))]])
    (matched, ans), = pm.matched_many(db, [query])
    assert matched
    want = pm.value_counts_host(db, ans, "V")
    order = sorted(want.items(), key=lambda kv: (-kv[1], kv[0]))
    before = db.group_stats["device"]
    assert das.value_counts(query, "V", top=3, names=True) == [(db.get_node_name(h), n) for h, n in order[:3]]
    assert das.value_counts(query, "V", top=3) == order[:3]
    assert das.value_counts(query, "V").as_dict() == dict(want)
    assert db.group_stats["device"] == before + 3
    (_, fresh), = pm.matched_many(db, [query])
    assert sorted(fresh.distinct("V")) == sorted(set(want)) and db.group_stats["device"] == before + 4
    assert len(want) > 1


# ---- 7. switches ------------------------------------------------------------

def test_gpu_switch_takes_the_host_path(kb, monkeypatch):
    ans = ask(kb, L("R65", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    dev = device_counts(kb, ans, "Vc", monkeypatch)
    monkeypatch.setenv("DAS_GROUP", "0")
    before = dict(kb.group_stats)
    host = ans.value_counts("Vc")
    assert kb.group_stats["host"] == before["host"] + 1 and kb.group_stats["device"] == before["device"]
    assert host.ids is None and host.as_dict() == dev.as_dict()
    assert host.most_common() == dev.most_common() and host.total == dev.total == 65
    monkeypatch.delenv("DAS_GROUP")
    monkeypatch.setattr(type(kb), "GROUP_MIN", 66)
    assert ans.value_counts("Vc").ids is None and kb.group_stats["host"] == before["host"] + 2


# ---- 8. ABI edges -----------------------------------------------------------

def test_gpu_abi_small_capacity_then_fill(kb, monkeypatch):
    import ctypes as C
    from das_amd import _lib
    ans = ask(kb, L("R1025", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    t, = ans._rel.tables
    th = (C.c_void_p * 1)(t.h)
    cols = np.array([0], dtype=np.int32)
    want_ids, want_counts, _ = kb.ctx.group_counts([t], [int(cols[0])])
    n = C.c_uint64()
    stats = np.zeros(2, dtype=np.uint64)
    ids, counts = np.zeros(len(want_ids), np.uint32), np.zeros(len(want_ids), np.uint64)
    call = lambda i, c, cap: _lib.lib().das_group_counts(kb.ctx.h, th, _lib.ptr(cols), 1, _lib.ptr(i), _lib.ptr(c), cap,  # noqa: E731,E501
                                                         C.byref(n), _lib.ptr(stats))
    assert call(None, None, 0) == _lib.ERR_INVALID and n.value == len(want_ids) > 1
    assert b"capacity" in _lib.lib().das_last_error(kb.ctx.h)
    n.value = 0
    assert call(ids, counts, 3) == _lib.ERR_INVALID and n.value == len(want_ids)
    with Prof(kb.ctx) as p:
        assert call(ids, counts, len(want_ids)) == 0 and n.value == len(want_ids)
        assert p.group_scopes() == set()                         # the kept result: not counted again
    assert np.array_equal(ids, want_ids) and np.array_equal(counts, want_counts)
    assert call(None, None, 5) == _lib.ERR_INVALID               # (cap && !out)
    with pytest.raises(ValueError):
        kb.ctx.group_counts([t], [2])                            # column out of range
    with pytest.raises(ValueError):
        kb.ctx.group_counts([t], [-1])


def test_gpu_abi_refuses_a_composite_table(kb):
    from das_amd import _lib
    cols = np.arange(12, dtype=np.uint32).reshape(2, 6)
    comp = kb.ctx.table_from_host(_lib.TABLE_COMPOSITE, (1, 2), cols, members=(0, 0))
    with pytest.raises(ValueError, match="ORDERED"):
        kb.ctx.group_counts([comp], [0])
    unordered = kb.ctx.table_from_host(_lib.TABLE_UNORDERED, (1, 2), cols)
    with pytest.raises(ValueError, match="ORDERED"):
        kb.ctx.group_counts([unordered], [0])


def test_gpu_abi_refuses_another_context(kb, monkeypatch):
    from das_amd import _lib
    other = _lib.Context(0, None)
    ans = ask(kb, reverse_spec(2049), monkeypatch, DAS_DEFER_JOIN="1", **JOIN_ENV)
    t, = ans._rel.tables
    col = 0
    with Prof(kb.ctx) as p:
        with pytest.raises(ValueError, match="context that made it"):
            other.group_counts([t], [col])
        assert p.read()[0] == 0                                  # and it stays unresolved
    ids, counts, stats = kb.ctx.group_counts([t], [col])
    assert int(counts.sum()) == ans.count() and sum(stats) == 1
