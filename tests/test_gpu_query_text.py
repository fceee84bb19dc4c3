"""answer.text / iter_text / das.query on the device (das_table_rows_text,
DESIGN.md §3g): the rows of an ordered answer rendered as str(set) text.

The byte-exact expectation is a host model: t.fetch(), db.hex_of of each
column and repr(dict(zip(names, row))) per row, joined by ", " in table row
order -- no Assignment objects.  The facade is compared with the host path
(DAS_QUERY_TEXT=0, the set of Assignment objects formatted as before) as a
multiset of row texts, the order of a set's rows being unspecified.

The KB.  a_i are nodes; R<n> (n in EDGE_ROWS: around 64 and around the tile's
row count T of a two-variable row) holds n links (a_i, c_{i % 7}); A1 holds
761 links (a_i, z), queried with one variable whose name has 1 .. 16
characters, so that a row and its separator take every length mod 16 and the
tiles' spans begin at every byte alignment; R3 holds links of arity 3.  Eight
columns are a host table of node ids: a Link of arity 8 with eight variables
has no pattern key in the reference (arities 1 .. 3 only) and never matches.
P130 / Q70 are the factors of a deferred product and M / I2049 the
deferred index join of tests/test_gpu_deferred_join.py (reverse fold)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from das_amd import _lib
from tests.util import build

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEP = b", "


def tile_rows(names):
    """Rows of one tile for rows binding `names`: the kernel's rule
    (rows_text.h) from the mirrored constants."""
    unit = len(repr({n: "0" * 32 for n in names}).encode("utf-8")) + len(SEP)
    return (_lib.ROWS_TEXT_STAGE_BYTES - 16) // unit


T2 = tile_rows(["Va", "Vc"])
EDGE_ROWS = (1, 63, 64, 65, T2 - 1, T2, T2 + 1, 2 * T2 + 1)
ALIGN_NAMES = ["V" + "x" * k for k in range(16)]                 # 1 .. 16 characters
N_A1 = 2 * tile_rows(ALIGN_NAMES[0]) + 1
TRICKY = ["it's", 'q"uote', "both ' and \"", "back\\slash", "né", "V6", "V7", "V8"]
N_PROBE = 2049                       # kIjSmall + 1: the index join goes through its count pass


def _arrays():
    from das_amd import loader
    b = loader.AtomBuilder()
    node = lambda name: b.terminal("Concept", name, True)  # noqa: E731
    a = [node(f"a{i}") for i in range(max(N_A1, EDGE_ROWS[-1]) + 8)]
    c = [node(f"c{i}") for i in range(7)]
    z = node("z")
    for n in EDGE_ROWS:
        for i in range(n):
            b.expr(f"R{n}", [a[i], c[i % 7]])
    for i in range(N_A1):
        b.expr("A1", [a[i], z])
    for i in range(5):
        b.expr("R3", [a[i], a[i + 1], c[i]])
    for i in range(130):
        b.expr("P130", [a[i % 65], c[i // 65]])
    for i in range(70):
        b.expr("Q70", [a[100 + i % 9], a[200 + i]])
    g = [node(f"g{i}") for i in range(6000)]
    bp = [node(f"b{i}") for i in range(64)]
    x = [node(f"x{i}") for i in range(2000)]
    p = [node(f"p{i}") for i in range(N_PROBE)]
    for i in range(6000):
        b.expr("M", [g[i], bp[0]])
    for i in range(3000):
        b.expr("M", [g[i], bp[1 + i % 50]])
    for j in range(2000):
        b.expr("M", [g[5], x[j]])
    for i in range(N_PROBE):
        b.expr(f"I{N_PROBE}", [bp[i % 64], p[i]])
    return b.finish()


@pytest.fixture(autouse=True)
def no_row_floor(monkeypatch):
    """Every eligible answer takes the device path whatever its size: no test
    depends on where HipDB.QUERY_TEXT_MIN puts the switch."""
    from das_amd.database.hip_db import HipDB
    monkeypatch.setattr(HipDB, "QUERY_TEXT_MIN", 0)
    monkeypatch.delenv("DAS_QUERY_TEXT", raising=False)


@pytest.fixture(scope="module")
def kb():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(_arrays())
    return db


def V(x):
    return ["Var", x]


def L(name, *targets):
    return ["Link", name, True, list(targets)]


Z = ["Node", "Concept", "z"]
JOIN_ENV = {"DAS_FUSED": "0", "DAS_REV_IJ": "1", "DAS_IJ_MID": "0"}
PRODUCT = ["And", [L("P130", V("V1"), V("V2")), L("Q70", V("V3"), V("V4"))]]
EXPANSION = ["And", [L("M", V("Vg"), V("Vb")), L(f"I{N_PROBE}", V("Vb"), V("Vp"))]]


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


def names_of(t):
    from das_amd.pattern_matcher import pattern_matcher as pm
    return [pm._var_name(v) for v in t.vars]


def model_rows(db, t, row0=0, n=None):
    """The host model: the text of each of the rows, in table row order."""
    cols = t.fetch(row0, n)
    hexes = [db.hex_of(c) for c in cols]
    names = names_of(t)
    return [repr(dict(zip(names, row))) for row in zip(*hexes)]


def device(db, t, row0=0, n=None, **kw):
    """das_table_rows_text of the rows, checked for its own invariants."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    lits = pm.row_literals(names_of(t))
    data, total, bad = db.ctx.rows_text(t, lits, SEP, row0=row0, nrows=n, **kw)
    assert bad == 0 and total == _lib.rows_text_size(lits, SEP, t.nrows - row0 if n is None else n)
    return bytes(data).decode("utf-8")


def rows_of(text):
    """The row texts of a str(set of ordered assignments)."""
    assert text.startswith("{") and text.endswith("}")
    return sorted(re.findall(r"\{[^{}]*\}", text[1:-1]))


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
        self.text_launches = sum(v["launches"] for k, v in st.items() if k.startswith("k_rows_text"))
        self.ctx.prof_reset()
        return w, c

    def __exit__(self, *exc):
        self.ctx.prof_enable(False)
        self.ctx.prof_reset()


# ---- 1. tile edges ----------------------------------------------------------

@pytest.mark.parametrize("n", EDGE_ROWS)
def test_gpu_tile_edges(kb, monkeypatch, n):
    ans = ask(kb, L(f"R{n}", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    t, = ans._rel.tables
    assert t.nrows == n and tile_rows(names_of(t)) == T2
    want = model_rows(kb, t)
    assert device(kb, t) == ", ".join(want)
    for row0 in (0, 1, 15, 16, 17):
        if row0 < n:
            assert device(kb, t, row0) == ", ".join(want[row0:]), row0
            assert device(kb, t, row0, 1) == want[row0], row0
    before = dict(kb.query_text_stats)
    with Prof(kb.ctx) as p:
        assert ans.text() == "{" + ", ".join(want) + "}"
        p.read()
        assert p.text_launches == 1                             # one launch per call
    assert kb.query_text_stats == {"device": before["device"] + 1, "host": before["host"]}
    assert ans._py is None                                      # no Assignment object was built


# ---- 2. every byte alignment of a tile's span -------------------------------

def test_gpu_alignment_names_cover_every_residue():
    units = {len(repr({n: "0" * 32}).encode()) + len(SEP) for n in ALIGN_NAMES}
    assert {u % 16 for u in units} == set(range(16))


@pytest.mark.parametrize("name", ALIGN_NAMES, ids=[str(len(n)) for n in ALIGN_NAMES])
def test_gpu_alignment(kb, monkeypatch, name):
    ans = ask(kb, L("A1", V(name), Z), monkeypatch, DAS_DEFER_JOIN="0")
    t, = ans._rel.tables
    assert names_of(t) == [name] and t.nrows == N_A1
    n = 2 * tile_rows([name]) + 1
    assert 3 <= n <= N_A1
    want = model_rows(kb, t)
    assert device(kb, t, 0, n) == ", ".join(want[:n])
    assert device(kb, t, 1, n - 1) == ", ".join(want[1:n])
    assert device(kb, t) == ", ".join(want)


# ---- 3. columns and variable names ------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_gpu_columns_and_tricky_names(kb, monkeypatch, k):
    from das_amd.database.hip_db import Relation
    from das_amd.expression_hasher import ExpressionHasher as EH
    from das_amd.pattern_matcher import pattern_matcher as pm
    names = TRICKY[:k]
    names = names[-1:] + names[:-1]
    if k < 8:
        spec = {1: L("A1", V(names[0]), Z), 2: L("R65", *map(V, names)), 3: L("R3", *map(V, names))}[k]
        ans = ask(kb, spec, monkeypatch, DAS_DEFER_JOIN="0")
    else:
        ids, cat, _ = kb.ctx.lookup_hex([EH.terminal_hash("Concept", f"a{i}") for i in range(12)])
        assert all(c == 1 for c in cat)
        cols = np.array([[ids[i + c] for i in range(5)] for c in range(8)], dtype=np.uint32)
        ans = pm.PatternMatchingAnswer()
        ans._set(kb, Relation([kb.ctx.table_from_host(_lib.TABLE_ORDERED, sorted(pm._vid(n) for n in names), cols)]))
    t, = ans._rel.tables
    assert sorted(names_of(t)) == sorted(names)
    want = model_rows(kb, t)
    text = ans.text()
    assert text == "{" + ", ".join(want) + "}"
    assert all(repr(n) + ": '" in text for n in names)
    assert "".join(ans.iter_text(chunk_rows=2)) == text
    monkeypatch.setenv("DAS_QUERY_TEXT", "0")
    assert rows_of(fresh_text(ans)) == sorted(want)            # byte for byte the host path's rows


def fresh_text(ans):
    """text() of a new answer over the same relation (the path the switches of the moment choose)."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    fresh = pm.PatternMatchingAnswer()
    fresh._set(ans._db, ans._rel)
    return fresh.text()


# ---- 4. cap -----------------------------------------------------------------

def test_gpu_cap_keeps_the_sentinel(kb, monkeypatch):
    from das_amd.pattern_matcher import pattern_matcher as pm
    ans = ask(kb, L(f"R{EDGE_ROWS[-1]}", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    t, = ans._rel.tables
    lits = pm.row_literals(names_of(t))
    want = np.frombuffer(", ".join(model_rows(kb, t)).encode(), dtype=np.uint8)
    for cap in (0, 1, 15, 16, 17, want.size - 1, want.size):
        out = np.full(want.size + 64, 0xEE, dtype=np.uint8)
        data, total, bad = kb.ctx.rows_text(t, lits, SEP, cap=cap, out=out)
        assert total == want.size and bad == 0 and data.size == cap
        assert np.array_equal(out[:cap], want[:cap]), cap
        assert np.all(out[cap:] == 0xEE), cap
    # a window that begins inside a tile, cut inside its second tile
    row = len(model_rows(kb, t, 0, 1)[0])
    cap = (T2 + 3) * (row + 2) + 5
    out = np.full(want.size, 0xEE, dtype=np.uint8)
    data, total, bad = kb.ctx.rows_text(t, lits, SEP, row0=7, cap=cap, out=out)
    assert total == want.size - 7 * (row + 2)
    assert np.array_equal(out[:cap], want[7 * (row + 2):][:cap]) and np.all(out[cap:] == 0xEE)


# ---- 5. unresolved answers --------------------------------------------------

def test_gpu_product_is_rendered_from_its_factors(kb, monkeypatch):
    with Prof(kb.ctx) as p:
        ans = ask(kb, PRODUCT, monkeypatch, DAS_DEFER_PRODUCT="1")
        assert ans.count() == 130 * 70 and p.read()[0] == 0
        t, = ans._rel.tables
        whole = ans.text()
        windows = {(r0, n): device(kb, t, r0, n) for r0, n in ((69, 3), (0, 70), (70 * 129 + 68, 2), (139, 141))}
        pieces = list(ans.iter_text(chunk_rows=1000))
        assert p.read()[0] == 0                                  # no k_cartesian launch
        t.fetch(0, 1)
        assert p.read()[0] == 1                                  # still deferred: a fetch expands the rows it reads
    want = model_rows(kb, t)
    assert len(want) == 9100 and whole == "{" + ", ".join(want) + "}"
    for (r0, n), got in windows.items():
        assert got == ", ".join(want[r0:r0 + n]), (r0, n)
    assert len(pieces) == 10 + 2 and "".join(pieces) == whole
    assert all(piece.startswith(", {") for piece in pieces[2:-1])


def test_gpu_scan_view_is_read_in_place(kb, monkeypatch):
    n = EDGE_ROWS[-1]
    with Prof(kb.ctx) as p:
        ans = ask(kb, L(f"R{n}", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="1")
        assert ans.count() == n and p.read() == (0, 0)
        t, = ans._rel.tables
        whole = ans.text()
        part = device(kb, t, 17, T2)
        assert p.read() == (0, 0)                                # no write, no copy of the view
        other = _lib.Context(0, None)
        with pytest.raises(ValueError, match="context that made it"):
            other.rows_text(t, [b"", b"", b""], SEP)
        kb.ctx.gather(t, np.array([0], dtype=np.uint32))
        assert p.read()[1] >= 1                                  # it was still a view: the gather copied it
    want = model_rows(kb, t)
    assert whole == "{" + ", ".join(want) + "}" and part == ", ".join(want[17:17 + T2])


def test_gpu_deferred_expansion_settles(kb, monkeypatch):
    from das_amd.pattern_matcher import pattern_matcher as pm
    with Prof(kb.ctx) as p:
        ans = ask(kb, EXPANSION, monkeypatch, DAS_DEFER_JOIN="1", **JOIN_ENV)
        assert p.read()[0] == 0 and ans.count() > N_PROBE
        t, = ans._rel.tables
        head = device(kb, t, 0, 3000)
        assert p.read()[0] == 1                                  # the one write
        tail = device(kb, t, t.nrows - 3000, 3000)
        assert p.read()[0] == 0
    assert head == ", ".join(model_rows(kb, t, 0, 3000))
    assert tail == ", ".join(model_rows(kb, t, t.nrows - 3000, 3000))
    lits = pm.row_literals(names_of(t))
    data, total, bad = kb.ctx.rows_text(t, lits, SEP, cap=0)
    assert data.size == 0 and bad == 0 and total == _lib.rows_text_size(lits, SEP, t.nrows)


# ---- 6. the facade ----------------------------------------------------------

def _animals():
    from das_amd import loader
    from das_amd.distributed_atom_space import DistributedAtomSpace
    from das_amd.database.hip_db import HipDB
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    db = HipDB(device=0)
    db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    return DistributedAtomSpace(db=db), db


INH = L("Inheritance", V("V1"), V("V2"))


def test_gpu_facade_equals_the_host_path(monkeypatch):
    from das_amd.pattern_matcher import pattern_matcher as pm
    das, db = _animals()
    queries = [build(["And", [INH, L("Inheritance", V("V2"), V("V3"))]]),
               build(["Or", [L("Inheritance", V("V1"), ["Node", "Concept", "mammal"]),
                             L("Inheritance", V("V1"), ["Node", "Concept", "animal"])]]),
               build(INH),
               pm.And([pm.NameMatch("V1", "Concept", "^m"), build(INH)])]
    for q in queries:
        monkeypatch.setenv("DAS_QUERY_TEXT", "0")
        before = dict(db.query_text_stats)
        host = das.query(q)
        assert db.query_text_stats == {"device": before["device"], "host": before["host"] + 1}
        ans = pm.PatternMatchingAnswer()
        assert q.matched(db, ans)
        assert rows_of(host) == sorted(repr(a.mapping) for a in ans.assignments)      # the old output
        assert len(rows_of(host)) == ans.count() > 1
        monkeypatch.delenv("DAS_QUERY_TEXT")
        dev = das.query(q)
        assert db.query_text_stats == {"device": before["device"] + 1, "host": before["host"] + 1}
        assert rows_of(dev) == rows_of(host) and len(dev) == len(host)
    # one row: byte-identical
    one = build(L("Inheritance", V("V1"), ["Node", "Concept", "dinosaur"]))
    monkeypatch.setenv("DAS_QUERY_TEXT", "0")
    host = das.query(one)
    monkeypatch.delenv("DAS_QUERY_TEXT")
    assert len(rows_of(host)) == 1 and das.query(one) == host


def test_gpu_facade_tables_and_host_cases(monkeypatch):
    from das_amd.database.hip_db import Relation
    from das_amd.pattern_matcher import pattern_matcher as pm
    das, db = _animals()
    # an Or of two schemas: both tables are rendered
    two = build(["Or", [INH, L("Inheritance", V("V3"), V("V4"))]])
    ans = pm.PatternMatchingAnswer()
    assert two.matched(db, ans) and len(ans._rel.tables) == 2
    before = dict(db.query_text_stats)
    dev = das.query(two)
    assert db.query_text_stats["device"] == before["device"] + 1
    want = [r for t in ans._rel.tables for r in model_rows(db, t)]
    assert rows_of(dev) == sorted(want) and "'V1'" in dev and "'V4'" in dev and len(want) == 24
    assert ans.text() == "{" + ", ".join(want) + "}"
    assert "".join(ans.iter_text(chunk_rows=5)) == ans.text()
    monkeypatch.setenv("DAS_QUERY_TEXT", "0")
    assert rows_of(das.query(two)) == sorted(want)
    monkeypatch.delenv("DAS_QUERY_TEXT")
    # two tables binding the same variables: a row could repeat, the set decides
    v1, v2 = pm._vid("V1"), pm._vid("V2")
    ids = ans._rel.tables[0].fetch()
    ta = db.ctx.table_from_host(_lib.TABLE_ORDERED, (v1, v2), ids[:, :5].copy())
    tb = db.ctx.table_from_host(_lib.TABLE_ORDERED, (v1, v2), ids[:, 3:9].copy())
    both = pm.PatternMatchingAnswer()
    both._set(db, Relation([ta, tb]))
    before = dict(db.query_text_stats)
    assert len(rows_of(both.text())) == 9                        # rows 3 and 4 are in both tables
    assert db.query_text_stats == {"device": before["device"], "host": before["host"] + 1}
    # unordered, empty and negated answers
    before = dict(db.query_text_stats)
    sim = das.query(pm.Link("Similarity", [pm.Variable("V1"), pm.Variable("V2")], False))
    assert sim.startswith("{") and db.query_text_stats == {"device": before["device"], "host": before["host"] + 1}
    empty = pm.PatternMatchingAnswer()
    empty._set(db, Relation([]))
    assert empty.text() == "set()" and list(empty.iter_text()) == ["set()"]
    assert db.query_text_stats["device"] == before["device"]
    assert das.query(pm.NameMatch("V2", "Concept", "no such name Q")) == ""
    neg = das.query(pm.Not(build(INH)))
    monkeypatch.setenv("DAS_QUERY_TEXT", "0")
    host_neg = das.query(pm.Not(build(INH)))
    assert neg[:4] == host_neg[:4] == "NOT " and rows_of(neg[4:]) == rows_of(host_neg[4:])


def test_gpu_row_floor_and_byte_ceiling(kb, monkeypatch):
    from das_amd.database.hip_db import HipDB
    ans = ask(kb, L("R65", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    dev = ans.text()
    for attr, value in (("QUERY_TEXT_MIN", 66), ("QUERY_TEXT_MAX_BYTES", len(dev) - 1)):
        monkeypatch.setattr(HipDB, attr, value)
        before = dict(kb.query_text_stats)
        assert rows_of(fresh_text(ans)) == rows_of(dev)
        assert kb.query_text_stats == {"device": before["device"], "host": before["host"] + 1}
        monkeypatch.setattr(HipDB, attr, {"QUERY_TEXT_MIN": 65, "QUERY_TEXT_MAX_BYTES": len(dev)}[attr])
        assert fresh_text(ans) == dev
        assert kb.query_text_stats == {"device": before["device"] + 1, "host": before["host"] + 1}


# ---- 7. errors --------------------------------------------------------------

def test_gpu_value_that_is_no_atom(kb):
    from das_amd.pattern_matcher import pattern_matcher as pm
    n_atoms = int(kb.ctx.stats().n_atoms)
    v = pm._vid("Vbad")
    t = kb.ctx.table_from_host(_lib.TABLE_ORDERED, (v,), np.array([[0, n_atoms, 1]], dtype=np.uint32))
    lits = pm.row_literals(["Vbad"])
    size = _lib.rows_text_size(lits, SEP, 3)
    for cap in (size, 20):
        out = np.full(size + 32, 0xEE, dtype=np.uint8)
        data, total, bad = kb.ctx.rows_text(t, lits, SEP, cap=cap, out=out)
        assert bad == 1 and total == size and np.all(out[cap:] == 0xEE)
    good = kb.ctx.table_from_host(_lib.TABLE_ORDERED, (v,), np.array([[0, n_atoms - 1, 1]], dtype=np.uint32))
    assert kb.ctx.rows_text(good, lits, SEP)[2] == 0


def test_gpu_row_limit(kb, monkeypatch):
    from das_amd.pattern_matcher import pattern_matcher as pm
    base = len(repr({"": "0" * 32})) + len(SEP)
    fits, beyond = "n" * (_lib.ROWS_TEXT_MAX_ROW - base), "n" * (_lib.ROWS_TEXT_MAX_ROW - base + 1)
    for name, ok in ((fits, True), (beyond, False)):
        ans = ask(kb, L("R3", V(name), ["Node", "Concept", "a1"], ["Node", "Concept", "c0"]), monkeypatch,
                  DAS_DEFER_JOIN="0")
        t, = ans._rel.tables
        lits = pm.row_literals([name])
        rc = _raw(kb, t, 0, t.nrows, lits)
        before = dict(kb.query_text_stats)
        text = ans.text()
        assert text == "{" + ", ".join(model_rows(kb, t)) + "}" and t.nrows == 1
        if ok:
            assert rc == 0 and kb.query_text_stats["device"] == before["device"] + 1
        else:
            assert rc == _lib.ERR_LIMIT and b"DAS_ROWS_TEXT_MAX_ROW" in _lib.lib().das_last_error(kb.ctx.h)
            assert kb.ctx.rows_text(t, lits, SEP) is None
            assert kb.query_text_stats == {"device": before["device"], "host": before["host"] + 1}


def _raw(db, t, row0, nrows, lits, off=None):
    """The status of the C call itself."""
    lit = np.frombuffer(b"".join(lits) or b"\0", dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(x) for x in lits])])
    off = np.asarray(off, dtype=np.uint32)
    sep = np.frombuffer(SEP, dtype=np.uint8)
    out = np.zeros(1 << 16, dtype=np.uint8)
    total, bad = C.c_uint64(), C.c_uint64()
    return _lib.lib().das_table_rows_text(db.ctx.h, t.h, row0, nrows, _lib.ptr(lit), _lib.ptr(off), _lib.ptr(sep),
                                          len(SEP), _lib.ptr(out), out.size, C.byref(total), C.byref(bad))


def test_gpu_abi_refusals(kb, monkeypatch):
    from das_amd.pattern_matcher import pattern_matcher as pm
    ans = ask(kb, L("R65", V("Va"), V("Vc")), monkeypatch, DAS_DEFER_JOIN="0")
    t, = ans._rel.tables
    lits = pm.row_literals(names_of(t))
    assert _raw(kb, t, 0, 65, lits) == 0 and _raw(kb, t, 65, 0, lits) == 0
    assert _raw(kb, t, 0, 66, lits) == _lib.ERR_INVALID          # the window ends past the table
    assert _raw(kb, t, 66, 0, lits) == _lib.ERR_INVALID
    assert _raw(kb, t, 1, 2 ** 64 - 1, lits) == _lib.ERR_INVALID   # row0 + nrows wraps
    assert _raw(kb, t, 0, 65, lits, off=[0, 9, 8, 21]) == _lib.ERR_INVALID
    assert b"ascending" in _lib.lib().das_last_error(kb.ctx.h)
    with pytest.raises(ValueError, match="rows out of range"):
        kb.ctx.rows_text(t, lits, SEP, row0=60, nrows=6)
    with pytest.raises(ValueError, match="one literal piece more"):
        kb.ctx.rows_text(t, lits[:2], SEP)
    cols = np.arange(12, dtype=np.uint32).reshape(2, 6)
    for kind, members in ((_lib.TABLE_UNORDERED, None), (_lib.TABLE_COMPOSITE, (0, 0))):
        other = kb.ctx.table_from_host(kind, t.vars, cols, members=members)
        with pytest.raises(ValueError, match="ORDERED"):
            kb.ctx.rows_text(other, lits, SEP)
    # any literals: the call knows no format
    data, total, bad = kb.ctx.rows_text(t, [b"", b"\t", b"\n"], b"", row0=2, nrows=2)
    hexes = [kb.hex_of(c) for c in t.fetch(2, 2)]
    assert bytes(data).decode() == "".join(f"{a}\t{b}\n" for a, b in zip(*hexes)) and total == 2 * 66
