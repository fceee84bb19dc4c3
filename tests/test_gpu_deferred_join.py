"""Deferred index-join expansions and scan views: a plan's
root And whose last fold is an index join through its count pass (k_ij_lc)
leaves the probe rows and the counts in place of its rows, a large scan that
is a range of index columns stays a view of them, and the rows are written
when something reads them -- or when the index they read is rebuilt.

Every case runs with DAS_DEFER_JOIN=1 (deferred, no size floors) against
DAS_DEFER_JOIN=0 (the rows written by the plan), through das_plan_execute and
das_plan_execute_many.  DAS_FUSED=0 keeps the one-launch And chain out of the
way, DAS_REV_IJ=1 drops the reverse index join's size floor, DAS_IJ_MID=0
sends probes above 2048 rows (kIjSmall) through k_ij_lc, and
DAS_DJ_BALANCED=0|1 picks the expansion kernel.

The KB.  M holds 11000 links (g, b): (g_i, b_0) for i < 6000 -- b_0 owns
most rows of a join keyed by b --, (g_i, b_{1 + i % 50}) for i < 3000, and
(g_5, x_j) for j < 2000 -- g_5 owns most rows of a join keyed by g.  For n in
PROBES (2049 = kIjSmall + 1 rows, then 127, 128 and 129 more: one expansion
unit is kXRows = 128 probe rows), I<n> holds n links (b_{k % 64}, p_k): the
probe of the reverse fold, b_51 .. b_63 without a partner in M; U<n> holds n
links (g_{5k}, hub): the probe of the forward fold, g_9000 and up without a
partner.  Wa / Wb (WIDE rows each) join 1:1 into a 5-column probe.

sorted_col has no accessor at the C ABI; the deferred path sets it on the
same lines of index_join as the eager one."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.util import build

pytestmark = pytest.mark.gpu

PROBES = (2049, 2176, 2177, 2178)
WIDE = 2177
WORDS = 51
N_G = 5 * PROBES[-1] + 8


def _arrays():
    from das_amd import loader
    b = loader.AtomBuilder()
    node = lambda name: b.terminal("Concept", name, True)  # noqa: E731
    g = [node(f"g{i}") for i in range(N_G)]
    bp = [node(f"b{i}") for i in range(64)]
    x = [node(f"x{i}") for i in range(2000)]
    p = [node(f"p{i}") for i in range(PROBES[-1])]
    a = [node(f"a{i}") for i in range(WIDE + 2)]
    k = [node(f"k{i}") for i in range(WIDE)]
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
    for i in range(WIDE):
        b.expr("Wa", [a[i], a[i + 1], k[i]])
        b.expr("Wb", [k[i], a[i + 2], g[5 * i]])
    for i in range(7):
        b.expr("A7", [p[i], a[i]])
    return b.finish()


def _small_arrays():
    from das_amd import loader
    b = loader.AtomBuilder()
    c = [b.terminal("Concept", f"c{i}", True) for i in range(9)]
    for i in range(8):
        b.expr("S", [c[i], c[i + 1]])
    return b.finish()


@pytest.fixture(scope="module")
def arrays():
    return _arrays()


@pytest.fixture(scope="module")
def kb(arrays):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(arrays)
    return db


def V(x):
    return ["Var", x]


def L(name, *targets):
    return ["Link", name, True, list(targets)]


HUB = ["Node", "Concept", "hub"]
M_SCAN = L("M", V("Vg"), V("Vb"))


def reverse_spec(n):
    """reverse_ij: I<n>'s rows (2 columns) expand M's ranges by b -- <2,1>."""
    return ["And", [M_SCAN, L(f"I{n}", V("Vb"), V("Vp"))]]


def forward_spec(n):
    """step()'s index join: U<n>'s rows (1 column) expand M's ranges by g -- <1,1>."""
    return ["And", [L(f"U{n}", V("Vg"), HUB), M_SCAN]]


# a 5-column probe (Wa |x| Wb on V3, written by the plan) index-joined with M
# by g: the 4 + 1 column slices of the write
WIDE_SPEC = ["And", [L("Wa", V("V1"), V("V2"), V("V3")), L("Wb", V("V3"), V("V4"), V("Vg")), M_SCAN]]

SPECS = {"reverse": reverse_spec, "forward": forward_spec}


def salts(t):
    return [int.from_bytes(hashlib.md5(b"v%d" % v).digest()[:8], "little") for v in t.vars]


def run(db, spec, monkeypatch, defer, many=False, no_overload=False, sharded=False, balanced="0"):
    """The plan's answer tables with DAS_DEFER_JOIN=`defer` (None: unset).
    no_overload is given to the plan call alone: lowered with it, a Link
    carries no index join at all (pattern_matcher._link_record), and the
    plan's own guard against deferring under it would never be reached."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    for k, v in (("DAS_FUSED", "0"), ("DAS_REV_IJ", "1"), ("DAS_IJ_MID", "0"), ("DAS_DJ_BALANCED", balanced)):
        monkeypatch.setenv(k, v)
    if defer is None:
        monkeypatch.delenv("DAS_DEFER_JOIN", raising=False)
    else:
        monkeypatch.setenv("DAS_DEFER_JOIN", defer)
    words = pm._lower(build(spec), db, False)
    assert words is not None
    n = len(words) // WORDS
    if sharded:
        matched, _, tables, _ = db.ctx.plan_execute_sharded(words, n, [], no_overload)
    elif many:
        other = pm._lower(build(L("A7", V("V1"), V("V2"))), db, False)
        matched, _, tables = db.ctx.plan_execute_many([(words, n), (other, len(other) // WORDS)], no_overload)[0]
    else:
        matched, _, tables = db.ctx.plan_execute(words, n, no_overload)
    assert matched
    return tables


def one(tables):
    assert len(tables) == 1
    return tables[0]


class Prof:
    """Launches recorded between enter and read(): (k_dj_write*, k_project + k_copy_*)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.prof_enable(True)
        self.ctx.prof_reset()
        return self

    def read(self):
        self.ctx.sync()
        st = self.ctx.prof_stats()
        w = sum(v["launches"] for k, v in st.items() if k.startswith("k_dj_write"))
        c = sum(v["launches"] for k, v in st.items() if k.startswith(("k_project", "k_copy_")))
        self.ctx.prof_reset()
        return w, c

    def __exit__(self, *exc):
        self.ctx.prof_enable(False)
        self.ctx.prof_reset()


def info(t):
    """(kind, vars, nrows) as das_table_info reports them now."""
    from das_amd import _lib
    kind, ncols, nrows = C.c_int32(), C.c_int32(), C.c_uint64()
    vars_ = (C.c_int32 * 16)()
    _lib.check(_lib.lib().das_table_info(t.h, C.byref(kind), C.byref(ncols), vars_, C.byref(nrows)))
    return kind.value, tuple(vars_[i] for i in range(ncols.value)), nrows.value


def members(t):
    from das_amd import _lib
    mem = (C.c_int32 * 16)()
    _lib.check(_lib.lib().das_table_members(t.h, mem))
    return tuple(mem[i] for i in range(len(t.vars)))


def check_equal(d, e):
    """Unresolved table d against written table e; the metadata first (it
    settles nothing), then the checksum and the rows in order."""
    assert info(d) == info(e) and members(d) == members(e)
    assert d.schema == e.schema and d.nrows == e.nrows
    assert d.bounds() == e.bounds()
    assert d.checksum(salts(d)) == e.checksum(salts(e))
    assert np.array_equal(d.fetch(), e.fetch())


_EAGER = {}


def eager(db, spec, monkeypatch, key, many=False, balanced="0"):
    """The written answer of `spec`, computed once per (key, entry point, kernel)."""
    k = (key, many, balanced)
    if k not in _EAGER:
        _EAGER[k] = one(run(db, spec, monkeypatch, "0", many, balanced=balanced))
    return _EAGER[k]


@pytest.mark.parametrize("balanced", ["0", "1"], ids=["units", "balanced"])
@pytest.mark.parametrize("many", [False, True], ids=["execute", "execute_many"])
@pytest.mark.parametrize("n", PROBES)
@pytest.mark.parametrize("fold", sorted(SPECS))
def test_gpu_deferred_join_equals_eager(kb, monkeypatch, fold, n, many, balanced):
    spec = SPECS[fold](n)
    e = eager(kb, spec, monkeypatch, (fold, n), many, balanced)
    with Prof(kb.ctx) as p:
        d = one(run(kb, spec, monkeypatch, "1", many, balanced=balanced))
        assert p.read()[0] == 0                   # the plan launched no expansion write
        assert len(d.vars) == (3 if fold == "reverse" else 2) and d.nrows == e.nrows > n
        assert info(d) == info(e) and d.bounds() == e.bounds() and members(d) == members(e)
        assert p.read() == (0, 0)                 # info, bounds and members settle nothing
        check_equal(d, e)
        assert p.read()[0] == 1                   # the one write, made by the first read


@pytest.mark.parametrize("balanced", ["0", "1"], ids=["units", "balanced"])
@pytest.mark.parametrize("many", [False, True], ids=["execute", "execute_many"])
def test_gpu_deferred_join_wide(kb, monkeypatch, many, balanced):
    e = eager(kb, WIDE_SPEC, monkeypatch, "wide", many, balanced)
    with Prof(kb.ctx) as p:
        d = one(run(kb, WIDE_SPEC, monkeypatch, "1", many, balanced=balanced))
        inside = p.read()[0]                      # (the first fold's direct join is written by the plan)
        assert len(d.vars) == 6 and d.nrows == e.nrows > WIDE
        check_equal(d, e)
        assert p.read()[0] == 2                   # 4 + 1 probe columns: two slices of the one expansion
    with Prof(kb.ctx) as p:
        one(run(kb, WIDE_SPEC, monkeypatch, "0", many, balanced=balanced))
        assert p.read()[0] == inside + 2


NOT_DEFERRED = {
    # A7's 7 rows are joined to the index join's output by a direct join
    "term_follows": (["And", [M_SCAN, L("I2049", V("Vb"), V("Vp")), L("A7", V("Vp"), V("Va"))]], {}),
    "not_follows": (["And", [M_SCAN, L("I2049", V("Vb"), V("Vp")), ["Not", L("A7", V("Vp"), V("Vg"))]]], {}),
    "not_before": (["And", [M_SCAN, ["Not", L("A7", V("Vp"), V("Vg"))], L("I2049", V("Vb"), V("Vp"))]], {}),
    # (a Not of anything but an index-joinable Link is scanned and antijoined)
    "not_follows_scanned": (["And", [L("U2049", V("Vg"), HUB), M_SCAN, ["Not", ["And", [L("A7", V("Vg"), V("Vb"))]]]]],
                            {}),
    "inside_or": (["Or", [reverse_spec(2049), reverse_spec(2176)]], {}),
    "no_overload": (forward_spec(2049), {"no_overload": True}),
    "floors_unset": (reverse_spec(2049), {"defer": None}),
    "sharded": (forward_spec(2049), {"sharded": True}),
}


@pytest.mark.parametrize("case", sorted(NOT_DEFERRED))
def test_gpu_join_not_deferred(kb, monkeypatch, case):
    """Where something still reads the join's rows inside the plan (or the
    switch and its floors say no), the plan writes them: the eager result, and
    the eager plan's k_dj_write launches while the plan runs."""
    spec, kw = NOT_DEFERRED[case]
    kw = dict(kw)
    defer = kw.pop("defer", "1")
    for many in ((False,) if kw.get("sharded") else (False, True)):
        with Prof(kb.ctx) as p:
            e = run(kb, spec, monkeypatch, "0", many=many, **kw)
            want = p.read()[0]
            assert want >= 1
            d = run(kb, spec, monkeypatch, defer, many=many, **kw)
            assert p.read()[0] == want
            assert [t.schema for t in d] == [t.schema for t in e] and len(d) >= 1
            for x, y in zip(d, e):
                assert x.nrows == y.nrows and x.bounds() == y.bounds()
                assert x.checksum(salts(x)) == y.checksum(salts(y))
                assert np.array_equal(x.fetch(), y.fetch())
            assert p.read() == (0, 0)


def _rows_sorted(t):
    r = t.fetch().T
    return r[np.lexsort(r.T[::-1])]


def _export(db, t):
    import torch
    buf = torch.empty((int(t.nrows), len(t.vars)), dtype=torch.int32, device=torch.device("cuda", db.ctx.device))
    torch.cuda.synchronize()
    db.ctx.export_rows(t, buf.data_ptr())
    db.ctx.sync()
    return buf.cpu().numpy()


class _DevColumn:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def _column(db, t, c):
    """Column c read through the device pointer das_table_column gives."""
    import torch
    from das_amd import _lib
    p = C.c_void_p()
    assert _lib.lib().das_table_column(t.h, c, C.byref(p)) == 0 and p.value
    db.ctx.sync()
    col = torch.as_tensor(_DevColumn(p.value, int(t.nrows)), device=torch.device("cuda", db.ctx.device))
    return col.cpu().numpy()


def _columns(db, t):
    return np.stack([_column(db, t, c) for c in range(len(t.vars))])


def _join_with(db, small_rows):
    """das_join of a table with four given rows of its own schema."""
    return lambda _, t: _rows_sorted(db.ctx.join(t, db.ctx.table_from_host(0, t.vars, small_rows)))


RESOLVERS = {
    "fetch": lambda db, t: t.fetch(3, 700),
    "column": _columns,
    "checksum": lambda db, t: np.asarray(t.checksum(salts(t)), dtype=np.uint64),
    "export_rows": _export,
    "dedup": lambda db, t: _rows_sorted(db.ctx.dedup(t)),
}


@pytest.mark.parametrize("op", sorted(RESOLVERS) + ["join"])
def test_gpu_deferred_join_settles_once(kb, monkeypatch, op):
    """A call that needs a deferred expansion's rows writes them, once: it
    launches one k_dj_write more than the same call on the written answer,
    and the second call launches what that one does."""
    spec = reverse_spec(2177)
    e = eager(kb, spec, monkeypatch, ("reverse", 2177))
    f = _join_with(kb, e.fetch()[:, 5:9]) if op == "join" else RESOLVERS[op]
    with Prof(kb.ctx) as p:
        want = f(kb, e)
        base = p.read()[0]
        d = one(run(kb, spec, monkeypatch, "1"))
        assert p.read()[0] == 0                   # the plan: no write
        before = (info(d), d.bounds(), members(d))
        assert p.read() == (0, 0)                 # the metadata calls: no write, no copy
        got = f(kb, d)
        assert p.read()[0] == base + 1            # the first call that needs the rows: the one write
        assert np.array_equal(got, want)
        assert np.array_equal(f(kb, d), want)
        assert p.read()[0] == base                # the second: none
        assert (info(d), d.bounds(), members(d)) == before
        check_equal(d, e)
        assert p.read()[0] == 0


def scan_view(db, monkeypatch, defer, through):
    """M's scan as an answer: das_scan_link's, or a lone Link plan's."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    monkeypatch.setenv("DAS_DEFER_JOIN", defer)
    if through == "scan_link":
        args, dedup = db.link_scan_spec("M", ["*", "*"], [pm._vid("Vg"), pm._vid("Vb")], True)
        assert not dedup
        return db.ctx.scan_link(*args)
    return one(run(db, M_SCAN, monkeypatch, defer))


@pytest.mark.parametrize("through", ["scan_link", "plan"])
def test_gpu_scan_view_equals_copy(kb, monkeypatch, through):
    """A scan answer left a view of the index: metadata and fetch read it in
    place, the first call that takes its columns copies them, once."""
    e = scan_view(kb, monkeypatch, "0", through)
    ncols = len(e.vars)
    with Prof(kb.ctx) as p:
        d = scan_view(kb, monkeypatch, "1", through)
        assert d.nrows == e.nrows == 11000
        assert info(d) == info(e) and d.bounds() == e.bounds() and members(d) == members(e)
        assert np.array_equal(d.fetch(), e.fetch()) and np.array_equal(d.fetch(7, 100), e.fetch(7, 100))
        assert p.read() == (0, 0)                 # no copy so far
        assert np.array_equal(_columns(kb, d), e.fetch())
        assert p.read() == (0, ncols)             # settled: one copy per column
        assert np.array_equal(_columns(kb, d), e.fetch())
        assert p.read() == (0, 0)
        check_equal(d, e)


@pytest.mark.parametrize("op", ["checksum", "dedup", "export_rows", "join"])
def test_gpu_scan_view_settles_once(kb, monkeypatch, op):
    e = scan_view(kb, monkeypatch, "0", "scan_link")
    f = _join_with(kb, e.fetch()[:, 5:9]) if op == "join" else RESOLVERS[op]
    want = f(kb, e)
    with Prof(kb.ctx) as p:
        d = scan_view(kb, monkeypatch, "1", "scan_link")
        assert p.read() == (0, 0)
        assert np.array_equal(f(kb, d), want)
        p.read()
        _columns(kb, d)
        assert p.read() == (0, 0)                 # the call settled it: its columns are its own already
        assert np.array_equal(f(kb, d), want)


# ---- lifetime: ordinary sequences of answers, frees and index rebuilds ----

@pytest.fixture()
def fresh(arrays):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(arrays)
    yield db


def _answers(db, monkeypatch, defer):
    return one(run(db, reverse_spec(2177), monkeypatch, defer)), scan_view(db, monkeypatch, defer, "scan_link")


def _small_query(db, monkeypatch):
    t = one(run(db, L("S", V("V1"), V("V2")), monkeypatch, "1"))
    assert t.nrows == 8
    return t.fetch()


def test_gpu_rebuild_while_answers_live(fresh, monkeypatch):
    """The index is rebuilt under a deferred join answer and a scan view: both
    then read the rows the old index gave."""
    ej, ev = _answers(fresh, monkeypatch, "0")
    want_j, want_v = ej.fetch(), ev.fetch()
    with Prof(fresh.ctx) as p:
        dj, dv = _answers(fresh, monkeypatch, "1")
        assert p.read()[0] == 0
        fresh.load_arrays(_small_arrays())
        assert p.read()[0] == 1                   # the rebuild settled the join (and copied the view)
        assert np.array_equal(dj.fetch(), want_j) and np.array_equal(dv.fetch(), want_v)
        assert np.array_equal(_columns(fresh, dj), want_j) and np.array_equal(_columns(fresh, dv), want_v)
        assert dj.checksum(salts(dj)) == ej.checksum(salts(ej))
        assert p.read()[0] == 0                   # settled once
    assert _small_query(fresh, monkeypatch).shape == (2, 8)


def test_gpu_free_before_rebuild(fresh, monkeypatch):
    with Prof(fresh.ctx) as p:
        dj, dv = _answers(fresh, monkeypatch, "1")
        dj.free()
        dv.free()
        fresh.load_arrays(_small_arrays())
        assert p.read()[0] == 0                   # nothing was left to settle
    assert _small_query(fresh, monkeypatch).shape == (2, 8)


def test_gpu_free_after_rebuild(fresh, monkeypatch):
    dj, dv = _answers(fresh, monkeypatch, "1")
    fresh.load_arrays(_small_arrays())
    dj.free()
    dv.free()
    assert _small_query(fresh, monkeypatch).shape == (2, 8)


def test_gpu_two_deferred_answers(fresh, monkeypatch):
    """Two deferred answers alive at once, read in the other order, one of
    them across a rebuild."""
    e1 = one(run(fresh, reverse_spec(2049), monkeypatch, "0"))
    e2 = one(run(fresh, forward_spec(2178), monkeypatch, "0"))
    want1, want2 = e1.fetch(), e2.fetch()
    d1 = one(run(fresh, reverse_spec(2049), monkeypatch, "1"))
    d2 = one(run(fresh, forward_spec(2178), monkeypatch, "1"))
    assert np.array_equal(d2.fetch(), want2)
    fresh.load_arrays(_small_arrays())
    assert np.array_equal(d1.fetch(), want1) and np.array_equal(d2.fetch(), want2)


def test_gpu_deferred_answer_across_rebuild(fresh, monkeypatch, arrays):
    """An answer kept across a rebuild, a query on the new index, a rebuild
    back, and the same query again."""
    want = one(run(fresh, reverse_spec(2176), monkeypatch, "0")).fetch()
    d = one(run(fresh, reverse_spec(2176), monkeypatch, "1"))
    fresh.load_arrays(_small_arrays())
    assert _small_query(fresh, monkeypatch).shape == (2, 8)
    fresh.load_arrays(arrays)
    d2 = one(run(fresh, reverse_spec(2176), monkeypatch, "1"))
    assert np.array_equal(d2.fetch(), want) and np.array_equal(d.fetch(), want)
