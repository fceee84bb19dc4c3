"""The deferred cross product: a plan's root And whose last
fold shares no variable leaves its two factors in place of its rows, and the
rows are expanded when something reads them.

Every case runs with DAS_DEFER_PRODUCT=1 (deferred, no size floor) against
DAS_DEFER_PRODUCT=0 (the product written by the plan), through
das_plan_execute and das_plan_execute_many.  The KB is tiny, so DAS_FUSED=0
keeps the one-launch And chain (which would answer these Ands whole) out of
the way and the folds go through join().

Link types of the KB, n in SIZES: A<n> holds n links (c_i, c_{3i+1}), W<n>
n links (c_i, c_{i+1}, c_{i+2}), U<n> n links (hub, c_i) -- two-, three- and,
with the hub grounded, one-variable terms of n rows each."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import das_oracle as O
from tests.util import build, record, same

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 7, 65)
N_NODES = 70
WORDS = 51


@pytest.fixture(scope="module")
def kb():
    from das_amd import loader
    from das_amd.database.hip_db import HipDB
    b = loader.AtomBuilder()
    c = [b.terminal("Concept", f"c{i}", True) for i in range(N_NODES)]
    hub = b.terminal("Concept", "hub", True)
    for n in SIZES:
        for i in range(n):
            b.expr(f"A{n}", [c[i], c[(3 * i + 1) % N_NODES]])
            b.expr(f"W{n}", [c[i], c[i + 1], c[i + 2]])
            b.expr(f"U{n}", [hub, c[i]])
    arrays = b.finish()
    db = HipDB(device=0)
    db.load_arrays(arrays)
    return arrays, db


def V(x):
    return ["Var", x]


def term(width, n, vs):
    """A Link term of `width` variables (vs) and n rows."""
    if width == 1:
        return ["Link", f"U{n}", True, [["Node", "Concept", "hub"], V(vs[0])]]
    return ["Link", f"{'A' if width == 2 else 'W'}{n}", True, [V(v) for v in vs[:width]]]


def product_spec(n1, n2, w1, w2):
    return ["And", [term(w1, n1, ["V1", "V2", "V3"]), term(w2, n2, ["V4", "V5", "V6"])]]


# (rows of the first term, of the second, their widths): total % 4 = 1, 1, 1,
# 0, 1, 2, 2 and, with the slices' first rows, every quad offset; both operand
# orders (the larger side is the probe); output widths 2..6
SHAPES = [(1, 1, 1, 1), (1, 5, 1, 2), (5, 1, 2, 2), (3, 4, 2, 3), (7, 3, 3, 3), (65, 2, 2, 1), (2, 65, 1, 3)]
# the generic kernel (7 columns): W3 |x| A7 on V3 (3 rows, 4 columns), then x W5
SPEC7 = ["And", [term(3, 3, ["V1", "V2", "V3"]), term(2, 7, ["V3", "V4"]), term(3, 5, ["V5", "V6", "V7"])]]
SPEC7_FACTORS = (3, 5)


def salts(t):
    return [int.from_bytes(hashlib.md5(b"v%d" % v).digest()[:8], "little") for v in t.vars]


def run(db, spec, monkeypatch, defer, many=False, no_overload=False, sharded=False):
    """The plan's ordered answer tables with DAS_DEFER_PRODUCT=`defer` (None: unset)."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    monkeypatch.setenv("DAS_FUSED", "0")
    if defer is None:
        monkeypatch.delenv("DAS_DEFER_PRODUCT", raising=False)
    else:
        monkeypatch.setenv("DAS_DEFER_PRODUCT", defer)
    words = pm._lower(build(spec), db, no_overload)
    assert words is not None
    n = len(words) // WORDS
    if sharded:
        matched, _, tables, _ = db.ctx.plan_execute_sharded(words, n, [], no_overload)
    elif many:
        other = pm._lower(build(term(2, 3, ["V1", "V2"])), db, no_overload)
        matched, _, tables = db.ctx.plan_execute_many([(words, n), (other, len(other) // WORDS)], no_overload)[0]
    else:
        matched, _, tables = db.ctx.plan_execute(words, n, no_overload)
    assert matched
    return tables


def one(tables):
    assert len(tables) == 1
    return tables[0]


class Prof:
    """k_cartesian launches recorded between enter and read()."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.prof_enable(True)
        self.ctx.prof_reset()
        return self

    def read(self):
        self.ctx.sync()
        n = sum(v["launches"] for k, v in self.ctx.prof_stats().items() if k.startswith("k_cartesian"))
        self.ctx.prof_reset()
        return n

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


def check_equal(d, e, nbuild):
    """Deferred table d against eager table e: schema, checksum, rows, slices."""
    assert info(d) == info(e)
    assert d.schema == e.schema and d.nrows == e.nrows
    assert d.bounds() == e.bounds()
    assert d.checksum(salts(d)) == e.checksum(salts(e))
    full = e.fetch()
    total = e.nrows
    assert np.array_equal(d.fetch(), full)
    for row0 in sorted({0, 1, 3, nbuild - 1, nbuild, nbuild + 1, total - 1}):
        if not 0 <= row0 < total:
            continue
        for n in sorted({1, 2, 5, total - row0}):
            if row0 + n > total:
                continue
            assert np.array_equal(d.fetch(row0, n), full[:, row0:row0 + n]), (row0, n)


@pytest.mark.parametrize("many", [False, True], ids=["execute", "execute_many"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_deferred_equals_eager(kb, monkeypatch, shape, many):
    _, db = kb
    n1, n2, w1, w2 = shape
    spec = product_spec(n1, n2, w1, w2)
    e = one(run(db, spec, monkeypatch, "0", many))
    with Prof(db.ctx) as p:
        d = one(run(db, spec, monkeypatch, "1", many))
        assert p.read() == 0                  # the plan launched no product
        assert len(d.vars) == w1 + w2 and d.nrows == n1 * n2
        check_equal(d, e, min(n1, n2))


@pytest.mark.parametrize("many", [False, True], ids=["execute", "execute_many"])
def test_gpu_deferred_seven_columns(kb, monkeypatch, many):
    _, db = kb
    e = one(run(db, SPEC7, monkeypatch, "0", many))
    with Prof(db.ctx) as p:
        d = one(run(db, SPEC7, monkeypatch, "1", many))
        assert p.read() == 0
    assert len(d.vars) == 7 and d.nrows == SPEC7_FACTORS[0] * SPEC7_FACTORS[1]
    check_equal(d, e, min(SPEC7_FACTORS))


def test_gpu_deferred_matches_oracle(kb, monkeypatch):
    arrays, db = kb
    odb = O.RedisMongoSemantics(O.KB.from_arrays(arrays))
    monkeypatch.setenv("DAS_FUSED", "0")
    monkeypatch.setenv("DAS_DEFER_PRODUCT", "1")
    for spec in (product_spec(7, 3, 3, 3), SPEC7):
        want = O.evaluate(spec, odb)
        assert want["n"] > 1
        assert same(record(spec, db), want)


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


RESOLVERS = {
    "export_rows": lambda db, t: _export(db, t),
    "column": lambda db, t: np.stack([_column(db, t, c) for c in range(len(t.vars))]),
    "join": lambda db, t: _rows_sorted(db.ctx.join(t, db.ctx.gather(t, [0, 2, 5]))),
    "join_right": lambda db, t: _rows_sorted(db.ctx.join(db.ctx.gather(t, [1, 4]), t)),
    "dedup": lambda db, t: _rows_sorted(db.ctx.dedup(t)),
    "gather": lambda db, t: db.ctx.gather(t, [20, 0, 3, 7, 7]).fetch(),
    "gather_ranges": lambda db, t: db.ctx.gather_ranges(t, [2, 9], [6, 21]).fetch(),
}


@pytest.mark.parametrize("op", sorted(RESOLVERS))
def test_gpu_deferred_resolves_on_use(kb, monkeypatch, op):
    """Calls that need the rows expand them, once; the handle then answers as before."""
    _, db = kb
    spec = product_spec(7, 3, 3, 3)
    e = one(run(db, spec, monkeypatch, "0"))
    want = RESOLVERS[op](db, e)
    with Prof(db.ctx) as p:
        d = one(run(db, spec, monkeypatch, "1"))
        before = (info(d), d.checksum(salts(d)), d.fetch())
        assert p.read() == 1                              # the fetch's slice launch; the table stays deferred
        got = RESOLVERS[op](db, d)
        assert p.read() == 1                              # the first resolving call: one product
        assert np.array_equal(got, want)
        assert np.array_equal(RESOLVERS[op](db, d), want)
        assert p.read() == 0                              # the second: none
        assert info(d) == before[0] and d.checksum(salts(d)) == before[1]
        assert np.array_equal(d.fetch(), before[2]) and np.array_equal(d.fetch(), e.fetch())
        assert d.fetch(5, 9).tolist() == before[2][:, 5:14].tolist()
        assert p.read() == 0


def test_gpu_deferred_names(kb, monkeypatch):
    """names() of a deferred answer: the node names of the eager one, and the
    answer's count, checksum and rows stay what they were."""
    from das_amd.pattern_matcher import pattern_matcher as pm
    _, db = kb
    spec = product_spec(7, 3, 3, 3)
    monkeypatch.setenv("DAS_FUSED", "0")
    got = {}
    for defer in ("0", "1"):
        monkeypatch.setenv("DAS_DEFER_PRODUCT", defer)
        ans = pm.PatternMatchingAnswer()
        assert build(spec).matched(db, ans)
        t = one([x for x in db.rel_local_tables(ans._relation()) if x.nrows])
        before = (ans.count(), t.checksum(salts(t)), t.fetch())
        on_device = db.name_fetch_stats["device"]
        names = [ans.names(v) for v in ("V1", "V5")] + [ans.names()]
        assert db.name_fetch_stats["device"] > on_device      # das_node_names read the table's columns
        assert (ans.count(), t.checksum(salts(t))) == before[:2] and np.array_equal(t.fetch(), before[2])
        got[defer] = (names, before[0], before[1], before[2].tolist())
    assert got["0"] == got["1"]
    assert got["1"][1] == 21 and sorted(set(got["1"][0][0])) == [f"c{i}" for i in range(7)]


NOT_DEFERRED = {
    # the product A3 x A4 is then joined with A7 on V4
    "term_follows": (["And", [term(2, 3, ["V1", "V2"]), term(2, 4, ["V3", "V4"]), term(2, 7, ["V4", "V5"])]], {}),
    "not_follows": (["And", [term(2, 3, ["V1", "V2"]), term(2, 4, ["V3", "V4"]),
                             ["Not", term(2, 7, ["V1", "V4"])]]], {}),
    "not_before": (["And", [term(2, 3, ["V1", "V2"]), ["Not", term(2, 7, ["V1", "V4"])],
                            term(2, 4, ["V3", "V4"])]], {}),
    "inside_or": (["Or", [product_spec(3, 4, 2, 2), product_spec(2, 5, 2, 2)]], {}),
    "no_overload": (product_spec(7, 5, 2, 2), {"no_overload": True}),
    "below_floor_unset": (product_spec(7, 3, 3, 3), {"defer": None}),
    "sharded": (product_spec(7, 3, 3, 3), {"sharded": True}),
}


@pytest.mark.parametrize("case", sorted(NOT_DEFERRED))
def test_gpu_product_not_deferred(kb, monkeypatch, case):
    """Where something still reads the product's rows inside the plan (or the
    switch says no), the plan writes them: the eager result, and a
    k_cartesian scope while the plan runs."""
    _, db = kb
    spec, kw = NOT_DEFERRED[case]
    kw = dict(kw)
    defer = kw.pop("defer", "1")
    for many in ((False,) if kw.get("sharded") else (False, True)):
        e = run(db, spec, monkeypatch, "0", many=many, **kw)
        with Prof(db.ctx) as p:
            d = run(db, spec, monkeypatch, defer, many=many, **kw)
            assert p.read() >= 1
            assert [t.schema for t in d] == [t.schema for t in e]
            for x, y in zip(d, e):
                assert x.nrows == y.nrows and x.checksum(salts(x)) == y.checksum(salts(y))
                assert np.array_equal(x.fetch(), y.fetch())
            assert p.read() == 0
    if case == "no_overload":
        assert 0 < one(e).nrows < 35                      # rows with one atom under two variables dropped
    if case == "not_follows":
        assert 0 < one(e).nrows < 12                      # the filter removed rows
