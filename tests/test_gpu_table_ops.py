"""The binding-table operators of query.hip / composite.hip, one by one
through the C ABI, against the host model (tests/table_model.py) on the case
tables of tests/table_cases.py -- the cases test_table_model.py admits.

Row order is compared exactly where the operator's header promises one
(concat, gather, gather_ranges, set_dedup, set_minus, antijoin, partition
inside a destination), as a sorted multiset elsewhere (join, dedup); the
schema (kind, vars, members) always; and after every operator call the
result's column bounds must contain its values."""
import numpy as np
import pytest

from tests import table_cases as TC
from tests import table_model as TM
from tests.table_model import ORDERED, NTable

pytestmark = pytest.mark.gpu

_case = dict(ids=lambda c: c.id)
SET_SORT = ["unset", "1"]


@pytest.fixture(scope="module")
def db():
    from das_amd.database.hip_db import HipDB
    d = HipDB(device=0)
    d.load_arrays(TC.kb_arrays())
    return d


@pytest.fixture(scope="module")
def ctx(db):
    n = int(db.ctx.stats().n_atoms)
    assert n >= 8192 and n == TC.n_atoms()        # the generators' `hi`: every value is an atom id
    return db.ctx


@pytest.fixture
def set_sort(request, monkeypatch):
    if request.param == "1":
        monkeypatch.setenv("DAS_SET_SORT", "1")
    else:
        monkeypatch.delenv("DAS_SET_SORT", raising=False)
    return request.param


def _sorted_rows(rows):
    rows = np.asarray(rows)
    if rows.shape[0] == 0 or rows.shape[1] == 0:
        return rows
    return rows[np.lexsort(rows.T[::-1])]


def _bounds_hold(T, rows):
    lo, hi = T.bounds()
    if rows.shape[0]:
        for k in range(rows.shape[1]):
            assert lo[k] <= int(rows[:, k].min()) and int(rows[:, k].max()) <= hi[k], (k, lo[k], hi[k])


def _check(T, want, exact):
    """Device table T against the model's table: schema, rows, bounds.  Returns T's rows."""
    assert T.schema == want.schema
    got = T.fetch().T
    assert T.nrows == got.shape[0] == want.nrows, (T.nrows, want.nrows)
    if exact:
        assert np.array_equal(got, want.rows)
    else:
        assert np.array_equal(_sorted_rows(got), _sorted_rows(want.rows))
    _bounds_hold(T, got)
    return got


def _tight(T, t):
    """Declare each column's min / max as T's bounds."""
    if t.nrows:
        T.set_bounds(t.rows.min(axis=0).tolist(), t.rows.max(axis=0).tolist())
    return T


# --------------------------------------------------------------------- join

@pytest.mark.parametrize("case", TC.JOIN_CASES, **_case)
def test_join_ordered(ctx, case):
    inp = TC.build(case)
    want = TC.want(case, TC.join_want)
    a, b = TM.to_device(ctx, inp["a"]), TM.to_device(ctx, inp["b"])
    if inp["bounds"] == "tight":
        _tight(a, inp["a"])
        _tight(b, inp["b"])
    _check(ctx.join(a, b, inp["no_overload"]), want, exact=False)
    if inp["swap"]:
        _check(ctx.join(b, a, inp["no_overload"]), want, exact=False)


def test_join_bounds_are_the_intersection(ctx):
    rng = np.random.default_rng(5)
    n = 3000
    a = NTable(ORDERED, [0, 1], np.stack([rng.integers(0, 8000, n), rng.integers(100, 5001, n)], 1))
    b = NTable(ORDERED, [1, 2], np.stack([rng.integers(3000, 8001, 900), rng.integers(50, 60, 900)], 1))
    A, B = TM.to_device(ctx, a), TM.to_device(ctx, b)
    A.set_bounds([0, 100], [7999, 5000])
    B.set_bounds([3000, 50], [8000, 59])
    for x, y in ((A, B), (B, A)):
        J = ctx.join(x, y)
        rows = _check(J, TM.join(a, b), exact=False)
        assert rows.shape[0] > 100
        assert J.bounds() == ([0, 3000, 50], [7999, 5000, 59])


@pytest.mark.parametrize("case", TC.THETA_CASES, **_case)
def test_join_and_antijoin_unordered_composite(ctx, case):
    inp = TC.build(case)
    a, b = TM.to_device(ctx, inp["a"]), TM.to_device(ctx, inp["b"])
    join = lambda x, y: ctx.join(x, y, inp.get("no_overload", False))  # noqa: E731
    for fn, want, exact in ((join, TC.want(case, TC.theta_join_want), False),
                            (ctx.antijoin, TC.want(case, TC.theta_anti_want), True)):
        if want is AttributeError:
            with pytest.raises(AttributeError):        # the reference's AttributeErrors
                fn(a, b)
        else:
            _check(fn(a, b), want, exact=exact)


# ----------------------------------------------------------------- antijoin

@pytest.mark.parametrize("set_sort", SET_SORT, indirect=True)
@pytest.mark.parametrize("case", TC.ANTI_CASES, **_case)
def test_antijoin_ordered(ctx, case, set_sort):
    inp = TC.build(case)
    _check(ctx.antijoin(TM.to_device(ctx, inp["a"]), TM.to_device(ctx, inp["t"])), TC.want(case, TC.anti_want),
           exact=True)


# -------------------------------------------------------------------- dedup

@pytest.mark.parametrize("set_sort", SET_SORT, indirect=True)
@pytest.mark.parametrize("case", TC.DEDUP_CASES, **_case)
def test_dedup(ctx, case, set_sort):
    inp = TC.build(case)
    _check(ctx.dedup(TM.to_device(ctx, inp["t"])), TC.want(case, TC.dedup_want), exact=False)


# ------------------------------------------------------- set_dedup / set_minus

@pytest.mark.parametrize("case", TC.SET_DEDUP_CASES, **_case)
def test_set_dedup(ctx, case):
    inp = TC.build(case)
    want = TC.want(case, TC.set_dedup_want)
    got = ctx.set_dedup([TM.to_device(ctx, t) for t in inp["ts"]])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _check(g, w, exact=True)


@pytest.mark.parametrize("case", TC.SET_MINUS_CASES, **_case)
def test_set_minus(ctx, case):
    inp = TC.build(case)
    want = TC.want(case, TC.set_minus_want)
    got = ctx.set_minus([TM.to_device(ctx, t) for t in inp["a"]], [TM.to_device(ctx, t) for t in inp["b"]])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _check(g, w, exact=True)


# ------------------------------------------------------------------- concat

@pytest.mark.parametrize("case", TC.CONCAT_CASES, **_case)
def test_concat(ctx, case):
    inp = TC.build(case)
    _check(ctx.concat([TM.to_device(ctx, t) for t in inp["ts"]]), TM.concat(inp["ts"]), exact=True)


def test_concat_schema_mismatch_raises(ctx):
    for pair in TC.concat_mismatches(np.random.default_rng(3), TC.n_atoms()):
        dev = [TM.to_device(ctx, t) for t in pair]
        with pytest.raises(ValueError, match="schema mismatch"):
            ctx.concat(dev)
        with pytest.raises(ValueError, match="schema mismatch"):
            ctx.concat(dev[::-1])


def test_concat_bounds_are_the_union(ctx):
    rng = np.random.default_rng(6)
    ts = [NTable(ORDERED, [0, 1], np.stack([rng.integers(lo, hi + 1, n), rng.integers(7, 9, n)], 1))
          for lo, hi, n in ((10, 20, 65), (15, 40, 3), (12, 13, 2049))]
    dev = [TM.to_device(ctx, t) for t in ts]
    for T, (lo, hi) in zip(dev, ((10, 20), (15, 40), (12, 13))):
        T.set_bounds([lo, 7], [hi, 8])
    C = ctx.concat(dev)
    _check(C, TM.concat(ts), exact=True)
    assert C.bounds() == ([10, 7], [40, 8])


# ------------------------------------------------------ gather / gather_ranges

@pytest.mark.parametrize("case", TC.GATHER_CASES, **_case)
def test_gather_and_gather_ranges(ctx, case):
    inp = TC.build(case)
    t = inp["t"]
    T = TM.to_device(ctx, t)
    for name, idx in inp["idx"].items():
        _check(ctx.gather(T, idx), TM.gather_rows(t, idx), exact=True)
    for name, rs in inp["ranges"].items():
        b, e = [x for x, _ in rs], [y for _, y in rs]
        _check(ctx.gather_ranges(T, b, e), TM.gather_ranges(t, b, e), exact=True)
    n = t.nrows
    for b, e in (([0], [n + 1]), ([0, n], [1, n + 1]), ([1], [0])):
        with pytest.raises(ValueError, match="gather range"):
            ctx.gather_ranges(T, b, e)
    with pytest.raises(ValueError, match="gather index"):
        ctx.gather(T, [0, n])


@pytest.mark.parametrize("how", ["reversed", "descending-ranges", "ascending-repeats"])
def test_gather_of_a_sorted_table_then_join(ctx, how, monkeypatch):
    """The sort-based dedup marks its result sorted by column 0, and the
    direct join skips its counting sort for a build side that says so.  A
    gather that reorders the rows must not pass that mark on."""
    monkeypatch.setenv("DAS_SET_SORT", "1")
    rng = np.random.default_rng(9)
    hi = TC.n_atoms()
    t = TM.ordered(rng, [0, 1], 3000, hi, dup=0.3)
    probe = NTable(ORDERED, [0, 5], np.stack([t.rows[rng.integers(0, 3000, 9000), 0], rng.integers(0, hi, 9000)], 1))
    D = ctx.dedup(TM.to_device(ctx, t))
    d = NTable(ORDERED, [0, 1], _check(D, TM.dedup(t), exact=False))
    assert (np.diff(d.rows[:, 0].astype(np.int64)) >= 0).all()
    n = d.nrows
    if how == "reversed":
        idx = np.arange(n)[::-1]
        G, g = ctx.gather(D, idx), TM.gather_rows(d, idx)
    elif how == "descending-ranges":
        b, e = [n // 2, 0], [n, n // 2]
        G, g = ctx.gather_ranges(D, b, e), TM.gather_ranges(d, b, e)
    else:
        idx = np.sort(rng.integers(0, n, 2 * n))
        G, g = ctx.gather(D, idx), TM.gather_rows(d, idx)
    _check(G, g, exact=True)
    P = TM.to_device(ctx, probe)
    want = TM.join(probe, g)
    assert want.nrows >= 9000
    _check(ctx.join(P, G), want, exact=False)
    _check(ctx.join(G, P), want, exact=False)


# ---------------------------------------------------------------- partition

@pytest.mark.parametrize("nparts", TC.NPARTS)
@pytest.mark.parametrize("case", TC.PARTITION_CASES, **_case)
def test_partition(ctx, case, nparts):
    """The device hash is its own: properties, not the model's destinations."""
    inp = TC.build(case)
    t, other = inp["t"], inp["other"]
    T, OT = TM.to_device(ctx, t), TM.to_device(ctx, other)
    for key in TC.PART_KEYS:
        Pt, counts = ctx.partition(T, list(key), nparts)
        assert Pt.schema == t.schema and counts.shape == (nparts,)
        assert int(counts.sum()) == t.nrows == Pt.nrows
        rows = Pt.fetch().T
        _bounds_hold(Pt, rows)
        assert np.array_equal(_sorted_rows(rows), _sorted_rows(t.rows))           # a permutation of the input
        cols = [t.vars.index(v) for v in key] if key else list(range(len(t.vars)))
        block_of = {}
        dest = np.repeat(np.arange(nparts), counts.astype(np.int64))
        for k, d in zip(map(tuple, rows[:, cols].tolist()), dest.tolist()):
            assert block_of.setdefault(k, d) == d                                 # equal keys share a block
        # rows of block d keep the input's order: a stable sort of the input by block is the output
        if t.nrows:
            din = np.array([block_of[k] for k in map(tuple, t.rows[:, cols].tolist())])
            assert np.array_equal(t.rows[np.argsort(din, kind="stable")], rows)
        if key == (1,):
            # another table on the same key variable: equal key values, equal block index
            Po, co = ctx.partition(OT, [1], nparts)
            orows = Po.fetch().T
            assert np.array_equal(_sorted_rows(orows), _sorted_rows(other.rows))
            odest = np.repeat(np.arange(nparts), co.astype(np.int64))
            oc = other.vars.index(1)
            common = 0
            for k, d in zip(orows[:, oc].tolist(), odest.tolist()):
                if (k,) in block_of:
                    common += 1
                    assert block_of[(k,)] == d
            assert common > 0 or t.nrows < 63


def test_partition_bad_count_raises(ctx):
    T = TM.to_device(ctx, TM.ordered(np.random.default_rng(1), [0, 1], 10, 100))
    for nparts in (0, 4097):
        with pytest.raises(ValueError, match="partition count"):
            ctx.partition(T, [0], nparts)
    with pytest.raises(ValueError, match="partition key"):
        ctx.partition(T, [3], 2)


# -------------------------------------------------------- export / import rows

@pytest.mark.parametrize("case", TC.ROWS_CASES, **_case)
def test_export_import_rows_round_trip(ctx, case):
    import torch
    t = TC.build(case)["t"]
    T = TM.to_device(ctx, t)
    k = len(t.vars)
    buf = torch.full((t.nrows, k), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.current_stream().synchronize()           # the buffer is ready before the context's stream writes it
    ctx.export_rows(T, buf.data_ptr())
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), t.rows)                # the buffer itself: row-major
    back = ctx.import_rows(t.kind, list(t.vars), buf.data_ptr() if t.nrows else None, t.nrows)
    ctx.sync()                                          # before `buf` can be freed
    _check(back, t, exact=True)


def test_import_rows_keeps_kind_and_members(ctx):
    import torch
    for t in (TM.unordered(np.random.default_rng(2), [1, 2], 65, 100),
              TM.composite(np.random.default_rng(3), [0], [[1, 2], [2, 3]], 130, 100)):
        T = TM.to_device(ctx, t)
        buf = torch.zeros((t.nrows, len(t.vars)), dtype=torch.int32, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        ctx.export_rows(T, buf.data_ptr())
        back = ctx.import_rows(t.kind, list(t.vars), buf.data_ptr(), t.nrows, list(t.members) if t.members else None)
        ctx.sync()
        _check(back, t, exact=True)


# ------------------------------------------------------------ operator sequences

def _dev_apply(ctx, op, a, b, extra):
    if op == "join":
        return ctx.join(a, b)
    if op == "antijoin":
        return ctx.antijoin(a, b)
    if op == "dedup":
        return ctx.dedup(a)
    if op == "concat":
        return ctx.concat([a, b])
    if op == "set_dedup":
        return ctx.concat(ctx.set_dedup([a, b]))
    if op == "set_minus":
        return ctx.set_minus([a], [b])[0]
    if op == "gather":
        return ctx.gather(a, extra)
    if op == "gather_ranges":
        return ctx.gather_ranges(a, [x for x, _ in extra], [y for _, y in extra])
    if op == "partition":
        return ctx.partition(a, list(extra[1]), extra[0])[0]
    raise AssertionError(op)


@pytest.mark.parametrize("seed", TC.SEQ_SEEDS)
def test_operator_sequences(ctx, seed, monkeypatch):
    """Twelve operators in a row, each on tables the earlier ones made: what
    an operator's result carries besides its rows (the sorted-column mark,
    the column bounds) is what the next one relies on.  Odd seeds take the
    sort-based set paths; seeds from 3 on start from declared tight bounds."""
    if seed % 2:
        monkeypatch.setenv("DAS_SET_SORT", "1")
    else:
        monkeypatch.delenv("DAS_SET_SORT", raising=False)
    rng = np.random.default_rng(seed)
    pool = TC.seq_start(rng, TC.n_atoms())
    dev = [TM.to_device(ctx, t) for t in pool]
    if seed >= 3:
        for T, t in zip(dev, pool):
            _tight(T, t)
    for step in range(TC.SEQ_STEPS):
        op, i, j, extra = TC.seq_step(rng, pool)
        want = TC.seq_apply(op, pool[i], pool[j], extra)
        assert want.nrows < TC.SEQ_CAP
        got = _dev_apply(ctx, op, dev[i], dev[j], extra)
        _check(got, want, exact=op in TC.SEQ_EXACT)
        # the next steps see the device's row order (equal as a multiset where the order is free)
        pool.append(TM.from_device(got))
        dev.append(got)
