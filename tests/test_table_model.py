"""The host model of the binding-table operators (tests/table_model.py) on
its own: literal results of small fixed tables, the invariants of the input
generators, and the admission of every case of tests/table_cases.py -- the
model alone must give a non-trivial result on a case before the device test
(tests/test_gpu_table_ops.py) may compare against it."""
import numpy as np
import pytest

from oracle import das_oracle as O
from tests import table_cases as TC
from tests import table_model as TM
from tests.table_model import COMPOSITE, ORDERED, UNORDERED, NTable


def _t(kind, vars_, rows, members=None):
    return NTable(kind, vars_, np.array(rows, np.uint32).reshape(-1, len(vars_)), members)


def _l(t):
    return t.rows.tolist()


# ------------------------------------------------------ the model, literally

def test_ordered_join_literals():
    a = _t(ORDERED, [0, 1], [[1, 2], [3, 2], [4, 5], [7, 7]])
    b = _t(ORDERED, [1, 2], [[2, 9], [2, 1], [5, 5], [7, 8]])
    j = TM.join(a, b)
    assert j.schema == (ORDERED, (0, 1, 2), None)
    assert _l(j) == [[1, 2, 9], [1, 2, 1], [3, 2, 9], [3, 2, 1], [4, 5, 5], [7, 7, 8]]
    # no_overload on a non-covering pair: rows with a repeated value go
    assert _l(TM.join(a, b, no_overload=True)) == [[1, 2, 9], [3, 2, 9], [3, 2, 1]]
    # ... and agrees with the oracle's _join_ordered pair by pair
    O.CONFIG["no_overload"] = True
    try:
        ref = [O.join(TM._to_oracle(a, r), TM._to_oracle(b, s)) for r in a.rows for s in b.rows]
    finally:
        O.CONFIG["no_overload"] = False
    assert [[v for _, v in x[1]] for x in ref if x is not None] == _l(TM.join(a, b, no_overload=True))
    # a covering pair returns the covering operand's rows, repeated values and all
    c = _t(ORDERED, [1], [[2], [7]])
    assert _l(TM.join(a, c, no_overload=True)) == [[1, 2], [3, 2], [7, 7]]
    assert _l(TM.join(c, a, no_overload=True)) == [[1, 2], [3, 2], [7, 7]]
    # no shared variable: the cartesian product, first operand major
    d = _t(ORDERED, [5], [[8], [9]])
    assert _l(TM.join(c, d)) == [[2, 8], [2, 9], [7, 8], [7, 9]]
    assert TM.join(a, _t(ORDERED, [1, 2], [])).nrows == 0


def test_antijoin_dedup_concat_gather_literals():
    a = _t(ORDERED, [0, 1], [[1, 2], [3, 2], [4, 5], [1, 2], [7, 7]])
    assert _l(TM.antijoin(a, _t(ORDERED, [1], [[2], [9]]))) == [[4, 5], [7, 7]]
    assert _l(TM.antijoin(a, _t(ORDERED, [0, 1], [[4, 5]]))) == [[1, 2], [3, 2], [1, 2], [7, 7]]
    assert TM.antijoin(a, _t(ORDERED, [1, 3], [[2, 0]])) is a            # not covered: unchanged
    assert _l(TM.dedup(a)) == [[1, 2], [3, 2], [4, 5], [7, 7]]
    assert _l(TM.concat([a, _t(ORDERED, [0, 1], []), _t(ORDERED, [0, 1], [[0, 0]])])) == _l(a) + [[0, 0]]
    assert _l(TM.gather_rows(a, [4, 0, 0])) == [[7, 7], [1, 2], [1, 2]]
    assert _l(TM.gather_ranges(a, [3, 0, 2], [5, 0, 3])) == [[1, 2], [7, 7], [4, 5]]
    p, counts = TM.partition(a, [0], 2)
    assert counts.tolist() == [1, 4] and sorted(_l(p)) == sorted(_l(a))
    assert _l(p) == [[4, 5], [1, 2], [3, 2], [1, 2], [7, 7]]


def test_composite_join_literal():
    # ordered (A, B) joined with an unordered {A, B}: the member must hold the ordered values
    o = _t(ORDERED, [0, 1], [[1, 2], [2, 1], [1, 3], [4, 4]])
    u = _t(UNORDERED, [0, 1], [[1, 2], [3, 4]])
    j = TM.join(o, u)
    assert j.schema == (COMPOSITE, (0, 1, 0, 1), (-1, -1, 0, 0))
    assert _l(j) == [[1, 2, 1, 2], [2, 1, 1, 2]]
    assert TM.join(u, o).schema == j.schema and _l(TM.join(u, o)) == [[1, 2, 1, 2], [2, 1, 1, 2]]
    # two unordered members with a shared variable need a shared value
    v = _t(UNORDERED, [1, 2], [[2, 5], [6, 7]])
    k = TM.join(u, v)
    assert k.schema == (COMPOSITE, (0, 1, 1, 2), (0, 0, 1, 1)) and _l(k) == [[1, 2, 2, 5]]
    # negation: an ordered row goes when an unordered row is covered by it
    assert _l(TM.antijoin(o, u)) == [[1, 3], [4, 4]]
    assert _l(TM.antijoin(u, _t(ORDERED, [0], [[3]]))) == [[1, 2]]


def test_set_dedup_and_minus_across_kinds_literal():
    o = _t(ORDERED, [0], [[1], [2], [1]])
    # a composite whose two members over {1, 2} are equal has its ordered part's identity
    c = _t(COMPOSITE, [0, 1, 2, 1, 2], [[2, 5, 6, 5, 6], [3, 5, 6, 5, 6], [3, 5, 6, 7, 8], [3, 7, 8, 5, 6]],
           [-1, 0, 0, 1, 1])
    u = _t(UNORDERED, [0], [[1], [1]])
    d = TM.set_dedup([o, c, u])
    assert [t.schema for t in d] == [o.schema, c.schema, u.schema]
    assert _l(d[0]) == [[1], [2]]
    assert _l(d[1]) == [[3, 5, 6, 5, 6], [3, 5, 6, 7, 8]]      # [2 | twins] is o's row 2; member order is no identity
    assert _l(d[2]) == [[1]]                                   # an unordered {0: 1} is not the ordered one
    m = TM.set_minus([c, o], [_t(ORDERED, [0], [[3]])])
    assert _l(m[0]) == [[2, 5, 6, 5, 6], [3, 5, 6, 7, 8], [3, 7, 8, 5, 6]] and _l(m[1]) == _l(o)
    assert TM.dedup(c).schema == c.schema and _l(TM.dedup(c)) == [[2, 5, 6, 5, 6], [3, 5, 6, 5, 6], [3, 5, 6, 7, 8]]


# ------------------------------------------------------------ the generators

def test_generators_keep_their_invariants():
    rng = np.random.default_rng(0)
    hi = 50
    t = TM.ordered(rng, [3, 1, 2], 1000, hi, dup=0.5)
    assert t.schema == (ORDERED, (1, 2, 3), None) and t.rows.shape == (1000, 3) and t.rows.max() < hi
    assert 400 <= 1000 - len(np.unique(TM.ordered(rng, [0, 1, 2], 1000, 1 << 20, dup=0.5).rows, axis=0)) <= 500
    assert len(np.unique(TM.ordered(rng, [0, 1], 100, hi, dup=1.0).rows, axis=0)) == 1
    assert TM.ordered(rng, [0], 0, hi).rows.shape == (0, 1)
    u = TM.unordered(rng, [2, 0, 1], 500, 9)
    assert u.schema == (UNORDERED, (0, 1, 2), None) and u.rows.max() < 9
    assert (np.diff(u.rows.astype(np.int64), axis=1) > 0).all()                 # ascending, distinct
    c = TM.composite(rng, [4, 0], [[2, 1], [3, 1, 5]], 300, 11)
    assert c.schema == (COMPOSITE, (0, 4, 1, 2, 1, 3, 5), (-1, -1, 0, 0, 1, 1, 1)) and c.rows.max() < 11
    assert (np.diff(c.rows[:, 2:4].astype(np.int64), axis=1) > 0).all()
    assert (np.diff(c.rows[:, 4:7].astype(np.int64), axis=1) > 0).all()
    assert TM._parts(c) == ([0, 4], [[1, 2], [1, 3, 5]])
    assert TM.composite(rng, [], [[0, 1]], 5, 4).members == (0, 0)


def _inputs_below_hi(inp):
    hi = TC.n_atoms()
    for v in inp.values():
        for t in (v if isinstance(v, list) else [v]):
            if isinstance(t, NTable) and t.nrows:
                assert int(t.rows.max()) < hi
                assert list(t.vars[:len(TM._parts(t)[0] or [])]) == sorted(TM._parts(t)[0] or [])


def test_kb_holds_enough_atoms():
    assert TC.n_atoms() >= 8192


# ------------------------------------------------------ admission of the cases

@pytest.mark.parametrize("case", TC.JOIN_CASES, ids=lambda c: c.id)
def test_join_case_is_admitted(case):
    inp = TC.build(case)
    _inputs_below_hi(inp)
    w = TC.want(case, TC.join_want)
    assert w.nrows < TC.JOIN_CAP
    assert inp["rows"] is None or (w.nrows > 0) == inp["rows"], w.nrows
    if inp["no_overload"]:
        plain = TM.join(inp["a"], inp["b"])
        rep = [len(set(r)) < len(r) for r in plain.rows.tolist()]
        assert any(rep) and not all(rep)                      # the filter has rows to drop and rows to keep
        if inp["covering"]:
            assert _l(w) == _l(plain)
        else:
            assert w.nrows == rep.count(False)


def test_join_cases_cover_every_cartesian_kernel_and_remainder():
    seen = set()
    for case in TC.JOIN_CASES:
        if case.id.startswith("cart-"):
            inp = TC.build(case)
            seen.add((len(inp["a"].vars) + len(inp["b"].vars), inp["a"].nrows * inp["b"].nrows % 4))
    assert {(w, r) for w in (2, 3, 4, 5, 6, 7) for r in range(4)} <= seen


def test_theta_cases_are_admitted():
    """Every pair of kinds (an ordered pair aside) has a join that produces
    rows or raises as the reference does, and -- unless it only raises -- an
    antijoin that drops some rows and keeps some."""
    joins, antis = {}, {}
    for case in TC.THETA_CASES:
        inp = TC.build(case)
        _inputs_below_hi(inp)
        if "empty" in case.id:
            assert inp["a"].nrows * inp["b"].nrows == 0
            assert TC.want(case, TC.theta_join_want).nrows == 0                 # and no AttributeError
            assert TC.want(case, TC.theta_anti_want).nrows == inp["a"].nrows
            continue
        if inp.get("no_overload"):
            w, plain = TC.want(case, TC.theta_join_want), TM.join(inp["a"], inp["b"])
            assert 0 < w.nrows < plain.nrows
            continue
        assert 1 <= inp["a"].nrows <= 300 and 1 <= inp["b"].nrows <= 300
        kinds = (inp["a"].kind, inp["b"].kind)
        w = TC.want(case, TC.theta_join_want)
        joins.setdefault(kinds, []).append("raise" if w is AttributeError else w.nrows)
        v = TC.want(case, TC.theta_anti_want)
        antis.setdefault(kinds, []).append("raise" if v is AttributeError else (v.nrows, inp["a"].nrows))
    kinds3 = (ORDERED, UNORDERED, COMPOSITE)
    pairs = {(x, y) for x in kinds3 for y in kinds3} - {(ORDERED, ORDERED)}
    assert set(joins) == pairs
    for k in pairs:
        assert any(n == "raise" or n > 0 for n in joins[k]), (k, joins[k])
        ran = [x for x in antis[k] if x != "raise"]
        assert not ran or any(0 < kept < n for kept, n in ran), (k, antis[k])
    assert any("raise" in v for v in joins.values()) and any("raise" in v for v in antis.values())
    assert sum(n != "raise" and n > 0 for v in joins.values() for n in v) >= 12


@pytest.mark.parametrize("case", TC.ANTI_CASES, ids=lambda c: c.id)
def test_antijoin_case_is_admitted(case):
    inp = TC.build(case)
    _inputs_below_hi(inp)
    w = TC.want(case, TC.anti_want)
    n = inp["a"].nrows
    if inp["covered"] and n >= 63:
        assert 0 < w.nrows < n
    if not inp["covered"]:
        assert w.nrows == n > 0


@pytest.mark.parametrize("case", TC.DEDUP_CASES, ids=lambda c: c.id)
def test_dedup_case_is_admitted(case):
    inp = TC.build(case)
    _inputs_below_hi(inp)
    w = TC.want(case, TC.dedup_want)
    n = inp["t"].nrows
    assert w.nrows <= n
    if inp["drops"]:
        assert w.nrows < n
    if inp["keeps"]:
        assert w.nrows > 0


def test_dedup_composite_case_cancels_twin_members():
    inp = TC.build([c for c in TC.DEDUP_CASES if c.id == "dedup-composite"][0])
    t = inp["t"]
    twins = (t.rows[:, 1:3] == t.rows[:, 3:5]).all(axis=1)
    assert twins.any() and not twins.all()
    # rows of twins with one ordered value are one identity whatever the twins hold
    tw = t.rows[twins]
    assert len(np.unique(tw, axis=0)) > len(np.unique(tw[:, 0]))
    assert TC.want(TC.DEDUP_CASES[-1], TC.dedup_want).nrows < len(np.unique(t.rows, axis=0))


@pytest.mark.parametrize("case", TC.SET_DEDUP_CASES, ids=lambda c: c.id)
def test_set_dedup_case_is_admitted(case):
    inp = TC.build(case)
    _inputs_below_hi(inp)
    w = TC.want(case, TC.set_dedup_want)
    n_in, n_out = sum(t.nrows for t in inp["ts"]), sum(t.nrows for t in w)
    assert 0 < n_out < n_in
    if len(inp["ts"]) > 1 and case.id != "setdedup-empty-in-the-middle":
        # identities repeat across tables, not only inside one: a later table loses more than on its own
        alone = sum(TM.set_dedup([t])[0].nrows for t in inp["ts"])
        assert n_out < alone, case.id


@pytest.mark.parametrize("case", TC.SET_MINUS_CASES, ids=lambda c: c.id)
def test_set_minus_case_is_admitted(case):
    inp = TC.build(case)
    _inputs_below_hi(inp)
    w = TC.want(case, TC.set_minus_want)
    n_in, n_out = sum(t.nrows for t in inp["a"]), sum(t.nrows for t in w)
    assert (n_out < n_in) == inp["drops"]
    assert (n_out > 0) == inp["keeps"]


def test_set_minus_ordered_takes_cancelled_composite_rows():
    case = [c for c in TC.SET_MINUS_CASES if c.id == "setminus-ordered-from-composite"][0]
    inp, w = TC.build(case), TC.want(case, TC.set_minus_want)
    comp = inp["a"][1]
    twins = (comp.rows[:, 2:4] == comp.rows[:, 4:6]).all(axis=1)
    gone = {tuple(r) for r in inp["b"][0].rows.tolist()}
    hit = np.array([tuple(r) in gone for r in comp.rows[:, :2].tolist()])
    assert (twins & hit).any() and (~twins & hit).any()
    assert w[1].nrows == comp.nrows - int((twins & hit).sum())


def test_sequences_are_admitted():
    """Host-only run of the operator sequences: they stay under the size cap,
    use every operator and keep producing rows."""
    used = set()
    for seed in TC.SEQ_SEEDS:
        rng = np.random.default_rng(seed)
        pool = TC.seq_start(rng, TC.n_atoms())
        nonempty = 0
        for _ in range(TC.SEQ_STEPS):
            op, i, j, extra = TC.seq_step(rng, pool)
            r = TC.seq_apply(op, pool[i], pool[j], extra)
            assert r.nrows < TC.SEQ_CAP
            used.add(op)
            nonempty += r.nrows > 0
            pool.append(r)
        assert nonempty >= TC.SEQ_STEPS // 2
    assert used == set(TC.SEQ_OPS)
