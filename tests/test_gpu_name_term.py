"""NameMatch inside queries on the device (das_scan_node_names,
das_table_name_filter; names.hip) against a fold over the CPU oracle that this
file writes itself: every ordinary term is the oracle's, a name term is the
`re.search` row set of its definition, And / Or / Not combine them by the
reference's rules.  Each case runs with the filter forced to `walk`, to `flags`
and on the definition path (DAS_NAME_TERM=0)."""
import hashlib
import json
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest

from das_amd import _lib
from das_amd.pattern_matcher import pattern_matcher as pm
from oracle import das_oracle as O
from tests import name_search_corpus as C
from tests.util import canon

pytestmark = pytest.mark.gpu

STAGE = _lib.NAME_STAGE_BYTES
MODES = ["walk", "flags", "host"]


# ---------------------------------------------------------------------------
# the KB
# ---------------------------------------------------------------------------
def _types():
    rng = random.Random(23)
    d = {""}
    while len(d) < 996:
        d.add("".join(rng.choice("abc0123456789") for _ in range(rng.randint(0, 40))))
    d = sorted(d - {""})
    rng.shuffle(d)                                              # (the links below pick nodes by position)
    d.insert(5, "")
    return {
        "A": ["a"],
        "D": d + ["mus123", "mus1234", "xmus123", "CoA"],
        "L": ["ab" + "-" * (64 * 1024 - 2) + "7", "b" + "-" * (STAGE - 2) + "a", "ab7"],
        "U": ["é", "naïve", "٣", "a٣7", "ma", "human", "x" * 70 + "é"],
        "Schema": ["gene_name", "gene_uniquename"],
    }


TYPES = _types()
DN = TYPES["D"]
SPECIAL = ["mus123", "mus1234", "xmus123", "CoA"]


def _n(t, name):
    return f'"{t} {name}"'


def _links():
    out = []
    for i in range(299):                                        # chains: a node is a source and a target
        out.append(f'(Inheritance {_n("D", DN[i + 1])} {_n("D", DN[i + 2])})')
        if i % 3 == 0:
            out.append(f'(Inheritance {_n("D", DN[i + 1])} {_n("D", DN[i + 8])})')
    names = SPECIAL + DN[600:746]
    for i in range(150):                                        # FlyBase shape: Execution(Schema, gene, name)
        out.append(f'(Execution {_n("Schema", "gene_name")} {_n("D", DN[400 + i])} {_n("D", names[i])})')
        out.append(f'(Execution {_n("Schema", "gene_uniquename")} {_n("D", DN[400 + i])} {_n("D", DN[800 + i])})')
    for i in range(12):
        out.append(f'(Similarity {_n("D", DN[2 * i + 1])} {_n("D", DN[2 * i + 30])})')
    for i in range(30):
        out.append(f'(Pair {_n("D", DN[900 + i])} {_n("D", DN[930 + i % 7])})')
    k = 10
    for t in ("L", "U", "A"):                                   # every node of the small types is a target
        for name in TYPES[t]:
            out.append(f'(Inheritance {_n("D", DN[k])} {_n(t, name)})')
            k += 1
    for i in range(10):                                         # List: the second target a node or a link
        out.append(f'(List {_n("D", DN[i + 1])} {_n("D", DN[i + 50])})')
        if i % 2 == 0:
            out.append(f'(List {_n("D", DN[i + 1])} (Inheritance {_n("D", DN[i + 1])} {_n("D", DN[i + 2])}))')
    return out


def _canonical():
    link_types = ["Inheritance", "Execution", "Similarity", "Pair", "List"]
    lines = [f"(: {t} Type)" for t in list(TYPES) + link_types]
    for t, names in TYPES.items():
        lines += [f'(: "{n}" {t})' for n in names]
    return "\n".join(lines + _links()) + "\n"


@pytest.fixture(scope="module")
def db():
    from das_amd.database.hip_db import HipDB
    d = HipDB(device=0)
    d.load_canonical(_canonical())
    return d


@pytest.fixture(scope="module")
def world(db):
    """The oracle's view of the KB and the host mirror, computed once."""
    kb = O.KB.from_arrays(db.arrays)
    _, cat, _, ty, nl = db._host_mirror()
    names = {int(i): db.arrays.node_name(int(nl[i])) for i in np.nonzero(cat == 1)[0]}
    return SimpleNamespace(kb=kb, odb=O.RedisMongoSemantics(kb), cat=cat, ty=ty, names=names, want={},
                           hits={})


@pytest.fixture(params=MODES)
def mode(request, monkeypatch):
    if request.param == "host":
        monkeypatch.setenv("DAS_NAME_TERM", "0")
    else:
        monkeypatch.setenv("DAS_NAME_TERM_FILTER", request.param)
    return request.param


# ---------------------------------------------------------------------------
# the expectation: a fold over the oracle (das_oracle.py:717-809 restated for
# trees that hold ["NameMatch", variable, type, pattern])
# ---------------------------------------------------------------------------
def has_name_term(spec):
    if spec[0] == "NameMatch":
        return True
    if spec[0] == "Not":
        return has_name_term(spec[1])
    if spec[0] in ("And", "Or"):
        return any(has_name_term(t) for t in spec[1])
    return False


def o_matched(spec, w, answer):
    kind = spec[0]
    if kind == "NameMatch":
        _, var, t, p = spec
        answer.rows = O.RowSet(O.o_row({var: h}) for h, (nt, name) in w.kb.nodes.items()
                               if nt == t and re.search(p, name))
        return bool(answer.rows)
    if not has_name_term(spec):
        return O.matched(spec, w.odb, answer)
    if kind == "Not":
        o_matched(spec[1], w, answer)
        answer.negation = not answer.negation
        return True
    if kind == "Or":
        union, or_matched, negative = None, False, []
        for term in spec[1]:
            if term[0] == "Not":
                negative.append(term)
                continue
            sub = O.Answer()
            if not o_matched(term, w, sub):
                continue
            or_matched = True
            if not sub.rows:
                continue
            if not union:
                union = sub.rows
                continue
            union.update(sub.rows)
        union = union or O.RowSet()
        if negative:
            sub = O.Answer()
            o_matched(["And", [t[1] for t in negative]], w, sub)
            answer.rows = sub.rows.minus(union)
            answer.negation = True
        else:
            answer.rows = union
        return or_matched
    assert kind == "And"
    acc, forbidden = [], O.RowSet()
    for term in spec[1]:
        sub = O.Answer()
        if not o_matched(term, w, sub):
            return False
        if not sub.rows:
            continue
        if sub.negation:
            forbidden.update(sub.rows)
            continue
        if not acc:
            acc = list(sub.rows)
            continue
        fast = O._ordered_hash_join(acc, sub.rows)              # the same rows as the nested loop, where it applies
        acc = fast if fast is not None else \
            [j for a in acc for b in sub.rows for j in [O.join(a, b)] if j is not None]
    result = O.RowSet()
    for a in acc:
        if all(O.check_negation(a, t) for t in forbidden):
            result.add(a)
    answer.rows = result
    return bool(result)


def _sha(rows):
    return hashlib.sha256("\n".join(rows).encode()).hexdigest()


def want_of(spec, w, no_overload=False):
    key = (json.dumps(spec), no_overload)
    if key not in w.want:
        O.CONFIG["no_overload"] = no_overload
        try:
            ans = O.Answer()
            m = o_matched(spec, w, ans)
        finally:
            O.CONFIG["no_overload"] = False
        rows = sorted(json.dumps(O.canon_json(r), sort_keys=True) for r in ans.rows)
        w.want[key] = {"matched": bool(m), "negation": ans.negation, "n": len(ans.rows), "sha256": _sha(rows)}
    return w.want[key]


def build(spec):
    kind = spec[0]
    if kind == "NameMatch":
        return pm.NameMatch(spec[1], spec[2], spec[3])
    if kind == "Node":
        return pm.Node(spec[1], spec[2])
    if kind == "Var":
        return pm.Variable(spec[1])
    if kind == "Link":
        return pm.Link(spec[1], [build(t) for t in spec[3]], spec[2])
    if kind == "Not":
        return pm.Not(build(spec[1]))
    return (pm.And if kind == "And" else pm.Or)([build(t) for t in spec[1]])


def got_of(spec, db, no_overload=False):
    pm.CONFIG["no_overload"] = no_overload
    try:
        ans = pm.PatternMatchingAnswer()
        m = build(spec).matched(db, ans)
        rows = sorted(json.dumps(canon(a), sort_keys=True) for a in ans.assignments)
        count = ans.count()
    finally:
        pm.CONFIG["no_overload"] = False
    return {"matched": bool(m), "negation": ans.negation, "n": len(rows), "sha256": _sha(rows)}, count


def check(spec, db, w, no_overload=False):
    want = want_of(spec, w, no_overload)
    got, count = got_of(spec, db, no_overload)
    assert got == want, spec
    assert count == want["n"], spec
    return want


def V(n):
    return ["Var", n]


def L(t, targets, ordered=True):
    return ["Link", t, ordered, targets]


def NM(var, t, p):
    return ["NameMatch", var, t, p]


INH = L("Inheritance", [V("V1"), V("V2")])
GN = L("Execution", [["Node", "Schema", "gene_name"], V("V1"), V("V2")])
GU = L("Execution", [["Node", "Schema", "gene_uniquename"], V("V1"), V("V3")])
PATTERNS = ["^[ab]", r"\d\d$", "CoA|mus", ""]


class Calls:
    """Counts the calls of one Context method."""

    def __init__(self, db, monkeypatch, name):
        self.n = 0
        orig = getattr(db.ctx, name)

        def counted(*a, **k):
            self.n += 1
            return orig(*a, **k)
        monkeypatch.setattr(db.ctx, name, counted, raising=False)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("t", list(TYPES) + ["Inheritance", "Nope"])
def test_stand_alone_term(db, world, mode, t):
    """Case 1: every pattern of the corpus against get_matched_node_name."""
    for p in C.ALL_PATTERNS:
        if (t, p) not in world.hits:
            world.hits[(t, p)] = set(db.get_matched_node_name(t, p))
        want = world.hits[(t, p)]
        before = dict(db.name_term_stats)
        ans = pm.PatternMatchingAnswer()
        m = pm.NameMatch("X", t, p).matched(db, ans)
        assert m == bool(want), (t, p)
        assert ans.negation is False
        assert ans.count() == len(want), (t, p)
        tables = db.rel_local_tables(ans._relation())
        assert all(x.kind == _lib.TABLE_ORDERED and len(x.vars) == 1 for x in tables)
        assert {a.mapping["X"] for a in ans.assignments} == want, (t, p)
        assert all(set(a.mapping) == {"X"} for a in ans.assignments)
        delta = {k: db.name_term_stats[k] - before[k] for k in before}
        if t not in TYPES:                                      # a type without nodes / an unknown type
            if t == "Nope":
                assert delta == {"device": 0, "host": 0}
            continue
        if mode == "host" or p in C.DECLINE_ALWAYS or (t == "U" and p in C.DECLINE_NON_ASCII):
            assert delta == {"device": 0, "host": 1}, (t, p)
        elif (t != "U" and p in C.MUST_COMPILE_ASCII) or (t == "U" and p in C.MUST_COMPILE_ANY):
            assert delta == {"device": 1, "host": 0}, (t, p)
        else:
            assert sum(delta.values()) == 1


def test_scan_table_is_sorted_with_tight_bounds(db):
    """Operator A itself: ascending ids, the bounds its first and last id."""
    from das_amd.name_search import compile_name_pattern
    tid = db.type_id["D"]
    for p in ("^[ab]", "CoA", "", "^mus123$"):
        dfa = compile_name_pattern(p, ascii_only=True)
        ids, n = db.ctx.match_node_names(tid, dfa)
        t = db.ctx.scan_node_names(tid, dfa, 5)
        assert (t.kind, t.vars, t.nrows) == (_lib.TABLE_ORDERED, (5,), n)
        got = t.fetch()[0]
        assert np.array_equal(got, ids) and np.all(np.diff(got.astype(np.int64)) > 0)
        assert t.bounds() == ([int(ids[0])], [int(ids[-1])])
    t = db.ctx.scan_node_names(tid, compile_name_pattern("no such name Q", ascii_only=True), 5)
    assert (t.kind, t.vars, t.nrows) == (_lib.TABLE_ORDERED, (5,), 0)
    t = db.ctx.scan_node_names(db.type_id["Inheritance"], compile_name_pattern("", ascii_only=True), 5)
    assert t.nrows == 0


@pytest.mark.parametrize("p", PATTERNS + [r"^mus\d\d\d$"])
def test_term_first_then_links(db, world, mode, p, monkeypatch):
    """Case 2: the index join runs from operator A's table."""
    ij = Calls(db, monkeypatch, "index_join")
    check(["And", [NM("V2", "D", p), INH]], db, world)
    check(["And", [NM("V1", "D", p), GN, GU]], db, world)
    assert check(["And", [NM("V2", "D", p), GN, GU]], db, world)["n"] > 0
    assert ij.n > 0


def test_term_after_its_variable_is_bound(db, world, mode, monkeypatch):
    """Case 3: the filter shortcut; the variable first, in the middle, last."""
    flt = Calls(db, monkeypatch, "table_name_filter")
    n = 0
    for p in PATTERNS:
        for var in ("V1", "V2"):
            n += check(["And", [INH, NM(var, "D", p)]], db, world)["n"]
        for var in ("V1", "V2", "V3"):
            n += check(["And", [GN, GU, NM(var, "D", p)]], db, world)["n"]
            n += check(["And", [GN, NM(var if var != "V3" else "V2", "D", p), GU]], db, world)["n"]
    # names of the small types: the first and the last slot of a type's range and of the heap
    for t, p in (("L", "7$"), ("L", "a$"), ("L", ""), ("A", "a"), ("U", "é"), ("U", "ma|human"), ("U", r"\d"),
                 ("Schema", "")):
        check(["And", [INH, NM("V2", t, p)]], db, world)
    assert n > 0
    assert (flt.n > 0) == (mode != "host")


def test_term_on_a_variable_of_its_own(db, world, mode):
    """Case 4: a cross product through the ordinary join."""
    pair = L("Pair", [V("V1"), V("V2")])
    for p in ("CoA|mus", "^[ab]"):
        assert check(["And", [pair, NM("V9", "D", p)]], db, world)["n"] > 30
        check(["And", [NM("V9", "D", p), pair]], db, world)


def test_reset_on_empty_and_failing_term(db, world, mode):
    """Cases 5 and 6."""
    # CoA is a name of the type, but no target of an Inheritance link: the join is empty, GN's rows stand
    w = check(["And", [INH, NM("V2", "D", "^CoA$"), L("Execution", [["Node", "Schema", "gene_name"], V("V3"), V("V4")])]],
              db, world)
    assert w["matched"] and w["n"] == 150
    # the issue's out-of-scope example: [L1, NameMatch(V of L3), L2, L3] with L1 join L2 empty
    l1 = L("Pair", [V("V1"), V("V2")])
    l2 = L("Inheritance", [V("V2"), ["Node", "A", "a"]])
    w = check(["And", [l1, NM("V3", "D", "^[ab]"), l2, L("Similarity", [V("V3"), V("V4")])]], db, world)
    assert w["matched"]
    # no name of the type matches: And is False, wherever the term stands
    for terms in ([INH, NM("V2", "D", "no such name Q")], [NM("V2", "D", "no such name Q"), INH],
                  [INH, NM("V2", "Nope", "")], [INH, NM("V7", "D", "no such name Q"), GN]):
        w = check(["And", terms], db, world)
        assert not w["matched"] and w["n"] == 0


def test_not_and_or(db, world, mode):
    """Case 7."""
    for p in ("^[ab]", "CoA|mus", "no such name Q"):
        check(["And", [INH, ["Not", NM("V2", "D", p)]]], db, world)
        check(["And", [["Not", NM("V1", "D", p)], GN]], db, world)
        check(["Or", [NM("V2", "D", p), INH]], db, world)
        check(["Or", [INH, ["Not", NM("V2", "D", p)]]], db, world)
        check(["Not", NM("V2", "D", p)], db, world)
        check(["And", [GN, ["Or", [NM("V2", "D", p), NM("V2", "D", "^mus")]]]], db, world)
    w = check(["And", [INH, ["Not", NM("V2", "D", "^[ab]")]]], db, world)
    assert 0 < w["n"] < want_of(INH, world)["n"]


def test_unordered_operand(db, world, mode, monkeypatch):
    """Case 8: the composite algebra, no shortcut."""
    flt = Calls(db, monkeypatch, "table_name_filter")
    sim = L("Similarity", [V("V1"), V("V2")], False)
    for p in ("^[ab0-4]", ""):
        assert check(["And", [sim, NM("V1", "D", p)]], db, world)["n"] > 0
        check(["And", [NM("V2", "D", p), sim]], db, world)
        check(["And", [sim, INH, NM("V1", "D", p)]], db, world)
    assert flt.n == 0


def test_cross_product_then_term(db, world, mode):
    """Case 9: two links without a shared variable, then the term."""
    pair = L("Pair", [V("V5"), V("V6")])
    for var, p in (("V2", "CoA|mus"), ("V6", "^[ab0-4]"), ("V1", "")):
        assert check(["And", [pair, GN, NM(var, "D", p)]], db, world)["n"] > 0


def test_rows_that_bind_links_are_dropped(db, world, mode):
    """Case 10."""
    lst = L("List", [V("V1"), V("V2")])
    w = check(["And", [lst, NM("V2", "D", "")]], db, world)
    assert w["n"] == 10 and want_of(lst, world)["n"] == 15
    check(["And", [L("*", [V("V1"), V("V2")]), NM("V2", "D", "^[ab]")]], db, world)
    check(["And", [L("*", [V("V1"), V("V2")]), NM("V1", "D", "^[ab]")]], db, world)


def test_no_overload(db, world, mode):
    """Case 11: cases 3 and 4 with distinct values per variable."""
    assert pm.CONFIG["no_overload"] is False
    pair = L("Pair", [V("V1"), V("V2")])
    for p in ("^[ab]", "CoA|mus"):
        for var in ("V1", "V2", "V3"):
            check(["And", [GN, GU, NM(var, "D", p)]], db, world, no_overload=True)
        check(["And", [INH, NM("V2", "D", p)]], db, world, no_overload=True)
        check(["And", [pair, NM("V9", "D", p)]], db, world, no_overload=True)
    # a value the row already holds cannot be bound to the fresh variable
    w = check(["And", [pair, NM("V9", "D", "")]], db, world, no_overload=True)
    assert w["n"] < want_of(["And", [pair, NM("V9", "D", "")]], world)["n"]
    assert pm.CONFIG["no_overload"] is False


def test_facade_equals_the_notebook_loop(db, world, mode):
    """Case 12: das.query / das.get_mappings of the one query against the loop
    of QueryFlyBase.ipynb (a name search, then queries per name)."""
    from das_amd.distributed_atom_space import DistributedAtomSpace
    das = DistributedAtomSpace(db=db)
    for p in (r"^mus\d\d\d$", "mus", "^[ab]"):
        rows = set()
        for h in db.get_matched_node_name("D", p):
            name = das.get_node_name(h)
            a1 = pm.PatternMatchingAnswer()
            q1 = pm.Link("Execution", [pm.Node("Schema", "gene_name"), pm.Variable("v1"), pm.Node("D", name)], True)
            if not q1.matched(db, a1):
                continue
            for a in a1.assignments:
                gene = das.get_node_name(a.mapping["v1"])
                a2 = pm.PatternMatchingAnswer()
                q2 = pm.Link("Execution", [pm.Node("Schema", "gene_uniquename"), pm.Node("D", gene),
                                           pm.Variable("v3")], True)
                if q2.matched(db, a2):
                    rows |= {(a.mapping["v1"], h, b.mapping["v3"]) for b in a2.assignments}
        query = pm.And([pm.NameMatch("v2", "D", p),
                        pm.Link("Execution", [pm.Node("Schema", "gene_name"), pm.Variable("v1"), pm.Variable("v2")], True),
                        pm.Link("Execution", [pm.Node("Schema", "gene_uniquename"), pm.Variable("v1"),
                                              pm.Variable("v3")], True)])
        assert rows
        text = das.query(query)
        assert text.count("'v1'") == len(rows)
        for v1, v2, v3 in rows:
            assert f"'v1': '{v1}'" in text and f"'v2': '{v2}'" in text and f"'v3': '{v3}'" in text
        ans = pm.PatternMatchingAnswer()
        assert query.matched(db, ans)
        assert {(a.mapping["v1"], a.mapping["v2"], a.mapping["v3"]) for a in ans.assignments} == rows
        before = dict(db.name_fetch_stats)
        assert sorted(das.get_mappings(query, "v3")) == sorted(das.get_node_name(r[2]) for r in rows)
        assert db.name_fetch_stats["device"] == before["device"] + 1     # ordered tables: answer.names' device path
        assert sorted(das.get_mappings(query, "v2")) == sorted(das.get_node_name(r[1]) for r in rows)
    assert das.get_mappings(pm.And([pm.NameMatch("v2", "D", "no such name Q")]), "v2") == []
    assert das.query(pm.NameMatch("v2", "D", "no such name Q")) == ""


def test_matched_many_evaluates_the_term_one_by_one(db, world, mode):
    specs = [INH, ["And", [INH, NM("V2", "D", "^[ab]")]], NM("V1", "A", "a"), ["Or", [NM("V2", "D", "CoA"), GN]]]
    res = pm.matched_many(db, [build(s) for s in specs])
    for s, (m, ans) in zip(specs, res):
        rows = sorted(json.dumps(canon(a), sort_keys=True) for a in ans.assignments)
        got = {"matched": bool(m), "negation": ans.negation, "n": len(rows), "sha256": _sha(rows)}
        assert got == want_of(s, world), s


def test_no_resident_memory_is_added(db, world):
    check(["And", [INH, NM("V2", "D", "^[ab]")]], db, world)    # (the heap exists now)
    before = int(db.ctx.stats().device_bytes)
    for spec in (["And", [INH, NM("V2", "D", "^[ab]")]], ["And", [NM("V2", "D", "CoA"), GN]], NM("V1", "L", "7$")):
        check(spec, db, world)
    assert int(db.ctx.stats().device_bytes) == before


def test_unsupported_dbs(db):
    from das_amd.parallel import ShardedDB
    with pytest.raises(NotImplementedError, match="NameMatch on a sharded DB"):
        pm.NameMatch("V1", "D", "a").matched(ShardedDB.__new__(ShardedDB), pm.PatternMatchingAnswer())
    with pytest.raises(TypeError):
        pm.And([build(INH), pm.NameMatch("V1", "D", "a")]).matched(object(), pm.PatternMatchingAnswer())


# ---------------------------------------------------------------------------
# operator B through _lib
# ---------------------------------------------------------------------------
FILTER_MODES = [("walk", _lib.NAME_FILTER_WALK), ("flags", _lib.NAME_FILTER_FLAGS)]
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]


def _host_keep(w, values, tid, rx):
    n_atoms = len(w.cat)
    return np.array([v < n_atoms and w.cat[v] == 1 and w.ty[v] == tid and rx.search(w.names[int(v)]) is not None
                     for v in values], dtype=bool)


def _value_pool(db, w, tid):
    n_atoms = len(w.cat)
    of_type = np.nonzero((w.cat == 1) & (w.ty == tid))[0]
    others = np.nonzero((w.cat == 1) & (w.ty != tid))[0]
    links = np.nonzero(w.cat == 2)[0]
    odd = np.array([_lib.DAS_NONE, n_atoms, n_atoms + 5], dtype=np.int64)
    return of_type, np.concatenate([others, links[:: max(1, len(links) // 40)], odd])


@pytest.mark.parametrize("name,mode_id", FILTER_MODES)
def test_filter_rows_columns_and_values(db, world, name, mode_id):
    from das_amd.name_search import compile_name_pattern
    rng = np.random.default_rng(5)
    for t, p in (("D", "^[ab]"), ("D", r"\d\d$"), ("L", "7$"), ("U", "a")):
        tid = db.type_id[t]
        dfa = compile_name_pattern(p, ascii_only=t != "U")
        assert dfa is not None
        rx = re.compile(p)
        of_type, rest = _value_pool(db, world, tid)
        for n in ROWS if t == "D" else [257]:
            for ncols in (1, 2, 3):
                for at in range(ncols):
                    cols = rng.integers(0, len(world.cat), size=(ncols, n), dtype=np.int64)
                    pick = rng.random(n)
                    col = np.where(pick < 0.7, of_type[rng.integers(0, len(of_type), n)],
                                   rest[rng.integers(0, len(rest), n)])      # (a value repeats: 1000 of ~1000)
                    cols[at] = col
                    cols = cols.astype(np.uint32)
                    vars_ = [20 + k for k in range(ncols)]
                    src = db.ctx.table_from_host(_lib.TABLE_ORDERED, vars_, cols)
                    lo, hi = [3 + k for k in range(ncols)], [_lib.DAS_NONE - k for k in range(ncols)]
                    src.set_bounds(lo, hi)
                    out = db.ctx.table_name_filter(src, 20 + at, tid, dfa, mode_id)
                    keep = _host_keep(world, cols[at], tid, rx) if n else np.zeros(0, dtype=bool)
                    assert (out.kind, out.vars, out.nrows) == (_lib.TABLE_ORDERED, tuple(vars_), int(keep.sum()))
                    assert np.array_equal(out.fetch(), cols[:, keep]), (t, p, n, ncols, at)
                    assert out.bounds() == (lo, hi)
                    if n >= 255 and t == "D":
                        assert 0 < out.nrows < n


def test_filter_auto_mode_around_its_cut_over(db, world, monkeypatch):
    """Mode 0 without the environment variable: flags from one row per node of
    the type on, walk below; the same rows either way."""
    from das_amd.name_search import compile_name_pattern
    monkeypatch.delenv("DAS_NAME_TERM_FILTER", raising=False)
    tid = db.type_id["D"]
    dfa, rx = compile_name_pattern("^[ab]", ascii_only=True), re.compile("^[ab]")
    of_type, rest = _value_pool(db, world, tid)
    assert len(of_type) == len(DN) == 1000
    rng = np.random.default_rng(9)
    db.ctx.prof_enable(True)
    try:
        for n, flags in ((999, False), (1000, True), (1001, True)):
            col = np.where(rng.random(n) < 0.8, of_type[rng.integers(0, 1000, n)], rest[rng.integers(0, len(rest), n)])
            cols = col.astype(np.uint32).reshape(1, -1)
            src = db.ctx.table_from_host(_lib.TABLE_ORDERED, [20], cols)
            db.ctx.prof_reset()
            out = db.ctx.table_name_filter(src, 20, tid, dfa)
            ran = {k for k, v in db.ctx.prof_stats().items() if v["launches"]}
            assert ("k_name_filter_flags" in ran, "k_name_filter" in ran) == (flags, not flags), (n, ran)
            assert np.array_equal(out.fetch(), cols[:, _host_keep(world, col, tid, rx)])
    finally:
        db.ctx.prof_enable(False)
        db.ctx.prof_reset()


@pytest.mark.parametrize("name,mode_id", FILTER_MODES)
def test_filter_keeps_the_sorted_mark(db, world, name, mode_id):
    """A scan sorted by V2, filtered on V2, then joined with a scan: the rows
    of the host join (a wrong sorted mark or bound loses rows)."""
    from das_amd.name_search import compile_name_pattern
    tid, inh = db.type_id["D"], db.type_id["Inheritance"]
    dfa = compile_name_pattern("^[ab0-4]", ascii_only=True)
    rx = re.compile("^[ab0-4]")
    none = _lib.DAS_NONE
    src = db.ctx.scan_link(2, inh, [none, none], [30, 31], 0, True, False, False, 1)
    rows = src.fetch()
    assert np.all(np.diff(rows[1].astype(np.int64)) >= 0) and len(set(rows[1])) < rows.shape[1]
    out = db.ctx.table_name_filter(src, 31, tid, dfa, mode_id)
    keep = _host_keep(world, rows[1], tid, rx)
    assert np.array_equal(out.fetch(), rows[:, keep]) and 0 < out.nrows < src.nrows
    assert out.bounds() == src.bounds()
    other = db.ctx.scan_link(2, inh, [none, none], [31, 32], 0, True)
    orow = other.fetch()
    want = sorted((int(a), int(b), int(c)) for a, b in zip(*rows[:, keep]) for b2, c in zip(*orow) if b2 == b)
    for j in (db.ctx.join(other, out), db.ctx.join(out, other)):
        f = j.fetch()
        at = {v: k for k, v in enumerate(j.vars)}
        assert sorted(zip(*(f[at[v]].tolist() for v in (30, 31, 32)))) == want
    assert want
    # and operator A's table as the build side
    scan = db.ctx.scan_node_names(tid, dfa, 31)
    j = db.ctx.join(other, scan)
    f = j.fetch()
    at = {v: k for k, v in enumerate(j.vars)}
    keep_o = _host_keep(world, orow[0], tid, rx)
    assert sorted(zip(f[at[31]].tolist(), f[at[32]].tolist())) == sorted(zip(*orow[:, keep_o].tolist()))


@pytest.mark.parametrize("name,mode_id", FILTER_MODES)
def test_filter_of_a_deferred_cross_product(db, world, name, mode_id):
    from das_amd.name_search import compile_name_pattern
    tid = db.type_id["D"]
    dfa = compile_name_pattern("CoA|mus|^[ab]", ascii_only=True)
    rx = re.compile("CoA|mus|^[ab]")
    expr = build(["And", [L("Pair", [V("V5"), V("V6")]), GN]])
    words = pm._lower(expr, db, False)
    matched, _, tables = db.ctx.plan_execute(words, len(words) // _lib.PLAN_WORDS, False)
    assert matched and len(tables) == 1 and tables[0].nrows == 30 * 150
    t = tables[0]
    var = pm._vid("V2")
    out = db.ctx.table_name_filter(t, var, tid, dfa, mode_id)
    rows = t.fetch()
    keep = _host_keep(world, rows[t.vars.index(var)], tid, rx)
    assert np.array_equal(out.fetch(), rows[:, keep]) and 0 < out.nrows < t.nrows


def _accept_all():
    return SimpleNamespace(n_states=2, n_classes=2, start=0, eot_class=1, byte_class=np.zeros(256, np.uint8),
                           next=np.array([1, 1, 1, 1], np.uint16), accept=np.array([0, 1], np.uint8))


def test_filter_refuses_bad_arguments_before_any_launch(db):
    tid = db.type_id["D"]
    cols = np.arange(8, dtype=np.uint32).reshape(2, 4)
    t = db.ctx.table_from_host(_lib.TABLE_ORDERED, [20, 21], cols)
    u = db.ctx.table_from_host(_lib.TABLE_UNORDERED, [20, 21], cols)
    db.ctx.sync()
    _, cat, _, ty, _ = db._host_mirror()
    ok = db.ctx.table_name_filter(t, 20, tid, _accept_all())    # (the heap exists before the launches are counted)
    assert ok.nrows == sum(1 for v in range(4) if cat[v] == 1 and ty[v] == tid)
    bad = []
    d = _accept_all(); d.next = np.array([1, 2, 1, 1], np.uint16); bad.append(d)        # next state out of range
    d = _accept_all(); d.next = np.array([1, 1, 0, 1], np.uint16); bad.append(d)        # accepting, not absorbing
    d = _accept_all(); d.n_states = 1025; d.n_classes = 1; d.next = np.zeros(1025, np.uint16)
    d.accept = np.zeros(1025, np.uint8); bad.append(d)
    d = _accept_all(); d.n_states = 100; d.n_classes = 100; d.next = np.zeros(10000, np.uint16)
    d.accept = np.zeros(100, np.uint8); bad.append(d)
    launches = _lib.counters()[0]
    for d in bad:
        with pytest.raises(ValueError):
            db.ctx.table_name_filter(t, 20, tid, d)
        with pytest.raises(ValueError):
            db.ctx.scan_node_names(tid, d, 20)
    with pytest.raises(ValueError):
        db.ctx.table_name_filter(t, 22, tid, _accept_all())     # a variable the table lacks
    with pytest.raises(ValueError):
        db.ctx.table_name_filter(u, 20, tid, _accept_all())     # not an ordered table
    with pytest.raises(ValueError):
        db.ctx.table_name_filter(t, 20, 10 ** 6, _accept_all())
    with pytest.raises(ValueError):
        db.ctx.table_name_filter(t, 20, tid, _accept_all(), 3)
    with pytest.raises(ValueError):
        db.ctx.scan_node_names(10 ** 6, _accept_all(), 20)
    assert _lib.counters()[0] == launches
