"""Rows of an answer per value of a variable, the parts that need no GPU: the
host definition value_counts_host and the ValueCounts value object, over the
oracle DB on the animals and toy-mining KBs.  The truth is a Counter the test
writes out itself from the oracle's rows, never the code under test."""
import json
import os
from collections import Counter

import numpy as np
import pytest

from das_amd.distributed_atom_space import DistributedAtomSpace
from das_amd.pattern_matcher import pattern_matcher as PM
from oracle import das_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _kb(name):
    with open(os.path.join(GOLDEN, name)) as f:
        d = json.load(f)
    odb = O.RedisMongoSemantics(O.KB.from_tables(d["nodes"], d["links"]))
    return odb, {h: n for h, t, n in d["nodes"]}


@pytest.fixture(scope="module")
def animals():
    return _kb("kb_animals.json")


@pytest.fixture(scope="module")
def toy():
    return _kb("kb_toy_mining.json")


def _answer(spec, odb):
    """The oracle's answer to `spec` as a PatternMatchingAnswer whose
    assignments are set by hand, and the oracle's rows."""
    oa = O.Answer()
    matched = O.matched(spec, odb, oa)
    out = []
    for row in oa.rows:
        if row[0] == "O":
            a = PM.OrderedAssignment()
            for var, value in row[1]:
                assert a.assign(var, value)
        else:
            assert row[0] == "U"
            a = PM.UnorderedAssignment()
            for var, value in zip(sorted(row[1]), row[2]):
                assert a.assign(var, value)
        assert a.freeze()
        out.append(a)
    ans = PM.PatternMatchingAnswer()
    ans.assignments = out
    return matched, ans, list(oa.rows)


def _want(rows, v):
    return Counter(dict(r[1])[v] for r in rows)


LINK = ["Link", "Inheritance", True, [["Var", "V1"], ["Var", "V2"]]]
CHAIN = ["And", [["Link", "Inheritance", True, [["Var", "V1"], ["Var", "V2"]]],
                 ["Link", "Inheritance", True, [["Var", "V2"], ["Var", "V3"]]]]]
# the toy-mining KB has no chain of two Inheritance links: its And shares the parent
SIBLINGS = ["And", [["Link", "Inheritance", True, [["Var", "V1"], ["Var", "V2"]]],
                    ["Link", "Inheritance", True, [["Var", "V3"], ["Var", "V2"]]]]]
EITHER = ["Or", [["Link", "Inheritance", True, [["Var", "V1"], ["Var", "V2"]]],
                 ["Link", "Similarity", True, [["Var", "V1"], ["Var", "V2"]]]]]


@pytest.mark.parametrize("kb", ["animals", "toy"])
@pytest.mark.parametrize("spec, variables", [(LINK, ("V1", "V2")), (CHAIN, ("V1", "V2", "V3")),
                                             (EITHER, ("V1", "V2"))], ids=["link", "and", "or"])
def test_value_counts_host_is_the_counter(kb, spec, variables, request):
    odb, name_of = request.getfixturevalue(kb)
    if spec is CHAIN and kb == "toy":
        spec = SIBLINGS
    matched, ans, rows = _answer(spec, odb)
    assert matched and len(rows) > 3
    for v in variables:
        want = _want(rows, v)
        assert PM.value_counts_host(odb, ans, v) == want
        vc = ans.value_counts(v, db=odb)
        assert vc.ids is None and vc.as_dict() == dict(want)
        assert vc.counts.dtype == np.uint64 and len(vc) == len(want)
        assert vc.total == len(rows) == ans.count()
        assert vc.handles == sorted(want)
        assert vc.names() == [name_of[h] for h in sorted(want)]
        assert ans.distinct(v, db=odb) == sorted(want)
    # a grouping that is not one row per value
    assert max(_want(rows, variables[-1]).values()) > 1


def test_unordered_answer_is_an_attribute_error(animals):
    odb, _ = animals
    spec = ["Link", "Similarity", False, [["Var", "V1"], ["Var", "V2"]]]
    matched, ans, rows = _answer(spec, odb)
    assert matched and rows and all(r[0] == "U" for r in rows)
    with pytest.raises(AttributeError):
        PM.value_counts_host(odb, ans, "V1")
    with pytest.raises(AttributeError):
        ans.value_counts("V1", db=odb)


def test_unbound_variable_is_a_key_error(animals):
    odb, _ = animals
    _, ans, _ = _answer(CHAIN, odb)
    with pytest.raises(KeyError) as e:
        PM.value_counts_host(odb, ans, "V9")
    assert e.value.args == ("V9",)
    with pytest.raises(KeyError):
        ans.value_counts("V9", db=odb)
    with pytest.raises(KeyError):
        ans.distinct("V9", db=odb)


def test_most_common_order_is_deterministic(animals):
    """Count descending, ties by handle ascending, whatever order the values
    arrived in; names and k follow that order."""
    odb, name_of = animals
    _, ans, rows = _answer(LINK, odb)
    ties = 0
    for v in ("V1", "V2"):
        want = _want(rows, v)
        order = sorted(want.items(), key=lambda kv: (-kv[1], kv[0]))
        ties += len(order) - len({n for _, n in order})
        vc = ans.value_counts(v, db=odb)
        assert vc.most_common() == order
        assert vc.most_common(2) == order[:2] and vc.most_common(0) == []
        assert vc.most_common(10 ** 6) == order
        assert vc.most_common(3, names=True) == [(name_of[h], n) for h, n in order[:3]]
        # built from the same counts in another insertion order
        again = PM.ValueCounts(odb, counter=Counter(dict(reversed(list(want.items())))))
        assert again.most_common() == order
    assert ties > 2                                              # the KB has ties to break


def test_empty_answer():
    ans = PM.PatternMatchingAnswer()
    ans.assignments = []
    for vc in (ans.value_counts("V1"), PM.ValueCounts(None, counter=Counter())):
        assert len(vc) == 0 and vc.total == 0
        assert vc.handles == [] and vc.as_dict() == {} and vc.most_common(3) == [] and vc.names() == []
        assert vc.counts.dtype == np.uint64
    assert ans.distinct("V1") == []
    empty = PM.ValueCounts(None, ids=np.zeros(0, np.uint32), counts=np.zeros(0, np.uint64))
    assert len(empty) == 0 and empty.total == 0 and empty.handles == [] and empty.most_common() == []


def test_counts_above_32_bits_are_kept():
    vc = PM.ValueCounts(None, counter=Counter({"b" * 32: 70000 * 70000, "a" * 32: 1}))
    assert vc.total == 70000 * 70000 + 1
    assert vc.most_common(1) == [("b" * 32, 4900000000)]


class _Query:
    def __init__(self, matched, rows):
        self.m, self.rows = matched, rows

    def matched(self, db, answer):
        answer.assignments = self.rows
        return self.m


def test_facade_value_counts(animals):
    odb, name_of = animals
    das = DistributedAtomSpace(db=odb)
    _, ans, rows = _answer(CHAIN, odb)
    want = _want(rows, "V3")
    order = sorted(want.items(), key=lambda kv: (-kv[1], kv[0]))
    q = _Query(True, ans.assignments)
    assert das.value_counts(q, "V3").as_dict() == dict(want)
    assert das.value_counts(q, "V3", top=3) == order[:3]
    assert das.value_counts(q, "V3", top=3, names=True) == [(name_of[h], n) for h, n in order[:3]]
    assert das.value_counts(q, "V3", names=True) == [(name_of[h], n) for h, n in order]
    miss = das.value_counts(_Query(False, ans.assignments), "V3")
    assert len(miss) == 0 and miss.total == 0
    assert das.value_counts(_Query(False, ans.assignments), "V3", top=3) == []
