"""Bulk node-name fetch, the parts that need no GPU: decoding das_node_names'
(off, bytes, kind), the argument checks of Context.node_names, and the host
definitions of PatternMatchingAnswer.names / get_mappings / get_node_names
over the oracle DB on the animals KB.  The truth is the node table the test
itself loaded (handle -> name), never the code under test."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from das_amd import _lib
from das_amd.distributed_atom_space import DistributedAtomSpace
from das_amd.pattern_matcher import pattern_matcher as PM
from oracle import das_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------
# decode_names
# ---------------------------------------------------------------------------

def _pack(names):
    """(off, bytes, kind) as the device call lays them out; None = not a node."""
    enc = [b"" if n is None else n.encode("utf-8") for n in names]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(e) for e in enc])
    data = np.frombuffer(b"".join(enc), dtype=np.uint8)
    kind = np.array([0 if n is None else 1 for n in names], dtype=np.uint8)
    return off, data, kind


@pytest.mark.parametrize("names", [
    [],
    [""],
    ["a"],
    ["human", "", "monkey", "a b", "x" * 300],
    ["é", "naïve", "٣", "", "plain", "a٣7"],
    [None],
    ["a", None, "", None, "é", None],
])
def test_decode_names(names):
    assert _lib.decode_names(*_pack(names)) == names


def test_decode_names_rejects_bad_input():
    off, data, kind = _pack(["ab", "c"])
    with pytest.raises(ValueError):
        _lib.decode_names(off[:-1], data, kind)                 # one offset short
    with pytest.raises(ValueError):
        _lib.decode_names(off, data[:-1], kind)                 # bytes missing (a capacity that was too small)
    with pytest.raises(ValueError):
        _lib.decode_names(np.array([0, 3, 2], dtype=np.uint64), data, kind)
    with pytest.raises(ValueError):
        _lib.decode_names(np.array([1, 2, 3], dtype=np.uint64), data, kind)


# ---------------------------------------------------------------------------
# Context.node_names: argument errors, raised before the library is touched
# ---------------------------------------------------------------------------

def test_node_names_argument_errors():
    ctx = _lib.Context.__new__(_lib.Context)            # no device context: every error below comes first
    ctx.h = None
    table = SimpleNamespace(vars=(0, 1), nrows=5, h=None)
    with pytest.raises(ValueError):
        ctx.node_names()
    with pytest.raises(ValueError):
        ctx.node_names(ids=np.zeros(1, np.uint32), table=table)
    for kw in ({"col": 2}, {"col": -1}, {"row0": 6}, {"row0": -1}, {"row0": 3, "nrows": 3}, {"nrows": -1}):
        with pytest.raises(ValueError):
            ctx.node_names(table=table, **kw)
    ids = np.arange(3, dtype=np.uint32)
    with pytest.raises(ValueError):
        ctx.node_names(ids=ids, out=np.zeros(8, np.uint32))
    with pytest.raises(ValueError):
        ctx.node_names(ids=ids, out=np.zeros((2, 8), np.uint8))
    with pytest.raises(ValueError):
        ctx.node_names(ids=ids, out=np.zeros(8, np.uint8), cap=9)
    with pytest.raises(ValueError):
        ctx.node_names(ids=ids, cap=-1)


def test_copy_threshold_agrees_with_the_header():
    import re
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "das_mi355x.h")).read()
    assert int(re.search(r"#define DAS_NAME_COPY_WAVE (\d+)", src).group(1)) == _lib.NAME_COPY_WAVE


# ---------------------------------------------------------------------------
# the host definitions over the oracle
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def animals():
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    odb = O.RedisMongoSemantics(O.KB.from_tables(d["nodes"], d["links"]))
    name_of = {h: n for h, t, n in d["nodes"]}
    return odb, name_of


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


CHAIN = ["And", [["Link", "Inheritance", True, [["Var", "V1"], ["Var", "V2"]]],
                 ["Link", "Inheritance", True, [["Var", "V2"], ["Var", "V3"]]]]]


def test_names_host_one_variable(animals):
    odb, name_of = animals
    matched, ans, rows = _answer(CHAIN, odb)
    assert matched and len(rows) > 3
    for v in ("V1", "V2", "V3"):
        want = sorted(name_of[dict(r[1])[v]] for r in rows)
        assert sorted(PM.names_host(odb, ans, v)) == want
        assert sorted(ans.names(v, db=odb)) == want
    assert len(set(want)) > 1


def test_names_host_all_variables_are_aligned(animals):
    odb, name_of = animals
    _, ans, rows = _answer(CHAIN, odb)
    got = ans.names(db=odb)
    assert sorted(got) == ["V1", "V2", "V3"]
    want = sorted(tuple(name_of[dict(r[1])[v]] for v in ("V1", "V2", "V3")) for r in rows)
    assert sorted(zip(got["V1"], got["V2"], got["V3"])) == want
    assert got == PM.names_host(odb, ans)


def test_names_host_unbound_variable_is_a_key_error(animals):
    odb, _ = animals
    _, ans, _ = _answer(CHAIN, odb)
    with pytest.raises(KeyError):
        PM.names_host(odb, ans, "V9")
    with pytest.raises(KeyError):
        ans.names("V9", db=odb)


def test_names_host_unordered_answer(animals):
    """A Similarity answer of unordered assignments has no per-variable
    mapping: the definition's own AttributeError, as the notebook's loop."""
    odb, _ = animals
    spec = ["Link", "Similarity", False, [["Var", "V1"], ["Var", "V2"]]]
    matched, ans, rows = _answer(spec, odb)
    assert matched and rows and all(r[0] == "U" for r in rows)
    with pytest.raises(AttributeError):
        [odb.get_node_name(a.mapping["V1"]) for a in ans.assignments]
    with pytest.raises(AttributeError):
        PM.names_host(odb, ans, "V1")
    with pytest.raises(AttributeError):
        ans.names("V1", db=odb)


def test_names_host_ordered_similarity(animals):
    """The notebooks' ordered Similarity links bind each variable."""
    odb, name_of = animals
    spec = ["Link", "Similarity", True, [["Var", "V1"], ["Var", "V2"]]]
    matched, ans, rows = _answer(spec, odb)
    assert matched and rows
    want = sorted((name_of[dict(r[1])["V1"]], name_of[dict(r[1])["V2"]]) for r in rows)
    got = ans.names(db=odb)
    assert sorted(zip(got["V1"], got["V2"])) == want


def test_names_host_strict(animals):
    """A value that is not a node: ValueError with get_node_name's text, or None."""
    odb, name_of = animals
    link = next(iter(odb.kb.links))
    node = next(iter(odb.kb.nodes))
    rows = []
    for value in (node, link):
        a = PM.OrderedAssignment()
        a.assign("V1", value)
        a.freeze()
        rows.append(a)
    ans = PM.PatternMatchingAnswer()
    ans.assignments = rows
    with pytest.raises(ValueError, match=f"Invalid handle: {link}"):
        ans.names("V1", db=odb)
    assert sorted(ans.names("V1", strict=False, db=odb), key=str) == sorted([name_of[node], None], key=str)


def test_empty_answer():
    ans = PM.PatternMatchingAnswer()
    ans.assignments = []
    assert ans.names("V1") == [] and ans.names() == {}


class _Query:
    def __init__(self, matched, rows):
        self.m, self.rows = matched, rows

    def matched(self, db, answer):
        answer.assignments = self.rows
        return self.m


def test_facade_get_mappings_and_get_node_names(animals):
    odb, name_of = animals
    das = DistributedAtomSpace(db=odb)
    _, ans, rows = _answer(CHAIN, odb)
    want = sorted(name_of[dict(r[1])["V2"]] for r in rows)
    assert sorted(das.get_mappings(_Query(True, ans.assignments), "V2")) == want
    assert das.get_mappings(_Query(False, ans.assignments), "V2") == []
    handles = list(name_of)
    assert das.get_node_names(handles) == [name_of[h] for h in handles]
    link = next(iter(odb.kb.links))
    with pytest.raises(ValueError, match=f"Invalid handle: {link}"):
        das.get_node_names(handles[:2] + [link] + ["nonsense"])
    assert das.get_node_names(handles[:2] + [link], strict=False) == [name_of[h] for h in handles[:2]] + [None]
