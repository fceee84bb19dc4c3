"""get_matched_node_name on the device (das_match_node_names, names.hip)
against the host path it replaces: same handles, same order, for every
pattern of the CPU corpus (test_name_search.py) and node types whose ranges
and heap offsets are unaligned, with names around the kernel's staging size."""
import json
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest

from das_amd import _lib, loader
from das_amd.name_search import compile_name_pattern
from tests import name_search_corpus as C

pytestmark = pytest.mark.gpu

STAGE = _lib.NAME_STAGE_BYTES
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _seeded_names(rng, n, alphabet, lo, hi):
    out = set()
    while len(out) < n:
        out.add("".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))))
    return sorted(out)


def _types():
    rng = random.Random(11)
    d = _seeded_names(rng, 4990, "abc0123456789", 1, 40)
    d += ["ab c0", "a b", "mus123", "mus1234", "xmus123", "CoA", "acetyl-CoA", "n17", "Ab", "x" * 3]
    return {
        "A": ["a"],
        "B": _seeded_names(rng, 63, "ab7_m", 1, 9),
        "C": [""] + _seeded_names(rng, 64, "abcmn17.", 1, 12),
        "D": d,
        # longer than the staged bytes (walked from the heap), exactly the staged bytes, short
        # (the filler is no word character, so `re` itself stays linear on these names)
        "L": ["ab" + "-" * (64 * 1024 - 2) + "7", "b" + "-" * (STAGE - 2) + "a", "ab7"],
        # around the staged size, the tile's first byte at different alignments
        "M": ["m" + "-" * (STAGE + k - 1) + "a7" for k in (-3, -2, -1, 0, 13, 14, 15)] + ["a", "7"],
        "U": ["é", "naïve", "٣", "a٣7", "ma", "human", "x" * 70 + "é", ""],
    }


def _canonical(types, links):
    lines = [f"(: {t} Type)" for t in types] + ["(: Inheritance Type)"]
    for t, names in types.items():
        lines += [f'(: "{n}" {t})' for n in names]
    lines += [f'(Inheritance "{a[0]} {a[1]}" "{b[0]} {b[1]}")' for a, b in links]
    return "\n".join(lines) + "\n"


TYPES = _types()
LINKS = [(("A", "a"), ("B", TYPES["B"][0])), (("B", TYPES["B"][1]), ("C", TYPES["C"][2])),
         (("D", TYPES["D"][5]), ("D", TYPES["D"][6])), (("U", "é"), ("L", "ab7")), (("M", "a"), ("D", "CoA"))]


def _fresh_db():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_canonical(_canonical(TYPES, LINKS))
    return db


@pytest.fixture(scope="module")
def db():
    return _fresh_db()


@pytest.fixture(scope="module")
def nodes(db):
    """Per type: (handles, names) in the order the host path lists them
    (ascending id), computed once."""
    return {t: (db.get_all_nodes(t), db.get_all_nodes(t, names=True)) for t in list(TYPES) + ["Inheritance"]}


def _host(db, t, p, monkeypatch):
    monkeypatch.setenv("DAS_NAME_SEARCH", "0")
    try:
        return db.get_matched_node_name(t, p)
    finally:
        monkeypatch.delenv("DAS_NAME_SEARCH")


def test_path_taken_and_no_host_mirror():
    """First in the file: a fresh load answered by the device alone."""
    db = _fresh_db()
    bytes0 = int(db.ctx.stats().device_bytes)
    for p in C.MUST_COMPILE_ASCII:
        for t in ("A", "B", "C", "D", "L", "M"):
            before = dict(db.name_search_stats)
            db.get_matched_node_name(t, p)
            assert db.name_search_stats["device"] == before["device"] + 1, (t, p)
            assert db.name_search_stats["host"] == before["host"]
    for p in C.MUST_COMPILE_ANY:
        before = dict(db.name_search_stats)
        db.get_matched_node_name("U", p)
        assert db.name_search_stats["device"] == before["device"] + 1, p
    assert db._mirror is None
    # the heap exists now and is counted
    assert int(db.ctx.stats().device_bytes) > bytes0
    n_bytes = sum(len(n.encode()) for t in TYPES for n in TYPES[t])
    got = [db.ctx.node_name_stats(db.type_id[t]) for t in TYPES]
    assert [g[0] for g in got] == [len(TYPES[t]) for t in TYPES]
    assert sum(g[1] for g in got) == n_bytes
    assert [g[2] for g in got] == [t != "U" for t in TYPES]
    assert db.ctx.node_name_stats(db.type_id["Inheritance"]) == (0, 0, True)
    assert db._mirror is None
    # declined patterns: the host answers
    for p in C.DECLINE_ALWAYS:
        before = dict(db.name_search_stats)
        db.get_matched_node_name("D", p)
        assert db.name_search_stats == {"device": before["device"], "host": before["host"] + 1}, p
    for p in C.DECLINE_NON_ASCII:
        before = dict(db.name_search_stats)
        db.get_matched_node_name("U", p)
        assert db.name_search_stats == {"device": before["device"], "host": before["host"] + 1}, p
    assert db._mirror is not None


def test_node_lists(db, nodes):
    for t, names in TYPES.items():
        assert sorted(nodes[t][1]) == sorted(names)
        assert len(nodes[t][0]) == len(names)
    assert nodes["Inheritance"] == ([], [])


@pytest.mark.parametrize("t", list(TYPES) + ["Inheritance"])
def test_differential(db, nodes, t, monkeypatch):
    handles, names = nodes[t]
    for p in C.ALL_PATTERNS:
        rx = re.compile(p)
        want = [h for h, n in zip(handles, names) if rx.search(n)]
        got = db.get_matched_node_name(t, p)
        assert got == want, (t, p)
        assert _host(db, t, p, monkeypatch) == want, (t, p)


def test_long_names_are_walked_whole(db, nodes):
    """Matches that depend on the last byte of the names around and beyond
    the staged size."""
    for t in ("L", "M"):
        handles, names = nodes[t]
        for p in ("7$", "a$", "a7$", "^ab", "-7$", "^b-+a$", "^m-+a7$", "b$", "^[^7]+$"):
            assert compile_name_pattern(p, ascii_only=True) is not None
            before = db.name_search_stats["device"]
            want = [h for h, n in zip(handles, names) if re.search(p, n)]
            assert db.get_matched_node_name(t, p) == want, (t, p)
            assert db.name_search_stats["device"] == before + 1
    assert len(db.get_matched_node_name("L", "7$")) == 2 and len(db.get_matched_node_name("M", "a7$")) == 7


def test_name_bytes(db, nodes):
    """'^' + re.escape(name) + '$' returns exactly the nodes with that name."""
    rng = random.Random(3)
    sample = [(t, n) for t in ("A", "L", "M", "U") for n in TYPES[t]]
    rest = [(t, n) for t in ("B", "C", "D") for n in TYPES[t]]
    sample += rng.sample(rest, 200 - len(sample))
    device0 = db.name_search_stats["device"]
    for t, n in sample:
        got = db.get_matched_node_name(t, "^" + re.escape(n) + "$")
        assert got == [db.get_node_handle(t, n)], (t, n[:40])
    assert db.name_search_stats["device"] - device0 >= 150      # (the longest names and type U decline)


def test_edge_answers(db, nodes):
    for t in TYPES:
        assert db.get_matched_node_name(t, "") == nodes[t][0]
        assert db.get_matched_node_name(t, "no such name Q") == []
    assert db.get_matched_node_name("Nope", "a") == []
    assert db.get_matched_node_name("Inheritance", "") == []
    with pytest.raises(re.error):
        db.get_matched_node_name("D", "(")


def test_reference_case_animals():
    """redis_mongo_db_test.py:265-271"""
    from das_amd.database.hip_db import HipDB
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    db = HipDB(device=0)
    db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    want = sorted(db.get_node_handle("Concept", n) for n in ("human", "mammal", "animal"))
    assert sorted(db.get_matched_node_name("Concept", "ma")) == want
    assert db.get_matched_node_name("blah", "Concept") == []
    assert db.get_matched_node_name("Concept", "blah") == []
    assert db.name_search_stats == {"device": 2, "host": 0}


def test_load_metta_names(monkeypatch):
    """The name's start inside its leaf on the other loader, and a name that
    ends in a newline (which the canonical reader does not admit)."""
    from das_amd.database.hip_db import HipDB
    names = {"Concept": ["a\n", "a", "ma", "naïve b", "long name x"], "Vé": ["c", "b7", "é"]}
    text = "(: Concept Type)\n(: Vé Type)\n(: Inheritance Type)\n"
    text += "".join(f'(: "{n}" {t})\n' for t in names for n in names[t])
    # (this reader stores the terminals that an expression mentions)
    flat = [n for t in names for n in names[t]]
    text += "".join(f'(Inheritance "{a}" "{b}")\n' for a, b in zip(flat[0::2], flat[1::2]))
    db = HipDB(device=0)
    db.load_metta(text)
    assert db.ctx.node_name_stats(db.type_id["Concept"])[2] is False
    assert db.ctx.node_name_stats(db.type_id["Vé"])[2] is False
    for t in names:
        for n in names[t]:
            got = db.get_matched_node_name(t, "^" + re.escape(n) + r"\Z")
            assert got == [db.get_node_handle(t, n)], (t, n)
    assert db.name_search_stats == {"device": 8, "host": 0}
    assert db._mirror is None
    for t in names:
        handles, nm = db.get_all_nodes(t), db.get_all_nodes(t, names=True)
        assert sorted(nm) == sorted(names[t])
        for p in ("a$", r"a\Z", "^a", "a", ".", r"\s", "é", "", r"\d$"):
            want = [h for h, n in zip(handles, nm) if re.search(p, n)]
            assert db.get_matched_node_name(t, p) == want, (t, p)
            assert _host(db, t, p, monkeypatch) == want
    # `a$` matches "a\n", `a\Z` does not
    a_nl = db.get_node_handle("Concept", "a\n")
    assert a_nl in db.get_matched_node_name("Concept", "a$")
    assert a_nl not in db.get_matched_node_name("Concept", r"a\Z")


def _accept_all():
    return SimpleNamespace(n_states=2, n_classes=2, start=0, eot_class=1, byte_class=np.zeros(256, np.uint8),
                           next=np.array([1, 1, 1, 1], np.uint16), accept=np.array([0, 1], np.uint8))


def test_raw_abi(db, nodes):
    for t in ("A", "B", "C", "D"):
        tid = db.type_id[t]
        want = db.ids_of(nodes[t][0])
        assert list(want) == sorted(want)
        ids, n = db.ctx.match_node_names(tid, _accept_all())
        assert n == len(want) and np.array_equal(ids, want)
        cap = min(10, len(want) - 1)
        ids, n = db.ctx.match_node_names(tid, _accept_all(), cap=cap)
        assert n == len(want) and np.array_equal(ids, want[:cap])
    ids, n = db.ctx.match_node_names(db.type_id["Inheritance"], _accept_all())
    assert n == 0 and ids.size == 0


def test_raw_abi_rejects_a_bad_dfa(db):
    tid = db.type_id["D"]
    bad = []
    d = _accept_all(); d.next = np.array([1, 2, 1, 1], np.uint16); bad.append(d)        # next state out of range
    d = _accept_all(); d.next = np.array([1, 1, 0, 1], np.uint16); bad.append(d)        # accepting, not absorbing
    d = _accept_all(); d.start = 2; bad.append(d)
    d = _accept_all(); d.eot_class = 2; bad.append(d)
    d = _accept_all(); d.byte_class = np.full(256, 2, np.uint8); bad.append(d)
    d = _accept_all(); d.n_states = 0; bad.append(d)
    d = _accept_all(); d.n_states = 1025; d.n_classes = 1; d.next = np.zeros(1025, np.uint16)
    d.accept = np.zeros(1025, np.uint8); bad.append(d)
    d = _accept_all(); d.n_states = 100; d.n_classes = 100; d.next = np.zeros(10000, np.uint16)
    d.accept = np.zeros(100, np.uint8); bad.append(d)
    launches = _lib.counters()[0]
    for d in bad:
        with pytest.raises(ValueError):
            db.ctx.match_node_names(tid, d, cap=4)
    with pytest.raises(ValueError):
        db.ctx.match_node_names(10 ** 6, _accept_all(), cap=4)
    assert _lib.counters()[0] == launches


def test_rebuild_invalidates_the_heap():
    db = _fresh_db()
    assert len(db.get_matched_node_name("D", "^a")) > 0
    other = {"D": ["zz", "a1"], "Q": ["a", "b"]}
    db.load_canonical(_canonical(other, [(("D", "zz"), ("Q", "a"))]))
    assert db.get_matched_node_name("D", "^a") == [db.get_node_handle("D", "a1")]
    assert db.get_matched_node_name("D", "z+$") == [db.get_node_handle("D", "zz")]
    assert sorted(db.get_matched_node_name("Q", "")) == sorted(db.get_node_handle("Q", n) for n in "ab")
    assert db.get_matched_node_name("B", "") == []
    assert db.ctx.node_name_stats(db.type_id["D"]) == (2, 4, True)
    assert db._mirror is None
