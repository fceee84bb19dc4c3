"""Node names of ids and of whole answer columns in one device call
(das_node_names, names.hip): HipDB.get_node_names, PatternMatchingAnswer.names,
DistributedAtomSpace.get_mappings and get_all_nodes over the name heap.

The truth is the names this file loaded: name -> get_node_handle -> id ->
fetched name must be the name again.  Name lengths sit around every size at
which the copy kernel changes path (a lane's own copy up to NAME_COPY_WAVE
bytes, a wave's above; 16-byte vectors; a tile's LDS image), and the names are
fetched behind pads of 0..15 bytes so that every destination alignment occurs;
the source alignments that occur are computed from the ids and asserted."""
import json
import os
import random

import numpy as np
import pytest

from das_amd import _lib, loader
from das_amd.pattern_matcher import pattern_matcher as PM
from das_amd.pattern_matcher.pattern_matcher import And, Link, Node, PatternMatchingAnswer, Variable

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = _lib.NAME_COPY_WAVE
BIG = 64 * 1024 + 1
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, BIG, T - 1, T, T + 1]
ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_"      # 63 symbols: no period of 2^k
VARIANTS = 20           # names per length up to T, twice as many above (every source alignment shows up: asserted)
BIG_VARIANTS = 4


def _name(length, variant):
    """A name of `length` bytes; variants differ, and no two windows of it
    that a misplaced copy could confuse are equal."""
    if length == 0:
        return ""
    if length == 1:
        return ALPHABET[variant]
    body = (ALPHABET[variant % 63:] + ALPHABET * (length // 63 + 1))[:length - 2]
    return f"{variant:02d}"[:2] + body


def _corpus():
    names = {"N": [], "M": ["m", "mammal-like", "x" * 40, "é", "m" * 65]}
    for length in sorted(set(LENGTHS)):
        k = 1 if length == 0 else BIG_VARIANTS if length == BIG else VARIANTS if length <= T else 2 * VARIANTS
        names["N"] += [_name(length, v) for v in range(k)]
    # pads of 1..15 bytes (the empty name is the pad of 0), told apart from the names above by '-'
    names["N"] += ["-" * length for length in range(1, 16)]
    # multi-byte names behind 0..7 ASCII bytes: some straddle a 4-byte boundary wherever they land
    for word in ("é", "naïve", "٣"):
        names["N"] += ["+" * k + word for k in range(8)]
    assert len(set(names["N"])) == len(names["N"])
    return names


NAMES = _corpus()
LINKS = [(("M", "m"), ("M", "é")), (("M", "mammal-like"), ("N", "-")), (("M", "x" * 40), ("M", "m" * 65))]


def _canonical(types, links, link_type="Inheritance"):
    lines = [f"(: {t} Type)" for t in types] + [f"(: {link_type} Type)"]
    for t, names in types.items():
        lines += [f'(: "{n}" {t})' for n in names]
    lines += [f"({link_type} " + " ".join(f'"{t} {n}"' for t, n in tg) + ")" for tg in links]
    return "\n".join(lines) + "\n"


def _fresh_db():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_canonical(_canonical(NAMES, LINKS))
    return db


@pytest.fixture(scope="module")
def db():
    d = _fresh_db()
    d.NAME_FETCH_MIN = 0          # every call below is meant for the device
    return d


@pytest.fixture(scope="module")
def kb(db):
    """The loaded nodes once: (type, name) pairs, their ids, and where each
    name lies in the heap (nodes in ascending id order, names back to back)."""
    pairs = [(t, n) for t in NAMES for n in NAMES[t]]
    ids = db.ids_of([db.get_node_handle(t, n) for t, n in pairs])
    assert (ids >= 0).all() and len(set(ids.tolist())) == len(pairs)
    src, at = {}, 0
    for i in np.argsort(ids).tolist():
        src[pairs[i]] = at
        at += len(pairs[i][1].encode())
    link_ids = db.ids_of([db.get_link_handle("Inheritance", [db.get_node_handle(*a), db.get_node_handle(*b)])
                          for a, b in LINKS])
    assert (link_ids >= 0).all()
    return {"pairs": pairs, "ids": ids.astype(np.uint32), "src": src, "id_of": dict(zip(pairs, ids.tolist())),
            "links": link_ids.astype(np.uint32), "n_atoms": int(db.ctx.stats().n_atoms)}


def _fetch(db, ids, **kw):
    off, data, kind = db.ctx.node_names(ids=np.asarray(ids, dtype=np.uint32), **kw)
    return off, data, kind


def _check(db, ids, names):
    """One device call answers `ids` with `names` (None: not a node)."""
    off, data, kind = _fetch(db, ids)
    lens = [0 if n is None else len(n.encode()) for n in names]
    assert off.tolist() == [0] + np.cumsum(lens, dtype=np.int64).tolist()
    assert kind.tolist() == [0 if n is None else 1 for n in names]
    got = _lib.decode_names(off, data, kind)
    if got != names:                                # (no megabyte-long assertion message)
        bad = [i for i, (g, w) in enumerate(zip(got, names)) if g != w]
        raise AssertionError(f"{len(bad)} names differ, first at {bad[0]}: length {lens[bad[0]]}")
    return off


def test_first_call_builds_the_heap():
    """First in the file: a fresh DB's first fetch builds the heap, by the
    device alone."""
    fresh = _fresh_db()
    bytes0 = int(fresh.ctx.stats().device_bytes)
    assert fresh.get_node_names([fresh.get_node_handle("M", "mammal-like"), fresh.get_node_handle("N", "")]) == \
        ["mammal-like", ""]
    assert fresh.name_fetch_stats == {"device": 1, "host": 0}
    assert int(fresh.ctx.stats().device_bytes) > bytes0
    assert fresh._mirror is None


def test_every_length_at_every_alignment(db, kb):
    pairs = [p for p in kb["pairs"] if p[0] == "N"]
    ids = [kb["id_of"][p] for p in pairs]
    names = [n for _, n in pairs]
    dst = {}
    for pad in range(16):
        off = _check(db, [kb["id_of"][("N", "-" * pad)]] + ids, ["-" * pad] + names)
        for p, o in zip(pairs, off[1:-1].tolist()):
            dst.setdefault(p, set()).add(o % 16)
    assert all(v == set(range(16)) for v in dst.values())
    # where the sources lie: every alignment among a lane's names and among a wave's names
    # (a 64 KiB name: few of them, but behind the 16 pads its source lies at every offset from its destination)
    by_class = {"lane": set(), "wave": set()}
    for p in pairs:
        ln = len(p[1].encode())
        if ln and ln != BIG:
            by_class["lane" if ln <= T else "wave"].add(kb["src"][p] % 16)
        if ln == BIG:
            assert {(kb["src"][p] - d) % 16 for d in dst[p]} == set(range(16))
    assert by_class["lane"] == set(range(16)) and by_class["wave"] == set(range(16)), by_class
    # a multi-byte character across a 4-byte boundary of the heap
    straddle = 0
    for t, n in pairs:
        at = kb["src"][(t, n)]
        for ch in n:
            w = len(ch.encode())
            straddle += w > 1 and at // 4 != (at + w - 1) // 4
            at += w
    assert straddle >= 3


ORDERS = ("ascending", "descending", "shuffled")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_counts_and_orders(db, kb, n):
    rng = random.Random(n)
    small = [p for p in kb["pairs"] if len(p[1]) != BIG]
    for order in ORDERS:
        pick = rng.sample(small, n)
        if order != "shuffled":
            pick.sort(key=lambda p: kb["id_of"][p], reverse=order == "descending")
        ids = np.array([kb["id_of"][p] for p in pick], dtype=np.uint32)
        names = [p[1] for p in pick]
        _check(db, ids, names)
        before = dict(db.name_fetch_stats)
        assert db.get_node_names(ids) == names
        assert db.get_node_names([db.get_node_handle(*p) for p in pick]) == names
        assert db.name_fetch_stats == {"device": before["device"] + 2, "host": before["host"]}
    assert db._mirror is None


def test_repeats(db, kb):
    one = ("N", _name(17, 3))
    _check(db, [kb["id_of"][one]] * 300, [one[1]] * 300)
    big = ("N", _name(BIG, 3))
    other = ("N", _name(5, 1))
    _check(db, [kb["id_of"][p] for p in (big, other, big)], [big[1], other[1], big[1]])


def test_not_nodes(db, kb):
    a, b = ("N", _name(64, 0)), ("M", "é")
    link = int(kb["links"][0])
    ids = np.array([kb["id_of"][a], link, _lib.DAS_NONE, kb["id_of"][b], kb["n_atoms"], kb["id_of"][a]],
                   dtype=np.uint32)
    want = [a[1], None, None, b[1], None, a[1]]
    _check(db, ids, want)
    assert db.get_node_names(ids, strict=False) == want
    link_handle = db.hex_of(ids[1:2])[0]
    with pytest.raises(ValueError, match=f"Invalid handle: {link_handle}"):
        db.get_node_names(ids)
    handles = [db.get_node_handle(*a), link_handle, "0" * 32, db.get_node_handle(*b)]
    assert db.get_node_names(handles, strict=False) == [a[1], None, None, b[1]]
    with pytest.raises(ValueError, match=f"Invalid handle: {link_handle}"):
        db.get_node_names(handles)
    with pytest.raises(ValueError, match="Invalid handle: " + "0" * 32):
        db.get_node_names(handles[2:])
    # all of them no nodes: nothing to copy
    _check(db, ids[[1, 2, 4]], [None, None, None])


def test_capacity_smaller_than_the_total(db, kb):
    big = ("N", _name(BIG, 2))
    pick = [("N", _name(63, 1)), ("N", _name(5, 4)), ("M", "é"), big, ("N", _name(257, 7)), ("N", _name(16, 9))]
    ids = [kb["id_of"][p] for p in pick]
    whole = b"".join(p[1].encode() for p in pick)
    total = len(whole)
    for cap in (0, 1, 15, 16, 17, 66, 70, 70 + BIG // 2, 70 + BIG + 100, total - 1, total):
        out = np.full(total + 64, 0xAA, dtype=np.uint8)
        off, data, kind = _fetch(db, ids, cap=cap, out=out)
        assert int(off[-1]) == total and kind.all()
        assert data.size == min(cap, total) and bytes(data) == whole[:cap]
        assert (out[cap:] == 0xAA).all()
    # the same inside one tile's image: short names only
    pick = [p for p in kb["pairs"] if 0 < len(p[1]) < 20][:40]
    ids = [kb["id_of"][p] for p in pick]
    whole = b"".join(p[1].encode() for p in pick)
    for cap in (3, 16, 31, len(whole) - 1):
        out = np.full(len(whole) + 64, 0xAA, dtype=np.uint8)
        off, data, kind = _fetch(db, ids, cap=cap, out=out)
        assert int(off[-1]) == len(whole) and bytes(data) == whole[:cap] and (out[cap:] == 0xAA).all()


# ---------------------------------------------------------------------------
# answers: names of table columns
# ---------------------------------------------------------------------------

def _animals_db():
    from das_amd.database.hip_db import HipDB
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    db = HipDB(device=0)
    db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    return db, {h: n for h, t, n in d["nodes"]}


S1, S2 = "Schema:gene_map_table_recombination_loc", "Schema:gene_uniquename"
GENES = {f"FBgn{k:07d}": (f"1-{k % 5}", f"gene{k}") for k in range(23)}      # id -> (location, unique name)


def _flybase_db():
    """Execution(Schema, gene, Verbatim) rows as QueryFlyBase.ipynb reads them."""
    from das_amd.database.hip_db import HipDB
    verb = sorted(set(GENES) | {v for pair in GENES.values() for v in pair})
    links = []
    for g, (loc, uniq) in GENES.items():
        links.append((("Schema", S1), ("Verbatim", g), ("Verbatim", loc)))
        links.append((("Schema", S2), ("Verbatim", uniq), ("Verbatim", g)))
    db = HipDB(device=0)
    db.load_canonical(_canonical({"Schema": [S1, S2], "Verbatim": verb}, links, "Execution"))
    return db


def _flybase_query(gene):
    v1, v2, v3 = Variable("v1"), Variable("v2"), Variable("v3")
    s1, s2, n1 = Node("Schema", S1), Node("Schema", S2), Node("Verbatim", gene)
    return And([Link("Execution", [s1, n1, v1], True), Link("Execution", [s1, v2, v1], True),
                Link("Execution", [s2, v3, v2], True)])


def _rows(d, variables):
    return sorted(zip(*[d[v] for v in variables]))


def _device_and_host(db, query, variables):
    """answer.names() by the device path, and the host definition's rows."""
    ans = PatternMatchingAnswer()
    assert query.matched(db, ans)
    before = dict(db.name_fetch_stats)
    got = ans.names()
    assert db.name_fetch_stats == {"device": before["device"] + len(variables), "host": before["host"]}
    assert db._mirror is None
    assert sorted(got) == sorted(variables)
    host = PM.names_host(db, ans)
    assert _rows(got, variables) == _rows(host, variables)
    for v in variables:
        assert sorted(ans.names(v)) == sorted(host[v])
    with pytest.raises(KeyError):
        ans.names("no_such_variable")
    return ans, got


def test_answer_names_animals():
    db, name_of = _animals_db()
    q = And([Link("Inheritance", [Variable("V1"), Variable("V2")], True),
             Link("Inheritance", [Variable("V2"), Variable("V3")], True)])
    ans, got = _device_and_host(db, q, ["V1", "V2", "V3"])
    # the truth: the rows' handles through the node table this test loaded
    want = sorted(tuple(name_of[a.mapping[v]] for v in ("V1", "V2", "V3")) for a in ans.assignments)
    assert _rows(got, ["V1", "V2", "V3"]) == want and len(want) > 3
    # sub-ranges of a column
    (t,) = db.rel_local_tables(ans._rel)
    full = _lib.decode_names(*db.ctx.node_names(table=t, col=1))
    assert len(full) == t.nrows
    for row0, nrows in ((0, 1), (2, 3), (t.nrows - 1, 1), (t.nrows, 0), (1, None)):
        sub = _lib.decode_names(*db.ctx.node_names(table=t, col=1, row0=row0, nrows=nrows))
        assert sub == full[row0:] if nrows is None else sub == full[row0:row0 + nrows]
    with pytest.raises(ValueError):
        db.ctx.node_names(table=t, col=1, row0=1, nrows=t.nrows)
    # the facade: one call per question
    q = Link("Inheritance", [Variable("V1"), Variable("V2")], True)
    from das_amd.distributed_atom_space import DistributedAtomSpace
    das = DistributedAtomSpace(db=db)
    assert sorted(das.get_mappings(q, "V1")) == sorted(name_of[a.mapping["V1"]] for a in _answer(db, q).assignments)
    false_q = Link("Inheritance", [Node("Concept", "human"), Node("Concept", "no such animal")], True)
    assert das.get_mappings(false_q, "V1") == []
    handles = list(name_of)
    assert das.get_node_names(handles) == [name_of[h] for h in handles]


def _answer(db, q):
    ans = PatternMatchingAnswer()
    assert q.matched(db, ans)
    return ans


def test_answer_names_similarity():
    db, name_of = _animals_db()
    # ordered, as the notebooks write it: the device path
    _, got = _device_and_host(db, Link("Similarity", [Variable("V1"), Variable("V2")], True), ["V1", "V2"])
    assert len(got["V1"]) > 0
    # unordered assignments: the host path, which has no per-variable value to name
    ans = _answer(db, Link("Similarity", [Variable("V1"), Variable("V2")], False))
    before = dict(db.name_fetch_stats)
    with pytest.raises(AttributeError):
        PM.names_host(db, ans, "V1")
    with pytest.raises(AttributeError):
        ans.names("V1")
    assert db.name_fetch_stats == {"device": before["device"], "host": before["host"] + 1}


def test_answer_names_flybase(monkeypatch):
    db = _flybase_db()
    from das_amd.distributed_atom_space import DistributedAtomSpace
    das = DistributedAtomSpace(db=db)
    gene = "FBgn0000007"
    same_loc = sorted(g for g, (loc, _) in GENES.items() if loc == GENES[gene][0])
    assert len(same_loc) > 2
    q = _flybase_query(gene)
    _, got = _device_and_host(db, q, ["v1", "v2", "v3"])
    assert _rows(got, ["v1", "v2", "v3"]) == sorted((GENES[g][0], g, GENES[g][1]) for g in same_loc)
    before = dict(db.name_fetch_stats)
    assert sorted(das.get_mappings(q, "v2")) == same_loc
    assert db.name_fetch_stats == {"device": before["device"] + 1, "host": before["host"]}
    assert das.get_mappings(_flybase_query("FBgn9999999"), "v2") == []
    # the host loop, as the parent commit ran it
    monkeypatch.setenv("DAS_NAME_FETCH", "0")
    before = dict(db.name_fetch_stats)
    assert sorted(das.get_mappings(q, "v2")) == same_loc
    assert db.name_fetch_stats == {"device": before["device"], "host": before["host"] + 1}


def test_switch_to_the_host_loop_after_prefetch():
    """After prefetch() a few names are a host lookup each: the loop answers
    below NAME_FETCH_MIN_PREFETCHED, the device call from there on."""
    db, name_of = _animals_db()
    handles = list(name_of)[:5]
    want = [name_of[h] for h in handles]
    assert db.get_node_names(handles) == want and db.name_fetch_stats == {"device": 1, "host": 0}
    db.prefetch()
    assert db.get_node_names(handles) == want and db.name_fetch_stats == {"device": 1, "host": 1}
    many = handles * (db.NAME_FETCH_MIN_PREFETCHED // len(handles) + 1)
    assert db.get_node_names(many) == want * (len(many) // len(handles))
    assert db.name_fetch_stats == {"device": 2, "host": 1}


# ---------------------------------------------------------------------------
# get_all_nodes
# ---------------------------------------------------------------------------

def test_get_all_nodes_equals_the_host_path(monkeypatch):
    db = _fresh_db()
    types = list(NAMES) + ["Inheritance", "NoSuchType"]
    before = dict(db.name_fetch_stats)
    dev = {t: (db.get_all_nodes(t), db.get_all_nodes(t, names=True)) for t in types}
    assert db.name_fetch_stats == {"device": before["device"] + 2 * (len(types) - 1), "host": before["host"]}
    assert db._mirror is None
    for t in NAMES:
        assert sorted(dev[t][1]) == sorted(NAMES[t])
        assert dev[t][0] == [db.get_node_handle(t, n) for n in dev[t][1]]
    assert dev["Inheritance"] == ([], []) and dev["NoSuchType"] == ([], [])
    monkeypatch.setenv("DAS_NAME_FETCH", "0")
    for t in types:
        assert (db.get_all_nodes(t), db.get_all_nodes(t, names=True)) == dev[t]


# ---------------------------------------------------------------------------
# lifecycle
# ---------------------------------------------------------------------------

def test_reload_returns_the_new_names():
    fresh = _fresh_db()
    fresh.NAME_FETCH_MIN = 0
    h = fresh.get_node_handle("M", "mammal-like")
    assert fresh.get_node_names([h]) == ["mammal-like"]
    other = {"M": ["zz", "mammal-like-2"], "Q": ["a", "b" * 70]}
    fresh.load_canonical(_canonical(other, [(("M", "zz"), ("Q", "a"))]))
    pairs = [(t, n) for t in other for n in other[t]]
    assert fresh.get_node_names([fresh.get_node_handle(*p) for p in pairs]) == [n for _, n in pairs]
    assert fresh.get_node_names([h], strict=False) == [None]
    assert fresh.get_all_nodes("N") == []
    assert fresh.name_fetch_stats["host"] == 0 and fresh._mirror is None


def test_load_metta_names():
    """The name's start inside its leaf differs on this loader; a name may end
    in a newline here."""
    from das_amd.database.hip_db import HipDB
    names = {"Concept": ["a\n", "a", "ma", "naïve b", "long name x", "y" * 100], "Vé": ["c", "b7", "é"]}
    text = "(: Concept Type)\n(: Vé Type)\n(: Inheritance Type)\n"
    text += "".join(f'(: "{n}" {t})\n' for t in names for n in names[t])
    flat = [n for t in names for n in names[t]]          # (this reader stores the terminals an expression mentions)
    text += "".join(f'(Inheritance "{a}" "{b}")\n' for a, b in zip(flat[0::2], flat[1::2]))
    text += f'(Inheritance "{flat[-1]}" "{flat[0]}")\n'
    db = HipDB(device=0)
    db.NAME_FETCH_MIN = 0
    db.load_metta(text)
    pairs = [(t, n) for t in names for n in names[t]]
    assert db.get_node_names([db.get_node_handle(*p) for p in pairs]) == [n for _, n in pairs]
    for t in names:
        assert sorted(db.get_all_nodes(t, names=True)) == sorted(names[t])
    assert db.name_fetch_stats["host"] == 0 and db._mirror is None
