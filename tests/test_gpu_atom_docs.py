"""Atom documents of many atoms in one device call (das_atoms_json,
das_links_outgoing; docs.hip): HipDB.atoms_json / get_atoms_as_dicts and the
ATOM_INFO / JSON outputs of DistributedAtomSpace against the per-atom host
walk on the same HipDB (atoms_json_host, get_atoms_as_dicts_host: the parent
commit's code).  Every comparison asserts which path answered.

The host walk costs two device round trips per visited atom, so an atom's
deep representation is asked of it once (`Ref`) and the expected text of a
list is json.dumps over those; whole-call comparisons with atoms_json_host
stand beside them."""
import json
import os

import numpy as np
import pytest

from das_amd import _lib, loader, synthetic
from das_amd.distributed_atom_space import DistributedAtomSpace, QueryOutputFormat
from das_amd.expression_hasher import ExpressionHasher as EH

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ATOM_INFO, JSON, HANDLE = QueryOutputFormat.ATOM_INFO, QueryOutputFormat.JSON, QueryOutputFormat.HANDLE
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]
E2, E3, E4 = "é", "€", "\U0001f600"            # 2-, 3- and 4-byte sequences
ESCAPES = ['q"uote', "back\\slash", "nl\nx", "cr\rx", "tab\tx", "bs\bx", "ff\fx", "one\x01", "us\x1f", "del\x7f",
           "nul\x00in", "sl/ash", E2 + "a", "a" + E2, E3 + "a", "a" + E3, E4 + "a", "a" + E4, E2 + E3 + E4,
           E4 + E3 + E2, E2, E3, E4, E4 + E4]
QUOTED_TYPE = 'Q"uo\\te'                                 # the builder admits any type name: this one needs escaping
LENGTHS = range(71)
VARIANTS = 3
BIG = ("big" + 'ab"\\' + E2) * 7300                      # 65700 bytes of UTF-8 (> 64 KiB), escapes throughout
CHAIN = 17                                               # levels of the deepest chain: one more than the device renders


def _sized(length, variant):
    body = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_" * 2
    return (f"{variant}" + body[variant * 7:])[:length] if length else ""


class _KB:
    """An AtomBuilder that remembers every atom's handle."""

    def __init__(self):
        self.b = loader.AtomBuilder()

    def node(self, type_, name):
        return self.b.terminal(type_, name, node=True), EH.terminal_hash(type_, name)

    def link(self, type_, kids):
        return (self.b.expr(type_, [r for r, _ in kids]),
                EH.expression_hash(EH.named_type_hash(type_), [h for _, h in kids]))


def _build():
    kb = _KB()
    out = {}
    sized = {(n, v): kb.node("Sized", _sized(n, v)) for n in LENGTHS for v in range(VARIANTS if n else 1)}
    out["sized"] = {k: h for k, (_, h) in sized.items()}
    pads = [kb.node("Pad", "-" * k) for k in range(16)]
    out["pads"] = [h for _, h in pads]
    esc = [kb.node("Concept", n) for n in ESCAPES]
    out["escapes"] = [h for _, h in esc]
    out["big"] = kb.node("Concept", BIG)[1]
    out["quoted"] = kb.node(QUOTED_TYPE, "n")[1]
    plain = [kb.node("Concept", f"c{k}") for k in range(300)]
    out["nodes"] = [h for _, h in plain]
    shared = kb.link("Similarity", [plain[0], esc[0]])
    out["shared"] = shared[1]
    out["links"] = [kb.link("Inheritance", [plain[k], shared])[1] for k in range(1, 260)]
    out["arity"] = {a: kb.link("List", plain[10:10 + a])[1] for a in (1, 2, 3, 8)}
    out["quoted_link"] = kb.link(QUOTED_TYPE, [plain[1], plain[2]])[1]
    chain = [plain[5]]
    for k in range(1, CHAIN):
        chain.append(kb.link("Nest", [plain[k], chain[-1]]))
    out["chain"] = [h for _, h in chain]             # chain[k] has k + 1 levels
    ghost = (kb.b.terminal("Concept", "ghost", node=False), EH.terminal_hash("Concept", "ghost"))
    out["ghost"] = ghost[1]
    out["ghost_link"] = kb.link("Inheritance", [plain[3], ghost])[1]
    return kb.b.finish(), out


def _new_db():
    """A HipDB whose document calls are all meant for the device, whatever
    the measured thresholds are."""
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.ATOM_DOCS_MIN = db.ATOM_DOCS_MIN_PREFETCHED = db.ATOM_DOCS_MIN_NODES = 0
    return db


class Ref:
    """The host walk's deep representation of each handle, asked once."""

    def __init__(self, db):
        self.db, self.docs = db, {}

    def __call__(self, h):
        if h not in self.docs:
            self.docs[h] = self.db.get_atom_as_deep_representation(h)
        return self.docs[h]

    def text(self, handles, as_list=True):
        docs = [self(h) for h in handles]
        return json.dumps(docs if as_list else docs[0], sort_keys=False, indent=4)


@pytest.fixture(scope="module")
def kb():
    arrays, h = _build()
    db = _new_db()
    db.load_arrays(arrays)
    return db, h, Ref(db)


def _device(db, handles, as_list=True):
    """atoms_json, answered by the device."""
    before = dict(db.atom_docs_stats)
    text = db.atoms_json(handles, as_list=as_list)
    assert db.atom_docs_stats == {"device": before["device"] + 1, "host": before["host"]}
    return text


def _same(got, want):
    if got != want:                                  # (no megabyte-long assertion message)
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"texts differ at {k} of {len(want)} ({len(got)} got): "
                             f"{got[max(k - 40, 0):k + 40]!r} != {want[max(k - 40, 0):k + 40]!r}")


def test_first_call_builds_the_heap_and_matches_the_host_walk():
    """First in the file: a fresh DB's first document call builds the name heap."""
    b = _KB()
    n1, n2 = b.node("Concept", "human"), b.node("Concept", 'mon"key')
    link = b.link("Similarity", [n1, n2])
    db = _new_db()
    db.load_arrays(b.b.finish())
    handles = [link[1], n1[1], link[1]]
    want = json.dumps([{"type": "Similarity", "targets": [{"type": "Concept", "name": "human"},
                                                          {"type": "Concept", "name": 'mon"key'}]},
                       {"type": "Concept", "name": "human"}], sort_keys=False, indent=4)
    _same(_device(db, handles[:2]), want)
    _same(_device(db, handles), db.atoms_json_host(handles))
    assert db.atom_docs_stats == {"device": 2, "host": 0}


@pytest.mark.parametrize("n", COUNTS)
def test_root_counts(kb, n):
    db, h, ref = kb
    mixed = [x for pair in zip(h["nodes"], h["links"]) for x in pair]
    for roots in (h["nodes"][:n], h["links"][:n], mixed[:n]):
        _same(_device(db, roots), ref.text(roots))
    if n in (0, 1, 65):
        roots = mixed[:n]
        _same(_device(db, roots), db.atoms_json_host(roots))


def test_repeated_roots_and_shared_sub_link(kb):
    db, h, ref = kb
    roots = [h["links"][0], h["shared"], h["links"][0], h["nodes"][0], h["links"][0]] + h["links"][:70] + \
        [h["shared"]] * 3
    _same(_device(db, roots), ref.text(roots))
    assert ref(h["links"][4])["targets"][1] == ref(h["shared"])


@pytest.mark.parametrize("levels", [1, 2, 3, 5, 16])
def test_nesting(kb, levels):
    db, h, ref = kb
    assert levels <= _lib.DOC_MAX_DEPTH
    root = h["chain"][levels - 1]
    _same(_device(db, [root], as_list=False), ref.text([root], as_list=False))
    roots = [root, h["nodes"][0], h["chain"][0], root]
    _same(_device(db, roots), ref.text(roots))


def test_nesting_beyond_the_limit_takes_the_host_walk(kb):
    db, h, ref = kb
    root = h["chain"][_lib.DOC_MAX_DEPTH]               # one level more than the device renders
    tj, toff = db._type_json_texts()
    assert db.ctx.atoms_json(tj, toff, ids=db.ids_of([root]).astype(np.uint32)) is None       # DAS_ERR_LIMIT
    before = dict(db.atom_docs_stats)
    text = db.atoms_json([h["nodes"][0], root])
    assert db.atom_docs_stats == {"device": before["device"], "host": before["host"] + 1}
    _same(text, ref.text([h["nodes"][0], root]))
    depth, doc = 1, ref(root)
    while "targets" in doc:
        depth, doc = depth + 1, doc["targets"][1]
    assert depth == _lib.DOC_MAX_DEPTH + 1


@pytest.mark.parametrize("arity", [1, 2, 3, 8])
def test_arities(kb, arity):
    db, h, ref = kb
    root = h["arity"][arity]
    assert len(ref(root)["targets"]) == arity
    _same(_device(db, [root], as_list=False), ref.text([root], as_list=False))
    _same(_device(db, [root, root]), ref.text([root, root]))


def test_arity_beyond_the_row_tables_is_refused_at_load():
    """Arity 9 is beyond the index's row tables (kMaxArity = 8): the index
    build refuses such a KB (DAS_ERR_UNSUPPORTED), so no loader admits a link
    of arity 9 and the device never meets one.  The layout of arity 9 is
    pinned by the size rule's restatement in tests/test_atom_docs.py."""
    from das_amd.database.hip_db import HipDB
    b = _KB()
    b.link("List", [b.node("Concept", f"c{k}") for k in range(9)])
    with pytest.raises(NotImplementedError):
        HipDB(device=0).load_arrays(b.b.finish())


def test_every_length_behind_every_pad(kb):
    """Names of every length 0..70: behind a pad node whose name is 0..15
    bytes long, each name's text begins at every offset mod 16 of the output;
    where the names lie in the heap (ascending id, back to back) follows from
    the ids, and every source alignment mod 16 occurs among them."""
    db, h, ref = kb
    keys = list(h["sized"])
    roots = [h["sized"][k] for k in keys]
    for (n, v), hd in h["sized"].items():
        assert len(ref(hd)["name"]) == n
    for pad in range(16):
        _same(_device(db, [h["pads"][pad]] + roots), ref.text([h["pads"][pad]] + roots))
    ids = db.ids_of(roots)
    at, src = 0, set()
    for i in np.argsort(ids).tolist():
        src.add(at % 16)
        at += keys[i][0]
    assert src == set(range(16))


def test_escapes_and_multibyte_names(kb):
    db, h, ref = kb
    assert [ref(x)["name"] for x in h["escapes"]] == ESCAPES
    _same(_device(db, h["escapes"]), ref.text(h["escapes"]))
    for x in h["escapes"][:4]:
        _same(_device(db, [x], as_list=False), ref.text([x], as_list=False))
    # a type whose name needs escaping, on a node and on a link
    roots = [h["quoted"], h["quoted_link"]]
    assert ref(h["quoted"])["type"] == QUOTED_TYPE
    _same(_device(db, roots), ref.text(roots))


def test_a_name_of_64_kib(kb):
    db, h, ref = kb
    assert len(BIG.encode()) > 64 * 1024 and ref(h["big"])["name"] == BIG
    roots = [h["nodes"][0], h["big"], h["links"][0], h["big"]]
    _same(_device(db, roots), ref.text(roots))


def test_cap_below_equal_and_zero(kb):
    db, h, ref = kb
    roots = h["links"][:5] + h["escapes"][:5]
    want = ref.text(roots).encode("ascii")
    ids = db.ids_of(roots).astype(np.uint32)
    tj, toff = db._type_json_texts()
    for cap in (0, 1, 2, 3, 17, len(want) // 2, len(want) - 1, len(want)):
        out = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
        data, total, other, bad = db.ctx.atoms_json(tj, toff, ids=ids, cap=cap, out=out)
        assert (total, other, bad) == (len(want), 0, 0)
        assert data.tobytes() == want[:cap] and out[:cap].tobytes() == want[:cap]
        assert (out[cap:] == 0xA5).all()
    one = db.ids_of(roots[:1]).astype(np.uint32)
    want1 = ref.text(roots[:1], as_list=False).encode("ascii")
    for cap in (0, 5, len(want1)):
        out = np.full(len(want1) + 64, 0xA5, dtype=np.uint8)
        data, total, _, _ = db.ctx.atoms_json(tj, toff, ids=one, as_list=False, cap=cap, out=out)
        assert total == len(want1) and data.tobytes() == want1[:cap] and (out[cap:] == 0xA5).all()
    with pytest.raises(ValueError):                      # as_list = 0 renders one root
        db.ctx.atoms_json(tj, toff, ids=ids, as_list=False)


def test_entries_that_are_no_atom(kb):
    db, h, ref = kb
    tj, toff = db._type_json_texts()
    n_atoms = int(db.ctx.stats().n_atoms)
    good = db.ids_of(h["nodes"][:2]).astype(np.uint32)
    ids = np.array([good[0], n_atoms, _lib.DAS_NONE, good[1]], dtype=np.uint32)
    assert db.ctx.atoms_json(tj, toff, ids=ids)[2] == 2
    # a category-0 atom, as a root and as a link's target
    gid = db.ids_of([h["ghost"]])
    assert gid[0] >= 0 and db._lookup(h["ghost"])[1] == 0
    assert db.ctx.atoms_json(tj, toff, ids=gid.astype(np.uint32))[2] == 1
    assert db.ctx.atoms_json(tj, toff, ids=db.ids_of([h["ghost_link"]]).astype(np.uint32))[2] == 1
    das = DistributedAtomSpace(db=db)
    for roots in ([h["ghost_link"]], [h["nodes"][0], h["ghost"]]):
        before = dict(db.atom_docs_stats)
        _same(das.get_atoms(roots, JSON), db.atoms_json_host(roots))
        assert db.atom_docs_stats == {"device": before["device"], "host": before["host"] + 1}
    roots = [h["nodes"][0], h["ghost"], h["links"][0]]
    infos = das.get_atoms(roots, ATOM_INFO)
    assert infos == db.get_atoms_as_dicts_host(roots) and infos[1] == {}
    assert das.get_atom(h["ghost"], ATOM_INFO) == {} == db.get_atom_as_dict(h["ghost"])
    # a handle the KB does not hold: the host's exception, the first in input order
    absent = ["0" * 32, "f" * 32, "not a handle"]
    for roots in ([h["nodes"][0], absent[1], absent[0]], [absent[2]], [None]):
        with pytest.raises(ValueError) as host:
            db.atoms_json_host(roots)
        with pytest.raises(ValueError) as dev:
            das.get_atoms(roots, JSON)
        assert str(dev.value) == str(host.value) and "Invalid handle" in str(dev.value)
        assert db.get_atoms_as_dicts(roots) == db.get_atoms_as_dicts_host(roots)
    with pytest.raises(ValueError) as dev:
        das.get_atom(absent[0], JSON)
    assert str(dev.value) == f"Invalid handle: {absent[0]}"


def test_table_column_input(kb):
    db, h, ref = kb
    roots = h["links"][:9] + h["nodes"][:4]
    ids = db.ids_of(roots).astype(np.uint32)
    t = db.ctx.table_from_host(_lib.TABLE_ORDERED, [1, 2], np.stack([ids[::-1], ids]))
    tj, toff = db._type_json_texts()
    assert db.ctx.atoms_json(tj, toff, table=t, col=1)[0].tobytes().decode() == ref.text(roots)
    assert db.ctx.atoms_json(tj, toff, table=t, col=0)[0].tobytes().decode() == ref.text(roots[::-1])
    for row0, nrows in ((0, 1), (2, 5), (len(roots) - 1, 1), (len(roots), 0), (3, None)):
        got = db.ctx.atoms_json(tj, toff, table=t, col=1, row0=row0, nrows=nrows)[0].tobytes().decode()
        assert got == ref.text(roots[row0:] if nrows is None else roots[row0:row0 + nrows])
    assert db.ctx.atoms_json(tj, toff, table=t, col=1, row0=4, nrows=1, as_list=False)[0].tobytes().decode() == \
        ref.text(roots[4:5], as_list=False)
    with pytest.raises(ValueError):
        db.ctx.atoms_json(tj, toff, table=t, col=1, row0=1, nrows=len(roots))
    with pytest.raises(ValueError):
        db.ctx.atoms_json(tj, toff, table=t, col=2)
    # das_links_outgoing over the same column and over host ids
    off, tg, ctype, kind = db.ctx.links_outgoing(table=t, col=1)
    off2, tg2, ctype2, kind2 = db.ctx.links_outgoing(ids=ids)
    assert off.tolist() == off2.tolist() == [2 * k for k in range(10)] + [18] * 4
    assert tg.tolist() == tg2.tolist() and ctype.tolist() == ctype2.tolist() and kind.tolist() == kind2.tolist()
    assert kind.tolist() == [2] * 9 + [1] * 4 and (ctype[9:] == _lib.DAS_NONE).all() and len(set(ctype[:9])) == 1
    assert db.hex_of(tg[:2]) == db.get_link_targets(roots[0])
    off3, tg3, _, kind3 = db.ctx.links_outgoing(ids=np.array([ids[0], _lib.DAS_NONE, ids[1]], dtype=np.uint32), cap=3)
    assert off3.tolist() == [0, 2, 2, 4] and tg3.tolist() == tg[:3].tolist() and kind3.tolist() == [2, 0, 2]


# ------------------------------------------------------------------ the facade
def _animals():
    db = _new_db()
    with open(os.path.join(HERE, "golden", "data", "animals.metta")) as f:
        db.load_metta(f.read())
    return db


def _flybase():
    db = _new_db()
    db.load_arrays(synthetic.flybase_kb(n_genes=40, n_schema=6, rows_per_schema=60, n_loc=7, n_do=5))
    return db


def _facade_calls(das, kind):
    if kind == "animals":
        human, monkey = das.get_node("Concept", "human"), das.get_node("Concept", "monkey")
        return [
            ("get_links typed", lambda f: das.get_links("Inheritance", output_format=f)),
            ("get_links template", lambda f: das.get_links("Similarity", target_types=["Concept", "Concept"],
                                                           output_format=f)),
            ("get_links targets", lambda f: das.get_links("Inheritance", targets=[human, "*"], output_format=f)),
            ("get_links wildcard", lambda f: das.get_links("*", targets=["*", human], output_format=f)),
            ("get_nodes", lambda f: das.get_nodes("Concept", output_format=f)),
            ("get_nodes named", lambda f: das.get_nodes("Concept", "human", output_format=f)),
            ("get_atom", lambda f: das.get_atom(human, output_format=f)),
            ("get_node", lambda f: das.get_node("Concept", "monkey", output_format=f)),
            ("get_link", lambda f: das.get_link("Similarity", [human, monkey], output_format=f)),
            ("get_atoms", lambda f: das.get_atoms([human, das.get_link("Similarity", [human, monkey]), monkey, human],
                                                  output_format=f)),
        ]
    schema = das.get_node("Schema", "Schema:gene_uniquename")
    gene, fb = das.get_node("gene", "g3"), das.get_node("Verbatim", "FBgn0000003")
    return [
        ("get_links typed", lambda f: das.get_links("Execution", output_format=f)),
        ("get_links template", lambda f: das.get_links("Execution", target_types=["Schema", "gene", "Verbatim"],
                                                       output_format=f)),
        ("get_links targets", lambda f: das.get_links("Execution", targets=[schema, "*", "*"], output_format=f)),
        ("get_links wildcard", lambda f: das.get_links("*", targets=["*", fb, "*"], output_format=f)),
        ("get_nodes", lambda f: das.get_nodes("Schema", output_format=f)),
        ("get_atom", lambda f: das.get_atom(fb, output_format=f)),
        ("get_node", lambda f: das.get_node("gene", "g3", output_format=f)),
        ("get_link", lambda f: das.get_link("Execution", [schema, gene, fb], output_format=f)),
        ("get_atoms", lambda f: das.get_atoms([fb, das.get_link("Execution", [schema, gene, fb]), gene],
                                              output_format=f)),
    ]


@pytest.mark.parametrize("kind", ["animals", "flybase"])
def test_facade_json_and_atom_info(kind, monkeypatch):
    db = _animals() if kind == "animals" else _flybase()
    das = DistributedAtomSpace(db=db)
    calls = _facade_calls(das, kind)
    device = {}
    for what, call in calls:
        for f in (JSON, ATOM_INFO):
            before = dict(db.atom_docs_stats)
            device[what, f] = call(f)
            assert db.atom_docs_stats == {"device": before["device"] + 1, "host": before["host"]}, what
    assert len(json.loads(device["get_links typed", JSON])) > 3 and len(device["get_links targets", ATOM_INFO]) > 0
    known = das.get_node(*(("Concept", "human") if kind == "animals" else ("gene", "g3")))
    assert das.get_atoms([known, "0" * 32, known]) == [known, "", known]
    # the same calls by the host walk: DAS_ATOM_DOCS=0 is the parent commit's code
    monkeypatch.setenv("DAS_ATOM_DOCS", "0")
    for what, call in calls:
        for f in (JSON, ATOM_INFO):
            before = dict(db.atom_docs_stats)
            host = call(f)
            assert db.atom_docs_stats == {"device": before["device"], "host": before["host"] + 1}, what
            if f == JSON:
                _same(device[what, f], host)
            else:
                assert device[what, f] == host, what


def test_atom_info_documents_own_their_lists(kb):
    db, h, ref = kb
    roots = h["links"][:3] + [h["nodes"][0], "0" * 32, h["links"][0], h["chain"][2]]
    before = dict(db.atom_docs_stats)
    docs = db.get_atoms_as_dicts(roots)
    assert db.atom_docs_stats == {"device": before["device"] + 1, "host": before["host"]}
    host = db.get_atoms_as_dicts_host(roots)
    assert docs == host and docs[4] == {} and list(docs[0]) == list(host[0]) and list(docs[3]) == list(host[3])
    assert docs[0]["template"] == ["Inheritance", "Concept", ["Similarity", "Concept", "Concept"]]
    docs[0]["template"].append("x")
    docs[0]["template"][2].append("y")
    docs[0]["targets"].append("z")
    assert docs[1:] == host[1:] and docs[5] == host[5] == host[0]
    assert db.get_atoms_as_dicts(roots) == host             # the per-load template cache is intact


def test_default_thresholds_send_a_lone_node_to_the_walk(kb):
    """As measured: one node is one round trip in the walk, so it
    stays there; one link, and two nodes, are the device's."""
    from das_amd.database.hip_db import HipDB
    shared, h, ref = kb
    db = HipDB(device=0)
    db.load_arrays(shared.arrays)
    node, link = h["nodes"][0], h["links"][0]
    for roots, path in (([node], "host"), ([link], "device"), ([node, node], "device"), ([node, link], "device")):
        before = dict(db.atom_docs_stats)
        _same(db.atoms_json(roots), ref.text(roots))
        assert db.get_atoms_as_dicts(roots) == shared.get_atoms_as_dicts_host(roots)
        other = "device" if path == "host" else "host"
        assert db.atom_docs_stats == {path: before[path] + 2, other: before[other]}, roots


def test_env_switch_and_reload(monkeypatch):
    db = _new_db()

    def load(tag):
        b = _KB()
        n1, n2 = b.node("Concept", "human"), b.node(tag, "x" + tag)
        link = b.link("Similarity" + tag, [n2, n1])
        db.load_arrays(b.b.finish())
        return [link[1], n2[1]], [{"type": "Similarity" + tag, "targets": [{"type": tag, "name": "x" + tag},
                                                                         {"type": "Concept", "name": "human"}]},
                                  {"type": tag, "name": "x" + tag}]

    roots, docs = load("One")
    _same(_device(db, roots), json.dumps(docs, sort_keys=False, indent=4))
    info = db.get_atoms_as_dicts(roots)
    assert info[0]["template"] == ["SimilarityOne", "One", "Concept"] and info == db.get_atoms_as_dicts_host(roots)
    monkeypatch.setenv("DAS_ATOM_DOCS", "0")
    before = dict(db.atom_docs_stats)
    _same(db.atoms_json(roots), json.dumps(docs, sort_keys=False, indent=4))
    assert db.get_atoms_as_dicts(roots) == info
    assert db.atom_docs_stats == {"device": before["device"], "host": before["host"] + 2}
    monkeypatch.delenv("DAS_ATOM_DOCS")
    # a reload: the type texts and the template cache are the new KB's
    roots, docs = load("LongerTypeName")
    _same(_device(db, roots), json.dumps(docs, sort_keys=False, indent=4))
    info = db.get_atoms_as_dicts(roots)
    assert info[0]["template"] == ["SimilarityLongerTypeName", "LongerTypeName", "Concept"]
    assert info == db.get_atoms_as_dicts_host(roots)
    with pytest.raises(ValueError):
        db.atoms_json(["0" * 32])
