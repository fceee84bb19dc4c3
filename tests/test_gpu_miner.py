"""The pattern miner's device path (das_halo_expand, das_pattern_counts,
miner.hip) against the per-call loops it replaces (miner.halo_host,
miner.pattern_counts_host) on the same HipDB, and against those loops over the
oracle: same links per level, same atoms, same templates, same counts.

One hand-built canonical KB, sized from the kernels' chunk sizes: a hub
component (one node in 4 workgroup passes + 104 incoming entries, a second
hub giving a (1,2)-grounded template whose shorter key range is more than one
wave chunk) and a small component with the edge cases (degrees 0, 1, 63, 64,
65; a link holding its seed twice; a nested link; arities 1 and 4; a
black-listed type; Similarity and Set)."""
import os

import numpy as np
import pytest

import bench
from das_amd import _lib, loader, miner
from das_amd.expression_hasher import ExpressionHasher as EH
from oracle import das_oracle as O

pytestmark = pytest.mark.gpu

W = "*"
N_HUB = 4 * _lib.HALO_BLOCK_ENTRIES + 104          # links through the hub H (> 4 workgroup passes)
N_G = _lib.PC_CHUNK_ROWS + 476                      # of them through the second hub G (> one wave chunk)
N_W = 20
BLACK = ["Blk"]


def C(name):
    return EH.terminal_hash("Concept", name)


def L(t, *targets):
    return EH.expression_hash(EH.named_type_hash(t), list(targets))


def _text():
    types = ["Concept", "Ex", "Inh", "Ev", "One", "Four", "Blk", "Similarity", "Set"]
    nodes = ["H", "G"] + [f"w{j}" for j in range(N_W)] + [f"k{i}" for i in range(N_HUB)]
    nodes += ["a", "b", "c", "d0", "d1", "d63", "d64", "d65", "p", "n2", "n3", "s1", "s2", "s3"]
    nodes += [f"y{j}" for j in range(65)]
    n = lambda x: f'"Concept {x}"'                                   # noqa: E731
    ex = [f"(Ex {n(f'k{i}')} {n('H')} {n('G' if i < N_G else f'w{i % N_W}')})" for i in range(N_HUB)]
    for d in (1, 63, 64, 65):
        ex += [f"(Inh {n(f'd{d}')} {n(f'y{j}')})" for j in range(d)]
    ex += [f"(Inh {n('a')} {n('a')})", f"(Ex {n('a')} {n('a')} {n('b')})", f"(Ex {n('b')} {n('a')} {n('a')})",
           f"(Inh {n('a')} {n('b')})", f"(Inh {n('b')} {n('c')})",
           f"(Ev {n('p')} (Inh {n('n2')} {n('n3')}))",
           f"(One {n('a')})", f"(Four {n('a')} {n('b')} {n('c')} {n('n3')})",
           f"(Blk {n('a')} {n('b')})", f"(Blk {n('b')} {n('c')})"]
    for x, y in (("s1", "s2"), ("s1", "s3"), ("a", "s1")):
        ex += [f"(Similarity {n(x)} {n(y)})", f"(Similarity {n(y)} {n(x)})"]
    ex += [f"(Set {n('s1')} {n('s2')} {n('s3')})", f"(Set {n('s3')} {n('a')} {n('s2')})",
           f"(Set {n('a')} {n('a')} {n('s1')})"]
    lines = [f"(: {t} Type)" for t in types] + [f'(: "{x}" Concept)' for x in nodes] + ex
    return "\n".join(lines) + "\n"


TEXT = _text()
INNER = L("Inh", C("n2"), C("n3"))
OUTER = L("Ev", C("p"), INNER)
SMALL_SEEDS = [C(x) for x in ("a", "d0", "d1", "d63", "d64", "d65", "p")] + [INNER]


def _fresh_db(text=TEXT, black=BLACK, **kw):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0, **kw)
    db.pattern_black_list = list(black)
    db.load_canonical(text)
    return db


@pytest.fixture(scope="module", params=["mirror", "no_mirror"])
def db(request):
    """The KB on the device, with the host mirror of the pattern keys (the
    default) and without it (DAS_HOST_KEY_MIRROR=0, read when the index is built)."""
    old = os.environ.get("DAS_HOST_KEY_MIRROR")
    if request.param == "no_mirror":
        os.environ["DAS_HOST_KEY_MIRROR"] = "0"
    try:
        return _fresh_db()
    finally:
        if old is None:
            os.environ.pop("DAS_HOST_KEY_MIRROR", None)
        else:
            os.environ["DAS_HOST_KEY_MIRROR"] = old


@pytest.fixture(scope="module")
def oracle():
    kb = O.KB.from_arrays(_lib.parse_canonical(TEXT))
    return bench.OracleFacade(O.RedisMongoSemantics(kb, pattern_black_list=BLACK))


@pytest.fixture(scope="module")
def oracle_halos(oracle):
    """The oracle's halos, computed once: small seeds at length 3, the hub at 2."""
    return {"small": miner.halo_host(oracle, SMALL_SEEDS, 3), "hub": miner.halo_host(oracle, [C("H")], 2)}


def _device(db, fn, *args):
    before = dict(db.miner_stats)
    out = fn(*args)
    assert db.miner_stats == {"device": before["device"] + 1, "host": before["host"]}
    return out


def _host(db, fn, *args):
    old = os.environ.get("DAS_MINER")
    os.environ["DAS_MINER"] = "0"
    before = dict(db.miner_stats)
    try:
        out = fn(*args)
    finally:
        if old is None:
            del os.environ["DAS_MINER"]
        else:
            os.environ["DAS_MINER"] = old
    assert db.miner_stats == {"device": before["device"], "host": before["host"] + 1}
    return out


def _same_halo(got, want, levels):
    assert len(got) == len(want) == levels
    for lv in range(levels):
        for g, w in ((got.links[lv], want.links[lv]), (got.atoms[lv], want.atoms[lv])):
            assert g.dtype == np.uint32 and np.array_equal(g, w), lv
            assert (np.diff(g.astype(np.int64)) > 0).all()


def _same_as_oracle(got, want, levels):
    for lv in range(levels):
        assert sorted(got.link_handles(lv)) == sorted(want.link_handles(lv)), lv
        assert sorted(got.atom_handles(lv)) == sorted(want.atom_handles(lv)), lv


def test_kb_has_the_shapes_the_kernels_split_on(db):
    ids = db.ids_of([C("H"), C("G"), C("d0"), C("d1"), C("d63"), C("d64"), C("d65")])
    deg = [len(db.ctx.incoming(int(i))) for i in ids]
    assert deg == [N_HUB, N_G, 0, 1, 63, 64, 65]
    assert deg[0] >= 4 * _lib.HALO_BLOCK_ENTRIES + 1 and deg[1] > _lib.PC_CHUNK_ROWS
    per_w = (N_HUB - N_G) // N_W
    assert N_HUB > 10 * (per_w + 1)                       # (1,2) template [Ex, *, H, w]: key ranges 10x apart


@pytest.mark.parametrize("length", [0, 1, 2, 3])
def test_halo_small_component(db, oracle_halos, length):
    """Degrees 0 / 1 / 63 / 64 / 65, a repeated seed, an unknown handle, a
    seed that is a link, a link holding the seed twice, arities 1 and 4 and
    the black-listed type never found."""
    seeds = SMALL_SEEDS + [C("a"), "0" * 32, C("nobody")]
    got = _device(db, db.halo, seeds, length)
    _same_halo(got, _host(db, db.halo, seeds, length), length)
    _same_as_oracle(got, oracle_halos["small"], length)
    assert got.universe_size == sum(len(oracle_halos["small"].links[lv]) for lv in range(length))
    if length:
        found = set(got.link_handles(0))
        assert {L("Inh", C("a"), C("a")), L("Ex", C("a"), C("a"), C("b")), OUTER,
                L("Set", C("a"), C("a"), C("s1"))} <= found
        everything = {h for lv in range(length) for h in got.link_handles(lv)}
        assert not everything & {L("One", C("a")), L("Four", C("a"), C("b"), C("c"), C("n3")),
                                 L("Blk", C("a"), C("b")), L("Blk", C("b"), C("c"))}
        assert len(everything) == got.universe_size            # a link is reported at one level only
        assert INNER not in got.atom_handles(0)                # a seed is not reached again


def test_halo_hub_and_word_boundaries(db, oracle, oracle_halos):
    """The hub's incoming list is split over workgroups; seeds picked so that
    atom ids sit on both sides of 32- and 64-bit bitmap word boundaries."""
    got = _device(db, db.halo, [C("H")], 1)
    _same_halo(got, _host(db, db.halo, [C("H")], 1), 1)
    assert len(got.links[0]) == N_HUB
    got2 = _device(db, db.halo, [C("H")], 2)
    _same_as_oracle(got2, oracle_halos["hub"], 2)
    ks = [C(f"k{i}") for i in range(N_HUB)]
    by_mod = {int(i) % 64: h for h, i in zip(ks, db.ids_of(ks))}
    seeds = [by_mod[m] for m in (31, 32, 63, 0)]
    got3 = _device(db, db.halo, seeds, 2)
    _same_as_oracle(got3, miner.halo_host(oracle, seeds, 2), 2)
    assert [len(x) for x in got3.links] == [4, N_HUB - 4]
    link_mods = {int(i) % 64 for i in got3.links[1]}
    assert {31, 32, 63, 0} <= link_mods


def test_halo_empty_seeds(db):
    for seeds in ([], ["0" * 32]):
        got = _device(db, db.halo, seeds, 2)
        assert [len(x) for x in got.links] == [0, 0] and [len(x) for x in got.atoms] == [0, 0]
        assert got.universe_size == 0 and got.link_handles(0) == []


def _same_counts(got, want):
    assert np.array_equal(got.arity, want.arity) and np.array_equal(got.type_id, want.type_id)
    assert np.array_equal(got.targets, want.targets)
    assert got.count.dtype == np.uint64 and np.array_equal(got.count, want.count)
    assert [got.template(i) for i in range(len(got))] == [want.template(i) for i in range(len(want))]


@pytest.fixture(scope="module")
def sample_links():
    hub = [L("Ex", C(f"k{i}"), C("H"), C("G" if i < N_G else f"w{i % N_W}")) for i in range(0, N_HUB, 97)]
    return hub + [L("Inh", C("a"), C("a")), L("Ex", C("a"), C("a"), C("b")), L("Ex", C("b"), C("a"), C("a")),
                  L("Inh", C("d65"), C("y3")), OUTER, INNER, L("One", C("a")),
                  L("Four", C("a"), C("b"), C("c"), C("n3")), L("Blk", C("a"), C("b")),
                  L("Similarity", C("s1"), C("s2")), L("Similarity", C("s2"), C("s1")),
                  L("Similarity", C("a"), C("s1")), L("Set", C("s1"), C("s2"), C("s3")),
                  L("Set", C("s3"), C("a"), C("s2")), L("Set", C("a"), C("a"), C("s1"))]


def test_pattern_counts_match_the_per_call_loop(db, oracle, sample_links):
    from das_amd.distributed_atom_space import DistributedAtomSpace
    got = _device(db, db.pattern_counts, sample_links)
    _same_counts(got, _host(db, db.pattern_counts, sample_links))
    assert got.as_dict() == miner.pattern_counts_host(oracle, sample_links).as_dict()
    das = DistributedAtomSpace(db=db)
    tpl = [got.template(i) for i in range(len(got))]
    for i, t in enumerate(tpl):
        assert int(got.count[i]) == len(das.get_links(t[0], None, t[1:])), t
    d = got.as_dict()
    key = lambda *t: EH.composite_hash(list(t))                         # noqa: E731
    # the long key range is chunked over waves; the shorter of two ranges 30x apart is the one scanned
    assert d[key("Ex", W, C("H"), C("G"))] == N_G
    assert d[key("Ex", W, C("H"), C("w3"))] == len([i for i in range(N_G, N_HUB) if i % N_W == 3])
    assert d[key("Ex", W, C("H"), W)] == N_HUB
    assert d[key("Ex", C("a"), C("a"), W)] == 1 and d[key("Inh", C("a"), W)] == 2
    # a black-listed type counts 0; a template over a link target is dropped; arities 1 and 4 give none
    assert d[key("Blk", W, C("b"))] == 0 and d[key("Blk", C("a"), W)] == 0
    assert key("Ev", W, INNER) not in d and d[key("Ev", C("p"), W)] == 1
    assert not any(t[0] in ("One", "Four") for t in tpl)
    # Similarity / Set: two templates as written, each under the sorted key
    assert d[key("Similarity", W, C("s1"))] == d[key("Similarity", C("s1"), W)] == 3
    lo, hi = sorted([C("s3"), C("s2")])
    assert d[key("Set", C("s3"), W, C("s2"))] == len(oracle.db.patterns.get((O.named_type_hash("Set"), W, lo, hi), ()))
    # ordered by (arity, type, targets), no template twice
    rows = [(int(got.arity[i]), int(got.type_id[i]), *map(int, got.targets[i])) for i in range(len(got))]
    assert rows == sorted(set(rows))


def test_pattern_counts_inputs(db, oracle, oracle_halos, sample_links):
    assert len(_device(db, db.pattern_counts, [])) == 0
    base = _device(db, db.pattern_counts, sample_links)
    _same_counts(_device(db, db.pattern_counts, sample_links + sample_links[::-1] + sample_links[:5]), base)
    _same_counts(_device(db, db.pattern_counts, np.asarray(db.ids_of(sample_links), dtype=np.uint32)), base)
    # a whole halo level, read on the device: no host copy of its ids is made
    halo = _device(db, db.halo, [C("H")], 2)
    for lv in range(2):
        got = _device(db, db.pattern_counts, halo.level(lv))
        assert halo.links._host[lv] is None
        assert got.as_dict() == miner.pattern_counts_host(oracle, oracle_halos["hub"].link_handles(lv)).as_dict()
    with pytest.raises(ValueError):
        db.pattern_counts(["0" * 32])


def test_stale_pattern_keys_take_the_host_path():
    db = _fresh_db(stale_pattern_keys=True)
    assert db._stale
    halo = db.halo(SMALL_SEEDS, 2)
    pc = db.pattern_counts(halo.level(0))
    assert db.miner_stats == {"device": 0, "host": 2}
    want = miner.halo_host(db, SMALL_SEEDS, 2)
    assert all(np.array_equal(halo.links[lv], want.links[lv]) for lv in range(2))
    assert pc.as_dict() == miner.pattern_counts_host(db, want.link_handles(0)).as_dict()


def test_rebuild_starts_from_the_new_kb():
    db = _fresh_db()
    first = db.halo([C("a")], 2)
    assert first.universe_size > 0
    text = "\n".join(["(: Concept Type)", "(: Inh Type)"] + [f'(: "z{i}" Concept)' for i in range(70)] +
                     [f'(Inh "Concept z{i}" "Concept z{i + 1}")' for i in range(69)] +
                     ['(Inh "Concept z0" "Concept z69")']) + "\n"
    db.pattern_black_list = []
    db.load_canonical(text)
    oracle = bench.OracleFacade(O.RedisMongoSemantics(O.KB.from_arrays(_lib.parse_canonical(text))))
    seeds = [C("z0"), C("a")]                               # `a` is gone with the old KB
    got = db.halo(seeds, 3)
    _same_as_oracle(got, miner.halo_host(oracle, seeds, 3), 3)
    assert [len(x) for x in got.links] == [2, 2, 2] and got.universe_size == 6
    assert db.pattern_counts(got.level(1)).as_dict() == \
        miner.pattern_counts_host(oracle, got.link_handles(1)).as_dict()
    assert db.miner_stats["host"] == 0


def test_raw_abi_validates_before_any_launch(db):
    n_atoms = int(db.ctx.stats().n_atoms)
    fresh = _lib.Context(0)
    launches = _lib.counters()[0]
    with pytest.raises(ValueError):
        db.ctx.halo_expand([0], _lib.HALO_MAX_LEVELS + 1)
    with pytest.raises(ValueError):
        db.ctx.halo_expand([0, n_atoms], 2)
    with pytest.raises(ValueError):
        db.ctx.pattern_counts(np.array([n_atoms], dtype=np.uint32))
    for call in (lambda: fresh.halo_expand([0], 1), lambda: fresh.pattern_counts(np.array([0], dtype=np.uint32))):
        with pytest.raises(_lib.DasNativeError) as e:
            call()
        assert e.value.code == _lib.ERR_NOT_BUILT
    assert _lib.counters()[0] == launches
    links, atoms = db.ctx.halo_expand([int(db.ids_of([C("a")])[0])], _lib.HALO_MAX_LEVELS)
    assert len(links) == len(atoms) == _lib.HALO_MAX_LEVELS and links[0].nrows > 0
    assert links[0].kind == _lib.TABLE_ORDERED and len(links[0].vars) == 1


def test_sharded_index_is_unsupported():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(_lib.parse_canonical(TEXT), shard=(0, 2))
    launches = _lib.counters()[0]
    with pytest.raises(NotImplementedError):
        db.ctx.halo_expand([0], 1)
    with pytest.raises(NotImplementedError):
        db.ctx.pattern_counts(np.array([0], dtype=np.uint32))
    assert _lib.counters()[0] == launches


def test_facade_notebook_flow_on_animals(golden):
    """get_matched_node_name -> halo -> pattern_counts -> And of two patterns
    through query, every count equal to the oracle's."""
    from das_amd.distributed_atom_space import DistributedAtomSpace
    from das_amd.pattern_matcher.pattern_matcher import And, PatternMatchingAnswer
    d = golden("kb_animals.json")
    das = DistributedAtomSpace()
    das.db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    odb = O.RedisMongoSemantics(O.KB.from_tables(d["nodes"], d["links"]))
    oracle = bench.OracleFacade(odb)
    seeds = das.db.get_matched_node_name("Concept", "ma")
    assert {"human", "mammal"} <= {das.get_node_name(h) for h in seeds}
    halo = das.halo(seeds)
    want = miner.halo_host(oracle, seeds, 2)
    _same_as_oracle(halo, want, 2)
    assert halo.universe_size == want.universe_size > 0
    pc = das.pattern_counts(halo.level(0))
    assert pc.as_dict() == miner.pattern_counts_host(oracle, want.link_handles(0)).as_dict()
    assert das.pattern_counts(halo.link_handles(1)).as_dict() == \
        miner.pattern_counts_host(oracle, want.link_handles(1)).as_dict()
    assert das.db.miner_stats == {"device": 3, "host": 0}
    tpl = [pc.template(i) for i in range(len(pc))]
    i, j = [k for k, t in enumerate(tpl) if t[0] == "Inheritance" and t[1] == W and int(pc.count[k]) > 1][:2]
    expr = And([pc.pattern(i), pc.pattern(j)])
    ans = PatternMatchingAnswer()
    matched = expr.matched(das.db, ans)
    spec = ["And", [["Link", "Inheritance", True, [["Var", "V1"], ["Node", "Concept", das.get_node_name(t[2])]]]
                    for t in (tpl[i], tpl[j])]]
    rows = O.evaluate(spec, odb)["rows"]
    assert (len(ans.assignments) if matched else 0) == len(rows)
    assert isinstance(das.query(expr), str)
