"""Counts of And-combinations of mined templates on the device
(das_conjunction_counts, miner.hip) against plain Python sets over the test's
own link list -- each template's (V1[, V2]) tuples, intersected or semi-joined
-- and, on samples, against the per-query loop (miner.conjunction_counts_host)
on the same HipDB and against the oracle's And.

One hand-built canonical KB, sized from the kernel's chunk (C driver rows per
wave step) and the wave (64): one-variable terms over three chunks with a
ragged last one and of 0 / 1 / 63 / 64 / 65 rows, (1,2)-grounded templates
whose shorter key range is more than one chunk, two-variable hubs of more than
2C rows, an 8-row term against a hub, and V1 values owning 1 / 64 / 65 / 130
rows of a driven two-variable term."""
import itertools
import os

import numpy as np
import pytest

from das_amd import _lib, loader, miner
from das_amd.database.db_interface import UNORDERED_LINK_TYPES
from das_amd.expression_hasher import ExpressionHasher as EH
from oracle import das_oracle as O

pytestmark = pytest.mark.gpu

C = _lib.CJ_CHUNK_ROWS
N_A, N_B, B_OFF = 2 * C + 104, 2 * C + 37, 100
BLACK = ["Blk"]
ARITY = {"Inh": 2, "Blk": 2, "Ex": 3, "Ey": 3, "Ez": 3, "Similarity": 2, "Set": 3}


def H(name):
    return EH.terminal_hash("Concept", name)


def LH(link):
    return EH.expression_hash(EH.named_type_hash(link[0]), [H(n) for n in link[1:]])


def x(i):
    return f"x{i}"


def y(j):
    return f"y{j}"


def _links():
    ls = [("Inh", x(i), "A") for i in range(N_A)]
    ls += [("Inh", x(i), "B") for i in range(B_OFF, B_OFF + N_B)]
    for d in (1, 63, 64, 65):
        ls += [("Inh", x(3 * i), f"D{d}") for i in range(d)]
    ls += [("Inh", x(i), "E") for i in range(41)]
    ls += [("Inh", x(i), "E2") for i in range(150, 260)]
    ls += [("Blk", x(i), "A") for i in range(5)]
    # (1,2)-grounded templates: key ranges P 2C+500, P2 C+750, Q1 2C+1000, Q2 C+250
    ls += [("Ex", x(i), "P", "Q1") for i in range(C + 300)]
    ls += [("Ex", x(i), "P", "Q2") for i in range(C, 2 * C + 200)]
    ls += [("Ex", x(i), "P2", "Q1") for i in range(200, C + 900)]
    ls += [("Ex", x(i), "P2", "Q2") for i in range(50)]
    ls += [("Ey", x(i), "R", "Q1") for i in range(500, 2 * C + 600)]
    ls += [("Inh", x(i), "S8") for i in range(C - 4, C + 4)]
    # V1 values owning 130 / 1 / 64 / 65 rows of [Ez, *, *, Z]; [Ez, *, *, Z2] is the larger term
    ls += [("Ez", "h", y(j), "Z") for j in range(130)] + [("Ez", "g", y(0), "Z")]
    ls += [("Ez", "g2", y(j), "Z") for j in range(64)] + [("Ez", "g3", y(j), "Z") for j in range(65)]
    ls += [("Ez", "h", y(j), "Z2") for j in range(100, 400)] + [("Ez", "g", y(0), "Z2")]
    ls += [("Ez", "g2", y(j), "Z2") for j in range(10)] + [("Ez", "g3", y(j), "Z2") for j in range(1, 65, 2)]
    ls += [("Inh", n, "M") for n in ("h", "g", "g2", "g3", x(0))]
    ls += [("Ex", "a", "a", "b"), ("Ex", "a", "c", "d"), ("Ex", "c", "d", "b"), ("Ex", "b", "a", "a"),
           ("Inh", "a", "a"), ("Inh", "a", "b"), ("Inh", "c", "b")]
    for p, q in (("s1", "s2"), ("s1", "s3"), ("a", "s1")):
        ls += [("Similarity", p, q), ("Similarity", q, p)]
    ls += [("Set", "s1", "s2", "s3"), ("Set", "s3", "a", "s2")]
    return ls


LINKS = _links()
NODES = list(dict.fromkeys(n for link in LINKS for n in link[1:]))


def _text(links, nodes, types):
    q = lambda n: f'"Concept {n}"'                                      # noqa: E731
    lines = ["(: Concept Type)"] + [f"(: {t} Type)" for t in types] + [f'(: "{n}" Concept)' for n in nodes]
    lines += [f"({link[0]} {' '.join(q(n) for n in link[1:])})" for link in links]
    return "\n".join(lines) + "\n"


TEXT = _text(LINKS, NODES, list(ARITY))

# the link list by (type, position, node): the rows a grounded target selects
BY_KEY = {}
for _l in LINKS:
    for _p, _n in enumerate(_l[1:]):
        BY_KEY.setdefault((_l[0], _p, _n), []).append(_l)


def T(link_type, *targets):
    """A template: None = wildcard."""
    assert len(targets) == ARITY[link_type]
    return (link_type, *targets)


_TUPLES = {}


def tuples_of(tpl):
    """The template's answer as a set: V1 values, or (V1, V2) pairs, the
    variables in wildcard order; a black-listed type has no pattern keys."""
    if tpl not in _TUPLES:
        grounded = [(p, n) for p, n in enumerate(tpl[1:]) if n is not None]
        wild = [p for p, n in enumerate(tpl[1:]) if n is None]
        out = set()
        if tpl[0] not in BLACK:
            p0, n0 = min(grounded, key=lambda g: len(BY_KEY.get((tpl[0], *g), ())))
            for link in BY_KEY.get((tpl[0], p0, n0), ()):
                if all(link[1 + p] == n for p, n in grounded):
                    out.add(link[1 + wild[0]] if len(wild) == 1 else (link[1 + wild[0]], link[1 + wild[1]]))
        _TUPLES[tpl] = out
    return _TUPLES[tpl]


def expected(combo):
    """The size of the natural join of the templates' tuple sets on V1 / V2."""
    sets = [tuples_of(t) for t in combo]
    if not all(sets):
        return 0
    one = [s for t, s in zip(combo, sets) if t[1:].count(None) == 1]
    two = [s for t, s in zip(combo, sets) if t[1:].count(None) == 2]
    if not two:
        return len(set.intersection(*one))
    pairs = set.intersection(*two)
    return sum(1 for v1, _ in pairs if all(v1 in s for s in one))


def _fresh_db(text=TEXT, black=BLACK, **kw):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0, **kw)
    db.pattern_black_list = list(black)
    db.load_canonical(text)
    return db


class Env:
    """The KB on the device with the templates of every ordered link (and of
    the Similarity / Set ones) as one PatternCounts, addressed by template."""

    def __init__(self, db, links=LINKS, nodes=NODES):
        self.db = db
        self.pc = db.pattern_counts([LH(link) for link in links])
        ids = dict(zip(nodes, np.asarray(db.ids_of([H(n) for n in nodes])).tolist()))
        assert min(ids.values()) >= 0
        self.ids = ids
        pc = self.pc
        self.rows = {key: i for i, key in enumerate(zip(pc.arity.tolist(), pc.type_id.tolist(),
                                                        *(pc.targets[:, p].tolist() for p in range(3))))}

    def row(self, tpl):
        tg = [self.ids[n] if n is not None else _lib.DAS_NONE for n in tpl[1:]]
        return self.rows[(len(tg), self.db.type_id[tpl[0]], *(tg + [_lib.DAS_NONE] * (3 - len(tg))))]

    def combos(self, combos):
        return np.array([[self.row(t) for t in combo] for combo in combos], dtype=np.uint32)

    def device(self, rows):
        before = dict(self.db.conjunction_stats)
        launches, readbacks = _lib.counters()
        got = self.db.conjunction_counts(self.pc, rows)
        assert self.db.conjunction_stats == {"device": before["device"] + len(rows), "host": before["host"]}
        after = _lib.counters()
        # resolve, plan, the scan's kernels, count; one read-back
        assert after[1] - readbacks == 1 and 3 <= after[0] - launches <= 10
        assert got.dtype == np.uint64 and got.shape == (len(rows),)
        return got

    def check(self, combos, host=0, oracle=None):
        """Device counts of the combinations (tuples of templates) against the
        set computation (one call per k); `host` of each call's also against
        the per-query loop, all of them against the oracle if one is given."""
        want = [expected(c) for c in combos]
        for k in sorted({len(c) for c in combos}):
            sel = [i for i, c in enumerate(combos) if len(c) == k]
            rows = self.combos([combos[i] for i in sel])
            assert self.device(rows).tolist() == [want[i] for i in sel]
            if host:
                pick = np.linspace(0, len(sel) - 1, min(host, len(sel))).astype(np.int64)
                assert miner.conjunction_counts_host(self.db, self.pc, rows[pick]).tolist() == \
                    [want[sel[i]] for i in pick]
        if oracle is not None:
            for combo, w in zip(combos, want):
                assert oracle_count(oracle, combo) == w, combo
        return want


def oracle_spec(tpl):
    k = itertools.count(1)
    return ["Link", tpl[0], tpl[0] not in UNORDERED_LINK_TYPES,
            [["Var", f"V{next(k)}"] if n is None else ["Node", "Concept", n] for n in tpl[1:]]]


def nested_and(specs):
    """build_composite_pattern's fold.  (A flat And of three terms is another
    query: the reference's And starts over from the next term once its
    running join is empty, pattern_matcher.py:717-729.)"""
    expr = specs[0]
    for s in specs[1:]:
        expr = ["And", [expr, s]]
    return expr


def oracle_count(odb, combo):
    r = O.evaluate(nested_and([oracle_spec(t) for t in combo]), odb)
    return r["n"] if r["matched"] else 0


@pytest.fixture(scope="module")
def env():
    return Env(_fresh_db())


@pytest.fixture(scope="module")
def odb():
    return O.RedisMongoSemantics(O.KB.from_arrays(_lib.parse_canonical(TEXT)), pattern_black_list=BLACK)


A, B, E, E2, S8, M = (T("Inh", None, n) for n in ("A", "B", "E", "E2", "S8", "M"))
D = {d: T("Inh", None, f"D{d}") for d in (1, 63, 64, 65)}
BLK = T("Blk", None, "A")
PQ1, PQ2, P2Q1, P2Q2 = T("Ex", None, "P", "Q1"), T("Ex", None, "P", "Q2"), T("Ex", None, "P2", "Q1"), \
    T("Ex", None, "P2", "Q2")
HUB_P, HUB_R, HUB_Q2 = T("Ex", None, "P", None), T("Ey", None, "R", None), T("Ex", None, None, "Q2")
Z, Z2 = T("Ez", None, None, "Z"), T("Ez", None, None, "Z2")


def test_kb_has_the_shapes_the_kernel_splits_on(env):
    count = lambda t: int(env.pc.count[env.row(t)])                     # noqa: E731
    assert [count(t) for t in (A, B, BLK, D[1], D[63], D[64], D[65], S8)] == [N_A, N_B, 0, 1, 63, 64, 65, 8]
    assert N_B == 2 * C + 37 and N_A > N_B                              # the driver: three chunks, the last ragged
    key = lambda p, n: len(BY_KEY[("Ex", p, n)])                        # noqa: E731
    # both (1,2)-grounded templates of the overlapping pair scan a range above one chunk, with rows that fail
    assert C < key(1, "P2") < key(2, "Q1") and count(P2Q1) < key(1, "P2")
    assert C < key(1, "P") < key(2, "Q1") and count(PQ1) < key(1, "P")
    assert C < key(2, "Q2") < key(1, "P2") and key(2, "Q2") < key(1, "P")
    assert count(HUB_P) > 2 * C and count(HUB_R) > 2 * C
    assert count(Z2) > count(Z) > count(M)                              # Z is the driven two-variable term
    own = lambda n: sum(1 for v1, _ in tuples_of(Z) if v1 == n)         # noqa: E731
    assert [own(n) for n in ("h", "g", "g2", "g3")] == [130, 1, 64, 65]
    assert count(T("Similarity", None, "s1")) > 0


def test_long_one_variable_terms_over_three_chunks(env, odb):
    assert env.check([(A, B), (B, A)], host=2, oracle=odb) == [N_A - B_OFF] * 2


def test_small_one_variable_terms(env, odb):
    """0 (black-listed), 1, 63, 64 and 65 rows, each against a long and a short partner."""
    small = [BLK] + list(D.values())
    combos = [(s, p) for s in small for p in (A, E)] + [(p, s) for s in small for p in (A, E)]
    want = env.check(combos, host=len(combos), oracle=odb)
    assert want[:4] == [0, 0, 1, 1] and want[8:10] == [65, 14]


def test_two_filtered_terms(env, odb):
    """Both terms are (1,2)-grounded: a filtered range has to drive."""
    want = env.check([(PQ2, P2Q2), (PQ1, P2Q1), (P2Q1, PQ1), (PQ1, PQ2), (PQ1, P2Q1, PQ2)], host=5, oracle=odb)
    assert want == [0, C + 100, C + 100, 300, 300]


def test_filtered_term_is_probed(env, odb):
    """By a one-variable driver and by a two-variable one."""
    want = env.check([(E2, P2Q1), (D[65], PQ1), (HUB_Q2, P2Q1), (P2Q1, HUB_Q2)], host=4, oracle=odb)
    assert want == [60, 65, 900, 900]


def test_two_hubs_share_pairs(env):
    """Two two-variable terms of more than 2C rows: the smaller drives, several chunks."""
    assert env.check([(HUB_P, HUB_R), (HUB_R, HUB_P), (HUB_P, HUB_R, HUB_P)], host=3) == [C - 200] * 3


def test_small_term_drives_a_hub(env, odb):
    """8 rows against more than 2C: the width of each x's equal range is added."""
    assert env.check([(S8, HUB_P), (HUB_P, S8)], host=2, oracle=odb) == [12, 12]
    assert env.check([(D[1], HUB_P), (BLK, HUB_P), (S8, HUB_R)], host=3) == [1, 0, 8]


def test_sub_ranges_per_lane_and_by_the_wave(env, odb):
    """One-variable and two two-variable terms: the sub-ranges of h (130 rows)
    and g3 (65) are walked by the whole wave, those of g (1) and g2 (64) by
    their lanes."""
    combos = [(M, Z, Z2), (Z, M, Z2), (Z2, Z, M), (M, Z, Z2, Z)]
    assert env.check(combos, host=4, oracle=odb) == [30 + 1 + 10 + 32] * 4


def test_k4_mixes_the_template_kinds(env):
    combos = [(A, PQ1, HUB_P, HUB_R), (HUB_R, A, HUB_P, PQ1), (B, P2Q1, HUB_P, HUB_R), (E2, PQ1, P2Q1, HUB_P),
              (A, E, D[65], D[64]),
              (T("Ex", "a", None, "b"), T("Inh", "a", None), T("Ex", None, "a", "a"), T("Inh", None, "b"))]
    want = env.check(combos, host=len(combos))
    assert want[0] == want[1] == C - 200 and all(w > 0 for w in want[:5])


def test_variables_follow_the_wildcard_order(env, odb):
    """[Ex, a, *, *] binds (t1, t2), [Ex, *, *, b] binds (t0, t1); Ex(a, a, b)
    gives the second a row with V1 == V2."""
    first, second = T("Ex", "a", None, None), T("Ex", None, None, "b")
    assert tuples_of(first) == {("a", "b"), ("c", "d")} and tuples_of(second) == {("a", "a"), ("c", "d")}
    want = env.check([(first, second), (second, T("Inh", "a", None)), (second, T("Inh", None, "b")),
                      (T("Ex", "a", "a", None), T("Inh", "a", None)), (T("Ex", "a", None, "b"), T("Inh", "a", None)),
                      (T("Ex", None, "a", "a"), T("Inh", "a", None))], host=6, oracle=odb)
    assert want == [1, 1, 2, 1, 1, 1]


def test_a_template_twice_and_every_order(env):
    want = env.check([(B, B), (PQ1, PQ1), (HUB_P, HUB_P), (S8, HUB_P, S8), (Z, Z, M), (BLK, BLK)], host=6)
    assert want == [N_B, C + 300, 2 * C + 500, 12, 260, 0]
    trio = (E2, HUB_P, P2Q1)
    counts = env.check(list(itertools.permutations(trio)))
    assert len(counts) == 6 and len(set(counts)) == 1 and counts[0] > 0


def test_all_pairs_of_a_halo_level(env, odb):
    """More combinations than one block's waves own: chunk offsets span several blocks."""
    db = env.db
    halo = db.halo([H("a"), H("g"), H("g2")], 1)
    level = db.pattern_counts(halo.level(0))
    names = {H(n): n for n in NODES}
    tpls = [tuple([t[0]] + [None if v == "*" else names[v] for v in t[1:]]) for t in level.templates()
            if t[0] not in UNORDERED_LINK_TYPES]
    combos = list(itertools.combinations(tpls, 2))
    assert len(combos) >= 4096
    want = env.check(combos, host=40)
    assert sum(1 for w in want if w) > 100
    for i in np.linspace(0, len(combos) - 1, 50).astype(np.int64).tolist():
        assert oracle_count(odb, combos[i]) == want[i]


def test_unordered_templates_take_the_per_query_loop_inside_a_batch(env):
    db, pc = env.db, env.pc
    sim, st = T("Similarity", None, "s1"), T("Set", None, "s2", "s3")
    combos = [(A, B), (sim, T("Inh", "a", None)), (S8, HUB_P), (T("Inh", None, "a"), sim), (st, sim), (E, D[65])]
    rows = env.combos(combos)
    before = dict(db.conjunction_stats)
    got = db.conjunction_counts(pc, rows)
    assert db.conjunction_stats == {"device": before["device"] + 3, "host": before["host"] + 3}
    assert got.tolist() == miner.conjunction_counts_host(db, pc, rows).tolist()
    assert got[[0, 2, 5]].tolist() == [expected(combos[i]) for i in (0, 2, 5)]       # input order is kept
    # a list of tuples, through the facade
    from das_amd.distributed_atom_space import DistributedAtomSpace
    das = DistributedAtomSpace(db=db)
    assert das.conjunction_counts(pc, [tuple(r) for r in rows.tolist()]).tolist() == got.tolist()
    for bad in ([(0,)], [(0, 1, 2, 3, 4)], [(0, 1), (0, 1, 2)], [(0, -1)], [(0, len(pc))]):
        with pytest.raises(ValueError):
            db.conjunction_counts(pc, bad)


SMALL_LINKS = [("Inh", x(i), "A") for i in range(70)] + [("Inh", x(i), "B") for i in range(30, 90)] + \
    [("Ex", x(i), "P", "Q1") for i in range(20, 50)] + [("Ex", x(i), "P2", "Q1") for i in range(40, 45)] + \
    [("Ex", "a", "a", "b"), ("Ex", "c", "a", "a")]
SMALL_NODES = list(dict.fromkeys(n for link in SMALL_LINKS for n in link[1:]))
SMALL_TEXT = _text(SMALL_LINKS, SMALL_NODES, ["Inh", "Ex"])
STALE_TEXT = _text(SMALL_LINKS + [("Blk", "a", "b"), ("Blk", "c", "a")], SMALL_NODES, ["Inh", "Ex", "Blk"])
SMALL_COMBOS = [(A, B), (A, PQ1), (B, HUB_P), (HUB_P, A), (T("Ex", None, "a", None), T("Ex", None, "a", None)),
                (T("Ex", None, None, "Q1"), HUB_P)]
SMALL_WANT = [40, 30, 20, 30, 2, 0]


def _small_rows(env):
    return env.combos(SMALL_COMBOS)


def test_host_path_switches(env):
    """DAS_MINER=0, CONFIG['no_overload'] and stale pattern entries: the
    per-query loop answers and `conjunction_stats["device"]` stays."""
    from das_amd.pattern_matcher.pattern_matcher import CONFIG
    db, pc = env.db, env.pc
    rows = env.combos([(A, B), (S8, HUB_P), (T("Ex", "a", None, None), T("Ex", None, None, "b"))])
    want = [N_A - B_OFF, 12, 1]
    before = dict(db.conjunction_stats)
    old = os.environ.get("DAS_MINER")
    os.environ["DAS_MINER"] = "0"
    try:
        assert db.conjunction_counts(pc, rows).tolist() == want
    finally:
        if old is None:
            del os.environ["DAS_MINER"]
        else:
            os.environ["DAS_MINER"] = old
    assert db.conjunction_stats == {"device": before["device"], "host": before["host"] + 3}
    CONFIG["no_overload"] = True
    try:
        got = db.conjunction_counts(pc, rows)
        assert got.tolist() == miner.conjunction_counts_host(db, pc, rows).tolist()
    finally:
        CONFIG["no_overload"] = False
    assert db.conjunction_stats == {"device": before["device"], "host": before["host"] + 6}
    stale = Env(_fresh_db(STALE_TEXT, BLACK, stale_pattern_keys=True), SMALL_LINKS, SMALL_NODES)
    assert stale.db._stale
    rows = _small_rows(stale)
    assert stale.db.conjunction_counts(stale.pc, rows).tolist() == \
        miner.conjunction_counts_host(stale.db, stale.pc, rows).tolist()
    assert stale.db.conjunction_stats == {"device": 0, "host": len(rows)}


def test_rebuild_counts_the_new_kb():
    db = _fresh_db()
    first = Env(db)
    assert first.device(first.combos([(A, B)])).tolist() == [N_A - B_OFF]
    db.pattern_black_list = []
    db.load_canonical(SMALL_TEXT)
    second = Env(db, SMALL_LINKS, SMALL_NODES)
    assert second.device(_small_rows(second)).tolist() == SMALL_WANT
    assert db.conjunction_stats["host"] == 0


def test_raw_abi_validates_before_any_launch(env):
    db, pc = env.db, env.pc
    n_atoms, n_types = int(db.ctx.stats().n_atoms), int(db.ctx.stats().n_types)
    NONE = _lib.DAS_NONE
    used = [env.row(t) for t in (A, HUB_P, PQ1)]
    good = np.vstack([pc.arity[used], pc.type_id[used], pc.targets[used].T]).astype(np.uint32)
    pairs = np.array([[0, 1], [1, 2]], dtype=np.uint32)

    def with_row(ar, ty, t0, t1, t2):
        return np.hstack([good, np.array([[ar], [ty], [t0], [t1], [t2]], dtype=np.uint32)])

    ex, inh, a = db.type_id["Ex"], db.type_id["Inh"], env.ids["a"]
    fresh = _lib.Context(0)
    launches = _lib.counters()[0]
    invalid = [
        (good, np.array([[0], [1]], dtype=np.uint32)),                          # k = 1
        (good, np.array([[0, 1, 2, 0, 1]], dtype=np.uint32)),                   # k = 5
        (good, np.array([[0, 3]], dtype=np.uint32)),                            # index >= m
        (with_row(4, ex, a, NONE, NONE), pairs),                                # arity
        (with_row(1, inh, NONE, NONE, NONE), pairs),
        (with_row(3, ex, a, a, a), pairs),                                      # no wildcard
        (with_row(2, inh, NONE, NONE, NONE), pairs),                            # no grounded target
        (with_row(3, ex, NONE, NONE, NONE), pairs),
        (with_row(2, n_types, a, NONE, NONE), pairs),                           # type id
        (with_row(3, ex, n_atoms, NONE, NONE), pairs),                          # grounded id
    ]
    for tpl, combos in invalid:
        with pytest.raises(ValueError):
            db.ctx.conjunction_counts(tpl, combos)
    with pytest.raises(NotImplementedError):
        db.ctx.conjunction_counts(with_row(2, db.type_id["Similarity"], a, NONE, NONE), pairs)
    with pytest.raises(_lib.DasNativeError) as e:
        fresh.conjunction_counts(good, pairs)
    assert e.value.code == _lib.ERR_NOT_BUILT
    out = db.ctx.conjunction_counts(good, np.zeros((0, 3), dtype=np.uint32))   # n = 0
    assert out.shape == (0,) and out.dtype == np.uint64
    assert _lib.counters()[0] == launches
    assert db.ctx.conjunction_counts(good, pairs).tolist() == [expected((A, HUB_P)), expected((HUB_P, PQ1))]
    assert _lib.counters()[0] > launches


def test_sharded_index_is_unsupported():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(_lib.parse_canonical(SMALL_TEXT), shard=(0, 2))
    tpl = np.array([[2], [db.type_id["Inh"]], [_lib.DAS_NONE], [0], [_lib.DAS_NONE]], dtype=np.uint32)
    launches = _lib.counters()[0]
    with pytest.raises(NotImplementedError):
        db.ctx.conjunction_counts(tpl, np.array([[0, 0]], dtype=np.uint32))
    assert _lib.counters()[0] == launches


@pytest.fixture(scope="module")
def animals(golden):
    """kb_animals.json on the device and in the oracle, and the notebook's
    flow up to the templates: get_matched_node_name -> halo -> pattern_counts."""
    from das_amd.distributed_atom_space import DistributedAtomSpace
    d = golden("kb_animals.json")
    das = DistributedAtomSpace()
    das.db.load_arrays(loader.from_tables(d["nodes"], d["links"]).finish())
    odb = O.RedisMongoSemantics(O.KB.from_tables(d["nodes"], d["links"]))
    seeds = das.db.get_matched_node_name("Concept", "ma")
    halo = das.halo(seeds)
    assert halo.universe_size > 0
    pc = das.pattern_counts(np.concatenate([halo.links[0], halo.links[1]]))
    level0 = {tuple(t) for t in das.pattern_counts(halo.level(0)).templates()}
    tpl = [tuple(t) for t in pc.templates()]
    first = [i for i, t in enumerate(tpl) if t in level0]
    assert first and len(first) < len(tpl)

    def spec(i):
        t, k = tpl[i], itertools.count(1)
        return ["Link", t[0], t[0] not in UNORDERED_LINK_TYPES,
                [["Var", f"V{next(k)}"] if h == "*" else ["Node", das.get_node_type(h), das.get_node_name(h)]
                 for h in t[1:]]]

    cache = {}

    def compute_count(expr_of, idx):
        """The notebook's compute_count over the oracle: `expr_of` builds the
        query of the template rows idx (nested_and, or a flat And)."""
        key = (expr_of.__name__, tuple(idx))
        if key not in cache:
            r = O.evaluate(expr_of([spec(i) for i in idx]), odb)
            cache[key] = r["n"] if r["matched"] else 0
        return cache[key]

    return das, pc, tpl, first, halo.universe_size, compute_count


def flat_and(specs):
    """And([t0, t1, ...]) as compute_isurprisingness writes its sub-combinations."""
    return ["And", list(specs)]


def notebook_isurprisingness(count, terms, counts, universe_size, compute_count, normalized):
    """compute_isurprisingness of the notebook (cell 3fa7b2ec), line by line,
    `terms` being template rows and And([...]) the flat query."""
    def prob(c):
        return c / universe_size

    def cc(*pos):
        return compute_count(flat_and, [terms[p] for p in pos])
    n = len(terms)
    if n == 3:
        subset_probs = [
            prob(counts[0]) * prob(counts[1]) * prob(counts[2]),
            prob(cc(0, 1)) * prob(counts[2]),
            prob(cc(0, 2)) * prob(counts[1]),
            prob(cc(1, 2)) * prob(counts[0]),
        ]
    else:
        subset_probs = [
            prob(counts[0]) * prob(counts[1]) * prob(counts[2]) * prob(counts[3]),
            prob(cc(0, 1)) * prob(cc(2, 3)),
            prob(cc(0, 2)) * prob(cc(1, 3)),
            prob(cc(0, 3)) * prob(cc(1, 2)),
            prob(cc(0, 1, 2)) * prob(counts[3]),
            prob(cc(0, 1, 3)) * prob(counts[2]),
            prob(cc(0, 2, 3)) * prob(counts[1]),
            prob(cc(1, 2, 3)) * prob(counts[0]),
        ]
    p = prob(count)
    isurprisingness = max([p - max(subset_probs), min(subset_probs) - p])
    if normalized:
        return isurprisingness / p if count else float("nan")      # (the notebook divides by zero)
    return isurprisingness


@pytest.mark.parametrize("k", [3, 4])
def test_notebook_flow_on_animals(animals, k):
    """isurprisingness of k-combinations whose first term is a level-0
    template, 200 at the most: `.count` is the oracle's count of the nested
    And, `.value` the notebook's formula with every sub-combination counted
    by the oracle the way the notebook asks for it -- for k = 4 the triples
    are flat three-term Ands, which differ from the join where the first two
    terms join to nothing."""
    das, pc, tpl, first, universe, compute_count = animals
    # Combinations with two or more Similarity templates are left out: the reference joins unordered
    # assignments in the order it meets them, so the count of such an And of three or more terms changes
    # with the order of the terms and with the iteration order of the reference's sets -- it is not a
    # function of the combination that a test could state.  (They take the per-query loop in any case.)
    unordered = [t[0] in UNORDERED_LINK_TYPES for t in tpl]
    every = [(i, *rest) for i in first for rest in itertools.combinations(range(len(tpl)), k - 1)
             if i not in rest and unordered[i] + sum(unordered[j] for j in rest) <= 1]
    # 150 spread over all of them, and up to 50 whose pairs all have a common answer in the oracle (of the
    # combinations spread evenly hardly one of four terms has a count)
    joins = {p: compute_count(flat_and, p) > 0 for p in itertools.combinations(range(len(tpl)), 2)}
    dense = [c for c in every if all(joins[tuple(sorted(p))] for p in itertools.combinations(c, 2))]
    combos = dense[::max(1, len(dense) // 50)][:50] + every[::max(1, len(every) // 150)][:150]
    assert 100 <= len(combos) <= 200
    before = das.db.conjunction_stats["device"]
    plain = das.isurprisingness(pc, combos, universe)
    assert das.db.conjunction_stats["device"] > before
    assert plain.count.dtype == np.uint64 and plain.value.dtype == np.float64 and len(plain) == len(combos)
    want_count = [compute_count(nested_and, c) for c in combos]
    assert plain.count.tolist() == want_count and any(want_count)
    terms = [[compute_count(nested_and, [i]) for i in c] for c in combos]
    assert terms == np.asarray(pc.count)[np.array(combos)].tolist()
    if k == 4:      # the case the flat And is about is in the sample
        assert any(compute_count(flat_and, c[:3]) != compute_count(nested_and, c[:3]) for c in combos)
    for normalized, got in ((False, plain), (True, das.isurprisingness(pc, combos, universe, normalized=True))):
        want = [notebook_isurprisingness(n, c, t, universe, compute_count, normalized)
                for c, n, t in zip(combos, want_count, terms)]
        np.testing.assert_allclose(got.value, want, rtol=1e-12, atol=0, equal_nan=True)
