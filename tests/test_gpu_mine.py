"""The exhaustive I-surprisingness search on the device (das_mine_combinations,
miner.hip; HipDB.mine) against brute force: every row of the search space
scored by miner.isurprisingness on the same HipDB, filtered and ordered as
miner.mine_host defines it -- rows, counts and the values bit for bit.

Two hand-built canonical KBs.  KB A (about 190 templates): random group
memberships and arity-3 links, a zero-count triangle (three groups that meet
pairwise but not all three), two groups with the same members (ties), a
black-listed type and, in a second PatternCounts, Similarity links.  KB T (the
tiling): one basic with exactly 300 partners and basics with 0, 1, 2 and 3,
so that with DAS_MX_TILE=64 one triangle spans 700 tiles and the last tile
holds the ranks of three basics."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from das_amd import _lib, miner
from das_amd.expression_hasher import ExpressionHasher as EH

pytestmark = pytest.mark.gpu

NONE = _lib.DAS_NONE
BLACK = ["Blk"]
TYPES = ["Inh", "Ex", "Blk", "Similarity"]


def H(name):
    return EH.terminal_hash("Concept", name)


def LH(link):
    return EH.expression_hash(EH.named_type_hash(link[0]), [H(n) for n in link[1:]])


def _text(links):
    nodes = list(dict.fromkeys(n for link in links for n in link[1:]))
    q = lambda n: f'"Concept {n}"'                                      # noqa: E731
    lines = ["(: Concept Type)"] + [f"(: {t} Type)" for t in TYPES] + [f'(: "{n}" Concept)' for n in nodes]
    lines += [f"({link[0]} {' '.join(q(n) for n in link[1:])})" for link in links]
    return "\n".join(lines) + "\n", nodes


def _links_a():
    rng = np.random.default_rng(11)
    xs = [f"x{i}" for i in range(30)]
    ls = [("Inh", xs[i], f"G{j}") for j in range(12) for i in range(30) if rng.random() < 0.3]
    ls += [("Ex", xs[int(rng.integers(30))], f"P{int(rng.integers(4))}", f"Q{int(rng.integers(4))}") for _ in range(40)]
    # three groups that meet pairwise -- t1 in TB and TI, t2 in TB and TJ, t3 in TI and TJ -- and not all three
    ls += [("Inh", "t1", "TB"), ("Inh", "t2", "TB"), ("Inh", "t1", "TI"), ("Inh", "t3", "TI"), ("Inh", "t2", "TJ"),
           ("Inh", "t3", "TJ")]
    # two groups with the same members: equal rows under different grounded targets
    ls += [("Inh", xs[i], d) for d in ("D1", "D2") for i in (0, 1, 5, 9)]
    ls += [("Blk", xs[i], "G0") for i in range(4)]
    return list(dict.fromkeys(ls))


LINKS_A = _links_a()
SIM = [("Similarity", "x0", "x1"), ("Similarity", "x1", "x0"), ("Similarity", "x0", "x5"), ("Similarity", "x5", "x0")]
TEXT_A, NODES_A = _text(LINKS_A + SIM)
UNIVERSE_A = len(LINKS_A)


def _links_t():
    rng = np.random.default_rng(5)
    ls = [("Inh", f"x{i}", "BIG") for i in range(20)]
    # link i makes three partners of BIG: [Ex,*,Pi,Qi] [Ex,*,*,Qi] [Ex,*,Pi,*]
    ls += [("Ex", f"x{i % 20}", f"P{i}", f"Q{i}") for i in range(100)]
    # more rows for those templates, so that triples of them do join
    ls += [("Ex", f"x{int(rng.integers(20))}", f"P{int(rng.integers(100))}", f"Q{int(rng.integers(100))}")
           for _ in range(60)]
    # u1 is in one candidate, u2 in two, u3 in three, u0 in none
    ls += [("Inh", "u0", "S0"), ("Inh", "u1", "S1"), ("Inh", "u2", "S2"), ("Inh", "u3", "S3")]
    ls += [("Ex", "u1", "P1", "Qn1"), ("Ex", "u2", "P2", "Qn2"), ("Ex", "u2", "Pn2", "Q3"), ("Ex", "u3", "P0", "Q0")]
    return list(dict.fromkeys(ls))


LINKS_T = _links_t()
TEXT_T, NODES_T = _text(LINKS_T)


def _fresh_db(text, **kw):
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0, **kw)
    db.pattern_black_list = list(BLACK)
    db.load_canonical(text)
    return db


class Env:
    """A KB on the device, the templates of `links` as one PatternCounts,
    addressed by template: (type, target | None, ...)."""

    def __init__(self, db, links, nodes):
        self.db = db
        self.pc = pc = db.pattern_counts([LH(link) for link in links])
        self.ids = dict(zip(nodes, np.asarray(db.ids_of([H(n) for n in nodes])).tolist()))
        assert min(self.ids.values()) >= 0
        self.rows = {key: i for i, key in enumerate(zip(pc.arity.tolist(), pc.type_id.tolist(),
                                                        *(pc.targets[:, p].tolist() for p in range(3))))}

    def row(self, tpl):
        tg = [self.ids[n] if n is not None else NONE for n in tpl[1:]]
        return self.rows[(len(tg), self.db.type_id[tpl[0]], *(tg + [NONE] * (3 - len(tg))))]

    def mine(self, basics, universe, **kw):
        before = dict(self.db.mine_stats)
        got = self.db.mine(self.pc, basics, universe, **kw)
        assert self.db.mine_stats == {"device": before["device"] + 1, "host": before["host"]}
        k = kw.get("ngram", 3)
        assert got.combos.dtype == np.uint32 and got.combos.shape == (len(got), k)
        assert got.count.dtype == np.uint64 and got.value.dtype == np.float64
        return got


_BRUTE = {}


def space_of(basics, candidates, ngram):
    return np.array([(b, *c) for b in basics for c in itertools.combinations(sorted(candidates), ngram - 1)
                     if b not in c], dtype=np.uint32).reshape(-1, ngram)


def brute(env, basics, candidates, universe, ngram, normalized):
    """(rows, count, value) of the whole space in enumeration order, scored
    once per (basics, candidates, ngram, normalized) and shared."""
    key = (id(env), tuple(basics), tuple(candidates), universe, ngram, normalized)
    if key not in _BRUTE:
        rows = space_of(basics, candidates, ngram)
        assert 0 < len(rows) <= 200_000
        res = miner.isurprisingness(env.db, env.pc, rows, universe, normalized)
        _BRUTE[key] = (rows, np.asarray(res.count), np.asarray(res.value))
    return _BRUTE[key]


def expected(env, basics, candidates, universe, ngram=3, support=0, normalized=False, top=None):
    rows, count, value = brute(env, basics, candidates, universe, ngram, normalized)
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero((value > 0) & (count >= support))
    keep = keep[np.argsort(-value[keep], kind="stable")][:top]
    return rows[keep], count[keep], value[keep]


def same(got, want):
    rows, count, value = want
    assert got.combos.tolist() == rows.tolist()
    assert got.count.tolist() == count.tolist()
    assert got.value.view(np.uint64).tolist() == value.view(np.uint64).tolist()      # bit for bit


@pytest.fixture(scope="module")
def env_a():
    return Env(_fresh_db(TEXT_A), LINKS_A, NODES_A)


@pytest.fixture(scope="module")
def env_t():
    return Env(_fresh_db(TEXT_T), LINKS_T, NODES_T)


def G(name):
    return ("Inh", None, name)


def basics_a(env):
    return [env.row(t) for t in (G("G0"), G("G1"), G("TB"), ("Ex", None, None, "Q0"), ("Ex", None, "P1", None),
                                 G("D1"))]


def test_kb_a_has_the_shapes(env_a):
    pc = env_a.pc
    assert 150 <= len(pc) <= 300
    assert len(basics_a(env_a)) * (len(pc) - 1) * (len(pc) - 2) // 2 <= 200_000
    blk = [i for i in range(len(pc)) if pc.type_id[i] == env_a.db.type_id["Blk"]]
    assert len(blk) == 5 and not pc.count[blk].any()
    assert int(pc.count[env_a.row(G("D1"))]) == int(pc.count[env_a.row(G("D2"))]) == 4
    assert ((pc.arity == 3) & ((pc.targets != NONE).sum(axis=1) == 1)).any()          # two-variable templates too


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("support", [0, 2])
@pytest.mark.parametrize("ngram", [2, 3])
def test_whole_list_is_brute_force(env_a, ngram, support, normalized):
    basics = basics_a(env_a)
    cands = list(range(len(env_a.pc)))
    want = expected(env_a, basics, cands, UNIVERSE_A, ngram, support, normalized)
    assert 0 < len(want[0]) <= _lib.MX_MAX_TOP
    got = env_a.mine(basics, UNIVERSE_A, ngram=ngram, support=support, normalized=normalized, top=_lib.MX_MAX_TOP)
    same(got, want)
    assert got.searched == len(space_of(basics, cands, ngram)) and got.tiles == 1
    # a basic that is also a candidate is never inside its own tuple
    assert not (got.combos[:, 1:] == got.combos[:, :1]).any()
    # a black-listed type's template (count 0) is in no reported row
    blk = np.flatnonzero(env_a.pc.type_id == env_a.db.type_id["Blk"])
    assert not np.isin(got.combos, blk).any()
    if ngram == 3:
        # pruned rows are really zero: fewer combinations counted than the space has, and the same answer
        assert got.scored < got.searched
        triples = sum(s * (s - 1) // 2 for s in partner_sizes(env_a, basics, cands))
        assert got.scored == len(basics) * len(cands) + triples
    else:
        assert got.scored == len(basics) * len(cands)
    # ready for das.query
    terms = [env_a.pc.pattern(int(i)) for i in got.combos[0]]
    assert repr(got.pattern(0)) == repr(miner.build_composite_pattern(terms))


def partner_sizes(env, basics, cands):
    pairs = np.array([(b, c) for b in basics for c in cands], dtype=np.uint32)
    counts = env.db.conjunction_counts(env.pc, pairs).reshape(len(basics), len(cands))
    return [int(((counts[i] > 0) & (np.asarray(cands) != b)).sum()) for i, b in enumerate(basics)]


def test_truncation_is_a_prefix(env_a):
    basics, cands = basics_a(env_a), list(range(len(env_a.pc)))
    for ngram in (2, 3):
        for top in (1, 3):
            want = expected(env_a, basics, cands, UNIVERSE_A, ngram, top=top)
            same(env_a.mine(basics, UNIVERSE_A, ngram=ngram, top=top), want)


def test_zero_count_triangle(env_a):
    """x1 in b and i, x2 in b and j, x3 in i and j, nothing in all three:
    count 0 and the value min(sp) > 0 -- reported with support 0, not with
    support 1, not normalized (the notebook divides by zero there)."""
    b, i, j = (env_a.row(G(n)) for n in ("TB", "TI", "TJ"))
    i, j = sorted((i, j))
    assert env_a.db.conjunction_counts(env_a.pc, [(b, i), (b, j), (i, j)]).tolist() == [1, 1, 1]
    assert env_a.db.conjunction_counts(env_a.pc, [(b, i, j)]).tolist() == [0]
    got = env_a.mine([b], UNIVERSE_A, candidates=[i, j])
    u = float(UNIVERSE_A)
    sp = [(2 / u) * (2 / u) * (2 / u), (1 / u) * (2 / u), (1 / u) * (2 / u), (1 / u) * (2 / u)]
    assert got.combos.tolist() == [[b, i, j]] and got.count.tolist() == [0] and got.value.tolist() == [min(sp)]
    assert got.searched == 1 and got.scored == 2 + 1
    assert len(env_a.mine([b], UNIVERSE_A, candidates=[i, j], support=1)) == 0
    assert len(env_a.mine([b], UNIVERSE_A, candidates=[i, j], normalized=True)) == 0
    # among all candidates the row is found too
    full = env_a.mine([b], UNIVERSE_A, top=_lib.MX_MAX_TOP)
    assert [b, i, j] in full.combos.tolist()


def test_ties_keep_the_enumeration_order(env_a):
    d1, d2 = sorted((env_a.row(G("D1")), env_a.row(G("D2"))))
    g0, g1 = env_a.row(G("G0")), env_a.row(G("G1"))
    cands = list(range(len(env_a.pc)))
    # as candidates: (b, D1) before (b, D2), equal values
    got = env_a.mine([g0, g1], UNIVERSE_A, ngram=2, top=_lib.MX_MAX_TOP)
    same(got, expected(env_a, [g0, g1], cands, UNIVERSE_A, 2))
    rows = got.combos.tolist()
    at1, at2 = rows.index([g0, d1]), rows.index([g0, d2])
    assert at2 == at1 + 1 and got.value[at1] == got.value[at2] and got.count[at1] == got.count[at2]
    # as basics: the order of the basics is the order of the ties
    for order in ([d1, d2], [d2, d1]):
        for ngram in (2, 3):
            got = env_a.mine(order, UNIVERSE_A, ngram=ngram, top=_lib.MX_MAX_TOP)
            same(got, expected(env_a, order, cands, UNIVERSE_A, ngram))
            rows = got.combos.tolist()
            first = next(r for r in rows if d1 not in r[1:] and d2 not in r[1:])
            other = [order[1] if first[0] == order[0] else order[0]] + first[1:]
            assert first[0] == order[0] and rows.index(other) > rows.index(first)
            assert got.value[rows.index(other)] == got.value[rows.index(first)]


def test_host_path_switches(env_a):
    """DAS_MINER=0, and an unordered candidate: mine_host answers, the same
    rows, and `mine_stats["host"]` counts the call."""
    db, pc = env_a.db, env_a.pc
    basics = basics_a(env_a)[:2]
    cands = list(range(0, len(pc), 9))
    want = expected(env_a, basics, cands, UNIVERSE_A, 3)
    same(env_a.mine(basics, UNIVERSE_A, candidates=cands, top=_lib.MX_MAX_TOP), want)
    before = dict(db.mine_stats)
    old = os.environ.get("DAS_MINER")
    os.environ["DAS_MINER"] = "0"
    try:
        got = db.mine(pc, basics, UNIVERSE_A, candidates=cands, top=_lib.MX_MAX_TOP)
    finally:
        if old is None:
            del os.environ["DAS_MINER"]
        else:
            os.environ["DAS_MINER"] = old
    same(got, want)
    assert db.mine_stats == {"device": before["device"], "host": before["host"] + 1}
    assert got.scored == got.searched == len(space_of(basics, cands, 3))
    # a PatternCounts that also holds the Similarity templates: one of them among the candidates
    env_u = Env(db, LINKS_A + SIM, NODES_A)
    sim = int(np.flatnonzero(env_u.pc.type_id == db.type_id["Similarity"])[0])
    bu = [env_u.row(G("G0")), env_u.row(G("D1"))]
    cu = sorted(set(range(0, len(env_u.pc), 9)) | {sim})
    before = dict(db.mine_stats)
    got = db.mine(env_u.pc, bu, UNIVERSE_A, ngram=2, candidates=cu, top=_lib.MX_MAX_TOP)
    assert db.mine_stats == {"device": before["device"], "host": before["host"] + 1}
    same(got, expected(env_u, bu, cu, UNIVERSE_A, 2))
    # without it the device answers the same call
    cu.remove(sim)
    got = env_u.mine(bu, UNIVERSE_A, ngram=2, candidates=cu, top=_lib.MX_MAX_TOP)
    same(got, expected(env_u, bu, cu, UNIVERSE_A, 2))


def test_refusal_comes_before_any_tile(env_a):
    basics, m = basics_a(env_a), len(env_a.pc)
    scored = env_a.mine(basics, UNIVERSE_A, top=1).scored
    assert scored > len(basics) * m
    with pytest.raises(ValueError, match=str(scored)):
        env_a.db.mine(env_a.pc, basics, UNIVERSE_A, max_combinations=scored - 1)
    assert len(env_a.mine(basics, UNIVERSE_A, top=1, max_combinations=scored)) == 1
    # the matrix alone is over the limit: refused with nothing launched
    launches = _lib.counters()[0]
    with pytest.raises(ValueError, match=str(len(basics) * m)):
        env_a.db.mine(env_a.pc, basics, UNIVERSE_A, max_combinations=len(basics) * m - 1)
    assert _lib.counters()[0] == launches
    # the host path refuses its own space
    with pytest.raises(ValueError, match=str(len(space_of(basics, range(m), 2)))):
        miner.mine_host(env_a.db, env_a.pc, basics, UNIVERSE_A, ngram=2, max_combinations=10)


# ---------------------------------------------------------------------------
# tiling
# ---------------------------------------------------------------------------

def _cands_t(env):
    out = []
    for i in range(100):
        out += [env.row(("Ex", None, f"P{i}", f"Q{i}")), env.row(("Ex", None, None, f"Q{i}")),
                env.row(("Ex", None, f"P{i}", None))]
    assert len(set(out)) == 300
    return sorted(out)


@pytest.mark.parametrize("order", [("S0", "S1", "S2", "BIG"), ("BIG", "S3", "S0", "S2")])
def test_tiles_of_64_give_the_same_answer(env_t, order):
    cands = _cands_t(env_t)
    basics = [env_t.row(G(n)) for n in order]
    sizes = dict(zip(order, partner_sizes(env_t, basics, cands)))
    want_sizes = {"S0": 0, "S1": 1, "S2": 2, "S3": 3, "BIG": 300}
    assert sizes == {n: want_sizes[n] for n in order}
    universe = len(LINKS_T)
    want = expected(env_t, basics, cands, universe, 3)
    assert len(want[0]) > 64                                            # survivors of many tiles meet in the top rows
    whole = env_t.mine(basics, universe, candidates=cands, top=_lib.MX_MAX_TOP)
    same(whole, want)
    triples = sum(s * (s - 1) // 2 for s in sizes.values())
    assert whole.tiles == 1 and whole.scored == 4 * 300 + triples < whole.searched == 4 * 300 * 299 // 2
    old = os.environ.get("DAS_MX_TILE")
    os.environ["DAS_MX_TILE"] = "64"
    try:
        tiled = env_t.mine(basics, universe, candidates=cands, top=_lib.MX_MAX_TOP)
        short = env_t.mine(basics, universe, candidates=cands, top=5, support=1)
        pairs = env_t.mine(basics, universe, ngram=2, candidates=cands, top=_lib.MX_MAX_TOP)
    finally:
        if old is None:
            del os.environ["DAS_MX_TILE"]
        else:
            os.environ["DAS_MX_TILE"] = old
    same(tiled, want)
    # 300 partners: a triangle of 44,850 ranks over 700 tiles; the ranks of the small basics share a tile with it
    assert tiled.tiles == -(-triples // 64) > 700 and triples % 64 != 0
    same(short, expected(env_t, basics, cands, universe, 3, support=1, top=5))
    same(pairs, expected(env_t, basics, cands, universe, 2))
    assert pairs.tiles == -(-4 * 300 // 64)


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------

def _abi_args(env):
    pc = env.pc
    used = [env.row(t) for t in (G("G0"), G("G1"), G("D1"), ("Ex", None, None, "Q0"))]
    tpl = np.vstack([pc.arity[used], pc.type_id[used], pc.targets[used].T]).astype(np.uint32)
    return tpl, np.asarray(pc.count)[used].astype(np.uint64)


def raw(ctx, tpl, cnt, basics, cands, k=3, universe=UNIVERSE_A, support=0, normalized=0, top=4, limit=2 ** 32,
        null=()):
    """das_mine_combinations as called from C: (status, rows, stats)."""
    tpl = np.ascontiguousarray(tpl, dtype=np.uint32)
    cnt = np.ascontiguousarray(cnt, dtype=np.uint64)
    b = np.ascontiguousarray(basics, dtype=np.uint32)
    c = np.ascontiguousarray(cands, dtype=np.uint32)
    combo, count, value = np.zeros(4 * 65536, np.uint32), np.zeros(65536, np.uint64), np.zeros(65536, np.float64)
    n_out, stats = C.c_uint32(), np.zeros(3, dtype=np.uint64)
    ptr = {"tpl": _lib.ptr(tpl), "cnt": _lib.ptr(cnt), "basics": _lib.ptr(b), "cands": _lib.ptr(c),
           "combo": _lib.ptr(combo), "count": _lib.ptr(count), "value": _lib.ptr(value),
           "n_out": C.cast(C.byref(n_out), C.c_void_p), "stats": _lib.ptr(stats)}
    for name in null:
        ptr[name] = None
    rc = _lib.lib().das_mine_combinations(ctx.h, ptr["tpl"], tpl.shape[1], ptr["cnt"], ptr["basics"], b.size,
                                          ptr["cands"], c.size, k, universe, support, normalized, top, limit,
                                          ptr["combo"], ptr["count"], ptr["value"], ptr["n_out"], ptr["stats"])
    return rc, n_out.value, stats.tolist()


def test_raw_abi_validates_before_any_launch(env_a):
    db = env_a.db
    tpl, cnt = _abi_args(env_a)
    sim = np.hstack([tpl, np.array([[2], [db.type_id["Similarity"]], [env_a.ids["x0"]], [NONE], [NONE]], np.uint32)])
    bad_arity = np.hstack([tpl, np.array([[4], [db.type_id["Ex"]], [env_a.ids["x0"]], [NONE], [NONE]], np.uint32)])
    cnt5 = np.append(cnt, np.uint64(1))
    fresh = _lib.Context(0)
    launches = _lib.counters()[0]
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    cases = [
        (INV, dict(k=1)), (INV, dict(k=4)),
        (INV, dict(basics=[4])), (INV, dict(cands=[1, 4])),                      # index >= m
        (INV, dict(basics=[0, 0])), (INV, dict(cands=[1, 2, 1])),                # a basic / a candidate twice
        (INV, dict(top=0)), (INV, dict(top=65537)),
        (INV, dict(universe=0)),
        (INV, dict(null=("tpl",))), (INV, dict(null=("cnt",))), (INV, dict(null=("basics",))),
        (INV, dict(null=("cands",))), (INV, dict(null=("combo",))), (INV, dict(null=("count",))),
        (INV, dict(null=("value",))), (INV, dict(null=("n_out",))), (INV, dict(null=("stats",))),
        (INV, dict(tpl=bad_arity, cnt=cnt5)),
        (UNS, dict(tpl=sim, cnt=cnt5)),
    ]
    for want, kw in cases:
        args = dict(tpl=tpl, cnt=cnt, basics=[0, 1], cands=[0, 1, 2, 3])
        args.update(kw)
        assert raw(db.ctx, **args)[0] == want, kw
    assert raw(fresh, tpl, cnt, [0, 1], [0, 1, 2, 3])[0] == _lib.ERR_NOT_BUILT
    # over the limit: its own status, the two sizes filled in, before anything is launched
    rc, n, stats = raw(db.ctx, tpl, cnt, [0, 1], [0, 1, 2, 3], limit=7)
    assert (rc, n, stats) == (_lib.ERR_LIMIT, 0, [2 * 3, 8, 0])
    # nothing to search: an empty answer
    assert raw(db.ctx, tpl, cnt, [], [0, 1, 2, 3], null=("basics",)) == (0, 0, [0, 0, 0])
    assert raw(db.ctx, tpl, cnt, [0, 1], [], null=("cands",)) == (0, 0, [0, 0, 0])
    assert _lib.counters()[0] == launches
    # after the matrix: refused with the sizes, no tile scored
    rc, n, stats = raw(db.ctx, tpl, cnt, [0, 1], [0, 1, 2, 3], limit=8)
    partners = partner_sizes(env_a, [env_a.row(G("G0")), env_a.row(G("G1"))],
                             [env_a.row(t) for t in (G("G0"), G("G1"), G("D1"), ("Ex", None, None, "Q0"))])
    triples = sum(s * (s - 1) // 2 for s in partners)
    assert triples > 0 and (rc, n, stats) == (_lib.ERR_LIMIT, 0, [6, 8 + triples, 0])
    rc, n, stats = raw(db.ctx, tpl, cnt, [0, 1], [0, 1, 2, 3], limit=8 + triples)
    assert rc == 0 and stats == [6, 8 + triples, 1] and n <= 4
    assert _lib.counters()[0] > launches
    # the wrapper raises what the codes map to
    with pytest.raises(ValueError):
        db.ctx.mine_combinations(tpl, cnt, [0, 0], [1, 2], 3, UNIVERSE_A)
    with pytest.raises(NotImplementedError):
        db.ctx.mine_combinations(sim, cnt5, [0], [1, 4], 3, UNIVERSE_A)


def test_sharded_index_is_unsupported():
    from das_amd.database.hip_db import HipDB
    db = HipDB(device=0)
    db.load_arrays(_lib.parse_canonical(TEXT_A), shard=(0, 2))
    tpl = np.array([[2, 2], [db.type_id["Inh"]] * 2, [NONE, NONE], [0, 1], [NONE, NONE]], dtype=np.uint32)
    launches = _lib.counters()[0]
    assert raw(db.ctx, tpl, [1, 1], [0], [0, 1], k=2)[0] == _lib.ERR_UNSUPPORTED
    assert _lib.counters()[0] == launches


def test_rebuild_mines_the_new_kb():
    db = _fresh_db(TEXT_T)
    first = Env(db, LINKS_T, NODES_T)
    big = first.row(G("BIG"))
    assert len(first.mine([big], len(LINKS_T), ngram=2, top=3)) == 3
    db.load_canonical(TEXT_A)
    second = Env(db, LINKS_A, NODES_A)
    basics, cands = basics_a(second)[:3], list(range(0, len(second.pc), 3))
    got = second.mine(basics, UNIVERSE_A, candidates=cands, top=_lib.MX_MAX_TOP)
    same(got, expected(second, basics, cands, UNIVERSE_A, 3))
    assert db.mine_stats["host"] == 0
