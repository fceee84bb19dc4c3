"""The case tables of the binding-table operator tests, in one place:
test_table_model.py admits each case on the host model alone (it produces
rows, drops and keeps what it is meant to), test_gpu_table_ops.py runs the
same cases on the device.  A case is an id and a builder `make(rng, hi)` of
its inputs; the rng is seeded from the id, `hi` is the KB's atom count (every
generated value is an atom id)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import table_model as TM
from tests.table_model import ORDERED, NTable

# row counts either side of every regime change: the wave (64), the scan tile
# (2048), the radix-sort tile (4096), the one-workgroup compaction (kSmallScan
# = 16384), and one size of several tiles
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4097, 16384, 16385, 40001)
JOIN_CAP = 200_000              # a join case's output stays below this
SEQ_CAP = 20_000                # an operator-sequence table stays below this
SEQ_SEEDS = (1, 2, 3, 4, 5)
SEQ_STEPS = 12

Case = namedtuple("Case", "id make")


def kb_arrays():
    """The synthetic KB of the device context: 8192 nodes and a few links."""
    from das_amd import synthetic
    return synthetic.powerlaw_kb(n_nodes=8192, n_links=512, link_types=2, seed=11)


@functools.lru_cache(maxsize=None)
def n_atoms():
    """Atom count of kb_arrays() from the oracle's KB (the device index must report the same)."""
    from oracle import das_oracle as O
    kb = O.KB.from_arrays(kb_arrays())
    return len(set(kb.nodes) | set(kb.links))


_BUILT = {}


def build(case):
    """The case's inputs (built once per process, then shared and left unchanged)."""
    if case.id not in _BUILT:
        _BUILT[case.id] = case.make(np.random.default_rng(zlib.crc32(case.id.encode())), n_atoms())
    return _BUILT[case.id]


_WANT = {}


def want(case, fn):
    """fn(inputs) of the model, computed once per case, fn and process."""
    key = (case.id, fn.__name__)
    if key not in _WANT:
        _WANT[key] = fn(build(case))
    return _WANT[key]


def _ids(cases):
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return cases


def _rows(rng, n, k, lo, hi):
    return rng.integers(lo, hi, size=(n, k), dtype=np.int64)


# --------------------------------------------------------------------- join
def _keyed_pair(rng, hi, nshared, npr, nb, fan, same_key=False):
    """Probe a (shared vars + 10) and build b (shared vars + 11): every build
    key occurs about `fan` times; 4 of 5 probe rows carry a build key."""
    shared = list(range(nshared))
    if fan == 0:                       # disjoint first key column: nothing joins
        ka = _rows(rng, npr, nshared, 0, hi // 2)
        kb = _rows(rng, nb, nshared, hi // 2, hi)
    elif same_key:
        key = _rows(rng, 1, nshared, 0, hi)
        ka, kb = np.repeat(key, npr, 0), np.repeat(key, nb, 0)
    else:
        pool = np.unique(_rows(rng, max(1, nb // fan), nshared, 0, hi), axis=0)
        kb = pool[rng.permutation(nb) % len(pool)]
        ka = pool[rng.integers(0, len(pool), npr)]
        miss = rng.random(npr) < 0.2
        ka[miss] = _rows(rng, int(miss.sum()), nshared, 0, hi)
    a = NTable(ORDERED, shared + [10], np.concatenate([ka, _rows(rng, npr, 1, 0, hi)], 1))
    b = NTable(ORDERED, shared + [11], np.concatenate([kb, _rows(rng, nb, 1, 0, hi)], 1))
    return a, b


def _join_case(cid, fn, rows=True, no_overload=False, swap=False, bounds=None, covering=False):
    """rows: the case is meant to produce output (False: none; None: either).  swap: join(b, a) is run
    too.  bounds 'tight': both inputs declare their columns' min / max."""
    def make(rng, hi):
        a, b = fn(rng, hi)
        return {"a": a, "b": b, "rows": rows, "no_overload": no_overload, "swap": swap, "bounds": bounds,
                "covering": covering}
    return Case(cid, make)


def _join_cases():
    out = []
    # sort-merge: two and three shared variables
    for ns in (2, 3):
        for n in SIZES:
            for fan in (0, 1, 8):
                if fan == 8 and n > 16385:          # ~6.4 outputs per probe row: over the cap at 40001
                    continue
                def fn(rng, hi, ns=ns, n=n, fan=fan):
                    return _keyed_pair(rng, hi, ns, n, max(1, n // 3), fan)
                out.append(_join_case(f"merge{ns}-n{n}-fan{fan}", fn, swap=n <= 4097,
                                      rows=False if fan == 0 or n == 0 else True if n >= 63 else None))
        out.append(_join_case(f"merge{ns}-samekey",
                              lambda rng, hi, ns=ns: _keyed_pair(rng, hi, ns, 600, 300, 1, same_key=True)))
    # cartesian: every k_cartesian<N> and the generic kernel, total % 4 = 0, 1, 2, 3
    for w in (2, 3, 4, 5, 6, 7):
        for na, nb in ((64, 64), (65, 61), (63, 66), (67, 65)):
            def fn(rng, hi, w=w, na=na, nb=nb):
                wa = (w + 1) // 2
                return (TM.ordered(rng, range(wa), na, hi), TM.ordered(rng, range(20, 20 + w - wa), nb, hi))
            out.append(_join_case(f"cart-w{w}-{na}x{nb}", fn, swap=True))
    for na, nb in ((1, 1), (1, 5), (3, 1), (1025, 97), (97, 1025)):
        def fn(rng, hi, na=na, nb=nb):
            return TM.ordered(rng, [0], na, hi), TM.ordered(rng, [1], nb, hi)
        out.append(_join_case(f"cart-w2-{na}x{nb}", fn, swap=True))
    # one shared variable: the direct-address join, bounds unset and tight
    for n, fan in ((4097, 3), (40001, 1)):
        for bounds in (None, "tight"):
            out.append(_join_case(f"direct-n{n}-{bounds or 'unset'}",
                                  lambda rng, hi, n=n, fan=fan: _keyed_pair(rng, hi, 1, n, n // 3, fan),
                                  swap=n <= 4097, bounds=bounds))
    # ... and a one-column build side: the key-set filter (distinct keys), the direct join (repeated keys)
    for name, dup in (("distinct", False), ("repeats", True)):
        def fn(rng, hi, dup=dup):
            a = TM.ordered(rng, [0, 1], 16385, hi)
            keys = rng.permutation(hi)[:3000]
            if dup:
                keys[1500:] = keys[:1500]
            return a, NTable(ORDERED, [1], keys.reshape(-1, 1))
        for bounds in (None, "tight"):
            out.append(_join_case(f"keyset-{name}-{bounds or 'unset'}", fn, bounds=bounds))
    # no_overload: values of a small range, so that rows repeat a value
    # (name, a's variables, rows, range, b's variables, rows, range)
    for name, va, na, ra, vb, nb, rb in (("direct", [0, 1], 300, 6, [1, 2], 200, 6),
                                         ("merge", [0, 1, 2], 300, 5, [1, 2, 3], 300, 5),
                                         ("cart", [0], 70, 9, [1, 2], 50, 9),
                                         ("covering", [0, 1, 2], 300, 4, [1, 2], 12, 4)):
        def fn(rng, hi, va=va, na=na, ra=ra, vb=vb, nb=nb, rb=rb):
            return TM.ordered(rng, va, na, ra), TM.ordered(rng, vb, nb, rb)
        out.append(_join_case(f"overload-{name}", fn, no_overload=True, swap=True, covering=name == "covering"))
    # either side empty
    for ns in (0, 1, 2):
        for na, nb in ((0, 50), (50, 0), (0, 0)):
            def fn(rng, hi, ns=ns, na=na, nb=nb):
                shared = list(range(ns))
                return TM.ordered(rng, shared + [10], na, hi), TM.ordered(rng, shared + [11], nb, hi)
            out.append(_join_case(f"empty-s{ns}-{na}x{nb}", fn, rows=False))
    return _ids(out)


JOIN_CASES = _join_cases()


def join_want(inp):
    return TM.join(inp["a"], inp["b"], inp["no_overload"])


# ------------------------------------------- join / antijoin with unordered and composite operands
THETA_HI = 7                     # a small value range: the containment checks hit and miss


def theta_operands(rng):
    """name -> table; 1 to 300 rows, with and without shared ordered variables."""
    t = {}
    t["O01"] = TM.ordered(rng, [0, 1], 300, THETA_HI)
    t["O12"] = TM.ordered(rng, [1, 2], 120, THETA_HI)
    t["O5"] = TM.ordered(rng, [5], 1, THETA_HI)
    t["U01"] = TM.unordered(rng, [0, 1], 120, THETA_HI)
    t["U012"] = TM.unordered(rng, [0, 1, 2], 90, THETA_HI)
    t["U01s"] = TM.unordered(rng, [0, 1], 5, THETA_HI)
    t["O01s"] = TM.ordered(rng, [0, 1], 3, THETA_HI)
    t["C_01s"] = TM.composite(rng, [], [[0, 1]], 3, THETA_HI)
    t["C0_01"] = TM.composite(rng, [0], [[0, 1]], 100, THETA_HI)
    t["C01_012"] = TM.composite(rng, [0, 1], [[0, 1, 2]], 80, THETA_HI)
    t["C_01_12"] = TM.composite(rng, [], [[0, 1], [1, 2]], 60, THETA_HI)
    # a composite's ordered part agrees with its members where the algebra made it: make some rows do
    for name in ("C0_01", "C01_012"):
        c = t[name]
        k = sum(1 for m in c.members if m < 0)
        fix = rng.random(c.nrows) < 0.6
        for j in range(k):
            c.rows[fix, j] = c.rows[fix, k + j]
    return t


def _theta_cases():
    names = ["O01", "O12", "O5", "O01s", "U01", "U012", "U01s", "C_01s", "C0_01", "C01_012", "C_01_12"]
    out = []
    for x in names:
        for y in names:
            if x[0] == "O" and y[0] == "O":
                continue                      # ordered pairs: the ordered cases above
            def make(rng, hi, x=x, y=y):
                t = theta_operands(np.random.default_rng(77))    # the same operands in every pair
                return {"a": t[x], "b": t[y]}
            out.append(Case(f"theta-{x}-{y}", make))
    # an empty side: the output schema without a row, and no AttributeError (no pair is evaluated)
    for x, y, which in (("U01", "O01", "b"), ("O01", "U01", "a"), ("C0_01", "C_01_12", "b"), ("O01", "C_01_12", "a")):
        def make(rng, hi, x=x, y=y, which=which):
            t = theta_operands(np.random.default_rng(77))
            inp = {"a": t[x], "b": t[y]}
            e = inp[which]
            inp[which] = NTable(e.kind, e.vars, e.rows[:0], e.members)
            return inp
        out.append(Case(f"theta-empty-{which}-{x}-{y}", make))
    # no_overload where the two ordered parts do not cover each other (CK_DISTINCT)
    for x, y in (("C0_01", "O12"), ("O12", "C0_01")):
        def make(rng, hi, x=x, y=y):
            t = theta_operands(np.random.default_rng(77))
            return {"a": t[x], "b": t[y], "no_overload": True}
        out.append(Case(f"theta-overload-{x}-{y}", make))
    return _ids(out)


THETA_CASES = _theta_cases()


def theta_join_want(inp):
    """The model's table, or the exception class the oracle raises."""
    try:
        return TM.join(inp["a"], inp["b"], inp.get("no_overload", False))
    except AttributeError:
        return AttributeError


def theta_anti_want(inp):
    try:
        return TM.antijoin(inp["a"], inp["b"])
    except AttributeError:
        return AttributeError


# ----------------------------------------------------------------- antijoin
def _anti_cases():
    out = []
    for tv in ((1,), (0, 2), (0, 1, 2)):
        for n in SIZES:
            def make(rng, hi, tv=tv, n=n):
                a = TM.ordered(rng, [0, 1, 2], n, hi)
                cols = [a.vars.index(v) for v in tv]
                nt = max(1, n // 8)
                # half of t: projections of rows of a's first half (those rows go); half random
                hit = np.zeros((0, len(tv)), np.int64)
                if n:
                    hit = a.rows[rng.integers(0, max(1, n // 2), nt // 2)][:, cols]
                t = NTable(ORDERED, tv, np.concatenate([hit, _rows(rng, nt - len(hit), len(tv), 0, hi)]))
                return {"a": a, "t": t, "covered": True}
            out.append(Case(f"anti-c{len(tv)}-n{n}", make))
    for n in (65, 16385):
        out.append(Case(f"anti-uncovered-n{n}", lambda rng, hi, n=n: {
            "a": TM.ordered(rng, [0, 1, 2], n, hi), "t": TM.ordered(rng, [1, 7], 40, hi), "covered": False}))
    out.append(Case("anti-t-empty", lambda rng, hi: {
        "a": TM.ordered(rng, [0, 1, 2], 2049, hi), "t": TM.ordered(rng, [1], 0, hi), "covered": False}))
    return _ids(out)


ANTI_CASES = _anti_cases()


def anti_want(inp):
    return TM.antijoin(inp["a"], inp["t"])


# -------------------------------------------------------------------- dedup
def _dedup_cases():
    out = []
    for w in (1, 2, 4, 16):
        for dup in (0.0, 0.5, 1.0):
            for n in SIZES:
                out.append(Case(f"dedup-w{w}-dup{dup}-n{n}", lambda rng, hi, w=w, dup=dup, n=n: {
                    "t": TM.ordered(rng, range(w), n, hi, dup=dup), "drops": dup > 0 and n >= 2,
                    "keeps": n >= 1}))
    out.append(Case("dedup-unordered", lambda rng, hi: {"t": TM.unordered(rng, [0, 1], 300, 6), "drops": True,
                                                        "keeps": True}))

    def comp(rng, hi):
        # two members over the same variables: equal tuples cancel (the XOR of the member hashes)
        t = TM.composite(rng, [0], [[1, 2], [1, 2]], 300, 4)
        return {"t": t, "drops": True, "keeps": True}
    out.append(Case("dedup-composite", comp))
    return _ids(out)


DEDUP_CASES = _dedup_cases()


def dedup_want(inp):
    return TM.dedup(inp["t"])


# ------------------------------------------------------- set_dedup / set_minus
def _twin_members(rng, n, hi):
    """Composite over ordered (0, 1) with two members on (2, 3): where the
    members are equal they cancel and the row's identity is its ordered part."""
    return TM.composite(rng, [0, 1], [[2, 3], [2, 3]], n, hi)


def _set_lists():
    """id -> builder of a list of tables."""
    L = {}
    L["odd3-then-2049"] = lambda rng, hi: [TM.ordered(rng, [0, 1], 3, 40), TM.ordered(rng, [0, 1], 2049, 40)]
    L["odd3-then-40001"] = lambda rng, hi: [TM.ordered(rng, [0, 1], 3, 150), TM.ordered(rng, [0, 1], 40001, 150)]
    L["odd2049-then-40001"] = lambda rng, hi: [TM.ordered(rng, [0, 1], 2049, 200), TM.ordered(rng, [0, 1], 40001, 200)]
    L["one-table"] = lambda rng, hi: [TM.ordered(rng, [0, 1, 2], 2049, hi, dup=0.5)]
    L["empty-in-the-middle"] = lambda rng, hi: [TM.ordered(rng, [0, 1], 300, 15), TM.ordered(rng, [0, 1], 0, 15),
                                                TM.ordered(rng, [0, 1], 301, 15)]
    L["same-ovars-two-kinds"] = lambda rng, hi: [TM.ordered(rng, [0, 1], 200, 4), _twin_members(rng, 200, 4)]
    L["twin-members"] = lambda rng, hi: [_twin_members(rng, 151, 4),
                                         TM.composite(rng, [0, 1], [[2, 3]], 150, 4),
                                         _twin_members(rng, 149, 4)]
    L["four-mixed"] = lambda rng, hi: [TM.unordered(rng, [0, 1], 150, 6), TM.composite(rng, [], [[0, 1]], 100, 6),
                                       TM.ordered(rng, [0], 64, 20), TM.unordered(rng, [0, 1], 65, 6)]
    L["no-ovars-twins"] = lambda rng, hi: [TM.composite(rng, [], [[0, 1], [0, 1]], 200, 4),
                                           TM.composite(rng, [], [[0, 1], [0, 1]], 60, 4),
                                           TM.composite(rng, [], [[0, 1]], 30, 4)]
    return L


def _set_dedup_cases():
    return _ids([Case(f"setdedup-{k}", lambda rng, hi, f=f: {"ts": f(rng, hi)}) for k, f in _set_lists().items()])


SET_DEDUP_CASES = _set_dedup_cases()


def set_dedup_want(inp):
    return TM.set_dedup(inp["ts"])


def _sample_of(rng, ts, share):
    """One table per schema of ts holding `share` of each table's rows (with repeats)."""
    out = []
    for t in ts:
        if t.nrows:
            pick = rng.integers(0, t.nrows, max(1, int(share * t.nrows)))
            out.append(NTable(t.kind, t.vars, t.rows[pick], t.members))
    return out


def _set_minus_cases():
    out = []
    for k, f in _set_lists().items():
        def some(rng, hi, f=f):
            a = f(rng, hi)
            return {"a": a, "b": _sample_of(rng, a, 0.3), "drops": True, "keeps": True}
        out.append(Case(f"setminus-{k}", some))
    L = _set_lists()
    out.append(Case("setminus-b-empty", lambda rng, hi: {"a": L["odd3-then-2049"](rng, hi), "b": [], "drops": False,
                                                         "keeps": True}))

    def superset(rng, hi):
        a = L["four-mixed"](rng, hi)
        return {"a": a, "b": list(reversed(a)) + [TM.ordered(rng, [0], 30, 20)], "drops": True, "keeps": False}
    out.append(Case("setminus-b-superset", superset))

    def hole(rng, hi):
        a = L["odd3-then-40001"](rng, hi)
        return {"a": a, "b": [TM.ordered(rng, [0, 1], 5000, 150), TM.ordered(rng, [0, 1], 0, 150)], "drops": True,
                "keeps": True}
    out.append(Case("setminus-b-with-empty-table", hole))

    def kinds(rng, hi):
        # an ordered b takes the composite rows whose twin members cancel
        a = L["same-ovars-two-kinds"](rng, hi)
        return {"a": a, "b": [TM.ordered(rng, [0, 1], 12, 4)], "drops": True, "keeps": True}
    out.append(Case("setminus-ordered-from-composite", kinds))
    return _ids(out)


SET_MINUS_CASES = _set_minus_cases()


def set_minus_want(inp):
    return TM.set_minus(inp["a"], inp["b"])


# ------------------------------------------------------------------- concat
def _concat_cases():
    out = []
    for name, ns in (("odd-offsets", (1, 3, 2048, 0, 5)), ("single", (2049,)), ("all-empty", (0, 0, 0)),
                     ("two-large", (16385, 40001))):
        out.append(Case(f"concat-{name}",
                        lambda rng, hi, ns=ns: {"ts": [TM.ordered(rng, [0, 1, 2], n, hi) for n in ns]}))
    out.append(Case("concat-composite", lambda rng, hi: {
        "ts": [TM.composite(rng, [0], [[1, 2]], n, hi) for n in (65, 1, 130)]}))
    out.append(Case("concat-unordered", lambda rng, hi: {"ts": [TM.unordered(rng, [1, 2, 3], n, hi) for n in (7, 64)]}))
    return _ids(out)


CONCAT_CASES = _concat_cases()


def concat_mismatches(rng, hi):
    """Pairs whose schemas differ: variables, width, kind, members."""
    o = TM.ordered(rng, [0, 1], 5, hi)
    return [[o, TM.ordered(rng, [0, 2], 5, hi)], [o, TM.ordered(rng, [0, 1, 2], 5, hi)],
            [o, TM.unordered(rng, [0, 1], 5, hi)],
            [TM.composite(rng, [0], [[1, 2]], 5, hi), TM.composite(rng, [], [[0], [1, 2]], 5, hi)]]


# ------------------------------------------------------ gather / gather_ranges
def _gather_cases():
    def big(rng, hi):
        t = TM.ordered(rng, [0, 1, 2], 40001, hi)
        n = t.nrows
        idx = {"repeats": rng.integers(0, n, 5000).repeat(2), "reversed": np.arange(n)[::-1],
               "empty": np.zeros(0, np.int64), "all": np.arange(n)}
        rng_lists = {
            "empties-head-middle-tail": [(5, 5), (0, 2048), (2048, 2048), (4000, 4000), (2048, 20000), (40001, 40001)],
            "overlapping": [(0, 3000), (1000, 5000), (2999, 3001), (0, 3000)],
            "whole": [(0, n)],
            "none": [],
            "descending": [(30000, 40001), (10, 20000), (0, 10)],
            "single-rows": [(i, i + 1) for i in range(0, n, 997)],
        }
        return {"t": t, "idx": idx, "ranges": rng_lists}

    def one(rng, hi):
        t = TM.ordered(rng, [4], 1, hi)
        return {"t": t, "idx": {"repeats": np.zeros(3, np.int64), "reversed": np.zeros(1, np.int64),
                                "empty": np.zeros(0, np.int64)},
                "ranges": {"empties-head-middle-tail": [(0, 0), (0, 1), (1, 1), (0, 1), (1, 1)],
                           "overlapping": [(0, 1), (0, 1)], "whole": [(0, 1)], "none": []}}

    def comp(rng, hi):
        t = TM.composite(rng, [0], [[1, 2]], 130, hi)
        return {"t": t, "idx": {"reversed": np.arange(130)[::-1]}, "ranges": {"overlapping": [(0, 100), (64, 130)]}}
    return _ids([Case("gather-40001x3", big), Case("gather-1x1", one), Case("gather-composite", comp)])


GATHER_CASES = _gather_cases()


# ---------------------------------------------------------------- partition
NPARTS = (1, 2, 3, 64, 4096)
PART_KEYS = ((), (1,), (0, 2))          # () = nkey 0: every column is the key


def _partition_cases():
    # keys of a range about a third of the rows: equal keys exist and must share a block
    return _ids([Case(f"part-n{n}", lambda rng, hi, n=n: {
        "t": TM.ordered(rng, [0, 1, 2], n, min(hi, max(2, n // 3))),
        "other": TM.ordered(rng, [1, 5], max(1, n // 2), min(hi, max(2, n // 3)))}) for n in SIZES])


PARTITION_CASES = _partition_cases()


# -------------------------------------------------------- export / import rows
def _rows_cases():
    return _ids([Case(f"rows-w{w}-n{n}", lambda rng, hi, w=w, n=n: {"t": TM.ordered(rng, range(w), n, hi)})
                 for w in (1, 3, 16) for n in SIZES])


ROWS_CASES = _rows_cases()


# ------------------------------------------------------------ operator sequences
SEQ_OPS = ("join", "antijoin", "dedup", "concat", "set_dedup", "set_minus", "gather", "gather_ranges", "partition")


def seq_start(rng, hi):
    """The tables a sequence starts from: ordered, over few variables and a
    value range small enough that joins produce rows."""
    r = 300
    return [TM.ordered(rng, [0, 1], 3000, r, dup=0.3), TM.ordered(rng, [1, 2], 900, r),
            TM.ordered(rng, [0, 1], 1500, r), TM.ordered(rng, [1], 120, r), TM.ordered(rng, [2, 3], 700, r)]


def join_rows(a, b):
    """Row count of the ordered join of a and b (without building it)."""
    shared = sorted(set(a.vars) & set(b.vars))
    if not shared:
        return a.nrows * b.nrows
    cnt = {}
    for k in map(tuple, b.rows[:, [b.vars.index(v) for v in shared]].tolist()):
        cnt[k] = cnt.get(k, 0) + 1
    return sum(cnt.get(k, 0) for k in map(tuple, a.rows[:, [a.vars.index(v) for v in shared]].tolist()))


def seq_step(rng, pool):
    """One step: (op, operand indices into pool, extra) -- drawn from the rng
    and the pool's schemas, sizes and row multisets only (never the row
    order), so a host-only run and a device run take the same steps.  A step
    whose result would reach SEQ_CAP rows becomes a dedup."""
    op = SEQ_OPS[int(rng.integers(0, len(SEQ_OPS)))]
    i = int(rng.integers(0, len(pool)))
    a = pool[i]
    same = [j for j, t in enumerate(pool) if t.schema == a.schema]
    j = int(rng.integers(0, len(pool)))
    extra = None
    if op in ("concat", "set_dedup", "set_minus"):
        j = same[int(rng.integers(0, len(same)))]
    if (op == "join" and join_rows(a, pool[j]) >= SEQ_CAP) or \
            (op in ("concat", "set_dedup") and a.nrows + pool[j].nrows >= SEQ_CAP):
        op = "dedup"
    if op == "gather":
        kind = int(rng.integers(0, 3))
        n = a.nrows
        extra = (np.arange(n)[::-1] if kind == 0 else rng.integers(0, max(n, 1), min(n, 2000)) if kind == 1
                 else np.sort(rng.integers(0, max(n, 1), min(n, 2000))))
        if n == 0:
            extra = np.zeros(0, np.int64)
    if op == "gather_ranges":
        n = a.nrows
        cuts = np.sort(rng.integers(0, n + 1, 6))
        extra = [(int(cuts[4]), int(cuts[5])), (int(cuts[0]), int(cuts[1])), (int(cuts[2]), int(cuts[2])),
                 (int(cuts[2]), int(cuts[3]))]
        if rng.random() < 0.5:
            extra = sorted(extra)
    if op == "partition":
        extra = (int(rng.integers(1, 9)), (a.vars[0],))
    return op, i, j, extra


def seq_apply(op, a, b, extra):
    """The model's result of one step (a table; for set ops the first table's result)."""
    if op == "join":
        return TM.join(a, b)
    if op == "antijoin":
        return TM.antijoin(a, b)
    if op == "dedup":
        return TM.dedup(a)
    if op == "concat":
        return TM.concat([a, b])
    if op == "set_dedup":
        return TM.concat(TM.set_dedup([a, b]))
    if op == "set_minus":
        return TM.set_minus([a], [b])[0]
    if op == "gather":
        return TM.gather_rows(a, extra)
    if op == "gather_ranges":
        return TM.gather_ranges(a, [x for x, _ in extra], [y for _, y in extra])
    if op == "partition":
        return TM.partition(a, extra[1], extra[0])[0]
    raise AssertionError(op)


# order of the result rows an operator's header promises (else: a multiset)
SEQ_EXACT = {"antijoin", "concat", "set_dedup", "set_minus", "gather", "gather_ranges"}
