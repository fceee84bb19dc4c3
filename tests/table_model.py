"""Host model of the binding-table operators (query.hip, composite.hip) and
the input generators of the tests that put it next to them.

The model is built on the oracle's row algebra (O.join, O.check_negation,
O.ident); test_parallel_gloo.py's NumpyLocal evaluates with it, and
test_gpu_table_ops.py compares every device operator against it.  No tests
in this module."""
import numpy as np

from oracle import das_oracle as O

ORDERED, UNORDERED, COMPOSITE = 0, 1, 2


class NTable:
    def __init__(self, kind, vars_, rows, members=None):
        self.kind = kind
        self.vars = tuple(vars_)
        self.members = tuple(members) if kind == COMPOSITE else None
        self.rows = np.asarray(rows, dtype=np.uint32).reshape(-1, len(vars_))

    @property
    def nrows(self):
        return self.rows.shape[0]

    @property
    def schema(self):
        return (self.kind, self.vars, self.members)

    def fetch(self):
        return self.rows.T.copy()


# ---- composite rows <-> the oracle's row model (ints as variables and values)
def _parts(t):
    """(ordered var list or None, [member var lists]) of a table schema."""
    if t.kind == ORDERED:
        return list(t.vars), []
    if t.kind == UNORDERED:
        return None, [list(t.vars)]
    o = [v for v, m in zip(t.vars, t.members) if m < 0]
    mem = {}
    for v, m in zip(t.vars, t.members):
        if m >= 0:
            mem.setdefault(m, []).append(v)
    return (o or None), [mem[m] for m in sorted(mem)]


def _to_oracle(t, r):
    r = [int(x) for x in r]
    if t.kind == ORDERED:
        return O.o_row(dict(zip(t.vars, r)))
    if t.kind == UNORDERED:
        return O.u_row(t.vars, r)
    o, mems = _parts(t)
    k = len(o) if o else 0
    orow = O.o_row(dict(zip(o, r[:k]))) if o else None
    us = []
    for mv in mems:
        us.append(O.u_row(mv, r[k:k + len(mv)]))
        k += len(mv)
    return ("C", orow, us)


def _join_schema(a, b):
    """Output schema of the CompositeAssignment join (composite.hip)."""
    if a.kind == ORDERED or (a.kind == UNORDERED and b.kind == COMPOSITE):
        x, y = b, a
    else:
        x, y = a, b
    xo, xm = _parts(x)
    yo, ym = _parts(y)
    o = set(xo or [])
    if y.kind != UNORDERED and not (xo and not yo):
        o |= set(yo or [])
    mems = xm + (ym if y.kind != ORDERED else [])
    vars_ = sorted(o) + [v for m in mems for v in m]
    members = [-1] * len(o) + [i for i, m in enumerate(mems) for _ in m]
    return vars_, members


def _from_oracle(vars_, members, rows):
    out = []
    for r in rows:
        vals = dict(r[1][1]) if r[1] is not None else {}
        line = [vals[v] for v, m in zip(vars_, members) if m < 0]
        for u in r[2]:
            line += list(u[2])
        out.append(line)
    return NTable(COMPOSITE, vars_, np.array(out, np.uint32).reshape(-1, len(vars_)), members)


# ---- the table operators
def partition(t, key_vars, nparts):
    cols = [t.vars.index(v) for v in key_vars] if key_vars else list(range(len(t.vars)))
    h = np.zeros(t.nrows, dtype=np.uint64)
    for c in cols:
        h = h * np.uint64(1000003) + t.rows[:, c].astype(np.uint64)
    dest = (h % np.uint64(nparts)).astype(np.int64)
    order = np.argsort(dest, kind="stable")
    counts = np.bincount(dest, minlength=nparts).astype(np.uint64)
    return NTable(t.kind, t.vars, t.rows[order], t.members), counts


def dedup(t):
    if t.nrows == 0:
        return t
    if t.kind == COMPOSITE:
        # das_dedup of a composite table is set_dedup of it alone (query.hip dedup())
        return set_dedup([t])[0]
    return NTable(t.kind, t.vars, np.unique(t.rows, axis=0))


def concat(ts):
    return NTable(ts[0].kind, ts[0].vars, np.concatenate([t.rows for t in ts]), ts[0].members)


def set_dedup(ts):
    seen, out = set(), []
    for t in ts:
        keep = []
        for r in t.rows:
            k = O.ident(_to_oracle(t, r))
            if k not in seen:
                seen.add(k)
                keep.append(r)
        out.append(NTable(t.kind, t.vars, np.array(keep, np.uint32).reshape(-1, len(t.vars)), t.members))
    return out


def set_minus(a, b):
    gone = {O.ident(_to_oracle(t, r)) for t in b for r in t.rows}
    return [NTable(t.kind, t.vars, np.array([r for r in t.rows if O.ident(_to_oracle(t, r)) not in gone],
                                            np.uint32).reshape(-1, len(t.vars)), t.members) for t in a]


def gather_rows(t, idx):
    return NTable(t.kind, t.vars, t.rows[np.asarray(idx, dtype=np.int64)], t.members)


def gather_ranges(t, begin, end):
    idx = [np.arange(int(b), int(e)) for b, e in zip(begin, end)]
    return gather_rows(t, np.concatenate(idx) if idx else np.zeros(0, np.int64))


def join(a, b, no_overload=False):
    if a.kind != ORDERED or b.kind != ORDERED:
        vars_, members = _join_schema(a, b)
        rb = [_to_oracle(b, r) for r in b.rows]
        was = O.CONFIG["no_overload"]
        O.CONFIG["no_overload"] = bool(no_overload)
        try:
            out = [j for r in a.rows for y in rb for j in [O.join(_to_oracle(a, r), y)] if j is not None]
        finally:
            O.CONFIG["no_overload"] = was
        return _from_oracle(vars_, members, out)
    shared = sorted(set(a.vars) & set(b.vars))
    uni = sorted(set(a.vars) | set(b.vars))
    ka = [a.vars.index(v) for v in shared]
    kb = [b.vars.index(v) for v in shared]
    # output column -> (from b?, source column); a shared variable's two values are equal
    src = [(True, b.vars.index(v)) if v in b.vars else (False, a.vars.index(v)) for v in uni]
    idx = {}
    for s in b.rows.tolist():
        idx.setdefault(tuple(s[c] for c in kb), []).append(s)
    out = []
    for r in a.rows.tolist():
        for s in idx.get(tuple(r[c] for c in ka), ()):
            out.append([s[c] if fb else r[c] for fb, c in src])
    # no_overload: where neither side's variables cover the other's, the
    # reference re-assigns every value and rejects a repeated one
    # (_join_ordered's NO_COVERING branch; k_overload_flags in query.hip);
    # a covering join returns an operand's rows as they are
    if no_overload and not (set(a.vars) <= set(b.vars) or set(b.vars) <= set(a.vars)):
        out = [r for r in out if len(set(int(x) for x in r)) == len(r)]
    return NTable(ORDERED, uni, np.array(out, np.uint32).reshape(-1, len(uni)))


def antijoin(a, t):
    if a.kind != ORDERED or t.kind != ORDERED:
        rt = [_to_oracle(t, r) for r in t.rows]
        keep = [r for r in a.rows if all(O.check_negation(_to_oracle(a, r), x) for x in rt)]
        return NTable(a.kind, a.vars, np.array(keep, np.uint32).reshape(-1, len(a.vars)), a.members)
    if not set(t.vars) <= set(a.vars):
        return a
    bad = {tuple(r) for r in t.rows}
    keep = [r for r in a.rows if tuple(r[a.vars.index(v)] for v in t.vars) not in bad]
    return NTable(a.kind, a.vars, np.array(keep, np.uint32).reshape(-1, len(a.vars)))


# ---- input generators (every value below `hi`; hi <= the context's n_atoms:
# the device sort paths sort id_bits(ctx) bits only, values are atom ids)
def ordered(rng, vars_, n, hi, dup=0.0):
    """ORDERED table of n rows over the sorted variables, values uniform in
    [0, hi); `dup`: the share of rows that repeat an earlier row (1: all rows
    equal the first)."""
    vars_ = sorted(vars_)
    rows = rng.integers(0, hi, size=(n, len(vars_)), dtype=np.int64)
    if n > 1 and dup > 0:
        if dup >= 1:
            rows[:] = rows[0]
        else:
            where = np.sort(rng.choice(np.arange(1, n), size=min(int(dup * n), n - 1), replace=False))
            for i in where:
                rows[i] = rows[rng.integers(0, i)]
    return NTable(ORDERED, vars_, rows)


def _distinct_sorted(rng, n, k, hi):
    """n rows of k distinct values of [0, hi), each row ascending."""
    assert k <= hi
    rows = np.zeros((n, k), dtype=np.int64)
    for i in range(n):
        rows[i] = np.sort(rng.choice(hi, size=k, replace=False))
    return rows


def unordered(rng, vars_, n, hi):
    """UNORDERED table (one member): each row's values distinct and ascending,
    the layout composite.hip's header requires."""
    vars_ = sorted(vars_)
    return NTable(UNORDERED, vars_, _distinct_sorted(rng, n, len(vars_), hi))


def composite(rng, ovars, members, n, hi):
    """COMPOSITE table: the ordered columns first (sorted by variable), then
    each member as its sorted variable ids with ascending values; its
    `members` array is the one das_table_from_host takes (-1 for an ordered
    column, else the member's index)."""
    ovars = sorted(ovars)
    members = [sorted(m) for m in members]
    parts = [rng.integers(0, hi, size=(n, len(ovars)), dtype=np.int64)]
    parts += [_distinct_sorted(rng, n, len(m), hi) for m in members]
    vars_ = ovars + [v for m in members for v in m]
    mem = [-1] * len(ovars) + [i for i, m in enumerate(members) for _ in m]
    return NTable(COMPOSITE, vars_, np.concatenate(parts, axis=1), mem)


def to_device(ctx, t):
    """NTable -> _lib.Table on the context."""
    return ctx.table_from_host(t.kind, list(t.vars), t.fetch(), list(t.members) if t.kind == COMPOSITE else None)


def from_device(T):
    """_lib.Table -> NTable (one fetch)."""
    return NTable(T.kind, T.vars, T.fetch().T, T.members)
