"""The bulk steps of notebooks/SimplePatternMiner.ipynb.

`halo` is the notebook's cell 6: around a set of seed atoms, level by level,
every link of arity 2 or 3 that holds a frontier atom (the five '*'-typed
templates [h,*] [*,h] [h,*,*] [*,h,*] [*,*,h]), each link reported at the
first level that finds it, and the targets of those links as the next
frontier.  `pattern_counts` is `build_patterns` (cell 5): the one- and
two-wildcard templates of a set of links, each with
len(get_links(type, None, template)).

`halo_host` / `pattern_counts_host` are those cells restated as loops of
per-call API over any DBInterface (or a facade with get_links): what a caller
had to write before, kept as the definition of the answer and as the path of
`DAS_MINER=0`, of a DB with stale pattern entries and of `ShardedDB`.
`HipDB.halo` / `HipDB.pattern_counts` answer from the resident index instead
(das_halo_expand, das_pattern_counts): one pass over the frontier's incoming
lists per level, one key-range width or equal range per template.

The mining loop (cells c34c1d24 / efac9ac6) is the third step:
`conjunction_counts_host` is its compute_count per And-combination of
templates, `HipDB.conjunction_counts` counts a batch of them from the index
(das_conjunction_counts) and `isurprisingness` adds the notebook's score, the
sub-combinations it needs counted once per batch.

`mine` is the exhaustive cell (efac9ac6) as one call: every basic with every
ascending tuple of candidates, counted, scored and cut to the best rows.
`mine_host` is its definition over `isurprisingness`; `HipDB.mine` enumerates,
counts, scores and selects on the device (das_mine_combinations).
"""
import itertools
import time

import numpy as np

from . import _lib
from .database.db_interface import UNORDERED_LINK_TYPES, WILDCARD
from .expression_hasher import ExpressionHasher

DAS_NONE = _lib.DAS_NONE


def halo_templates(h):
    """SimplePatternMiner.ipynb cell 6."""
    return [[h, WILDCARD], [WILDCARD, h], [h, WILDCARD, WILDCARD], [WILDCARD, h, WILDCARD], [WILDCARD, WILDCARD, h]]


def pattern_templates(link_type, targets):
    """build_patterns' templates of one link (cell 5): arity 2 -> 2, arity 3
    -> 6 (the all-wildcard one is commented out there), else none."""
    if len(targets) == 2:
        return [[link_type, WILDCARD, targets[1]], [link_type, targets[0], WILDCARD]]
    if len(targets) == 3:
        t0, t1, t2 = targets
        return [[link_type, WILDCARD, t1, t2], [link_type, t0, WILDCARD, t2], [link_type, t0, t1, WILDCARD],
                [link_type, WILDCARD, WILDCARD, t2], [link_type, WILDCARD, t1, WILDCARD],
                [link_type, t0, WILDCARD, WILDCARD]]
    return []


def _links_of(db, link_type, targets):
    """das.get_links(link_type, None, targets) in HANDLE format over a facade
    or a DBInterface."""
    if hasattr(db, "get_links"):
        return db.get_links(link_type, None, targets)
    link_type = WILDCARD if link_type is None else link_type
    if hasattr(db, "get_matched_link_handles"):
        return db.get_matched_link_handles(link_type, targets)
    return [a if isinstance(a, str) else a[0] for a in db.get_matched_links(link_type, targets)]


def _exists(db, handle):
    if hasattr(db, "_lookup"):
        return db._lookup(handle)[0] >= 0
    for probe in (db.get_node_name, db.get_link_targets):
        try:
            probe(handle)
            return True
        except Exception:
            pass
    return False


class _Levels:
    """Per-level id arrays of a device halo, copied to the host on first use."""

    def __init__(self, tables):
        self._tables = tables
        self._host = [None] * len(tables)

    def __len__(self):
        return len(self._tables)

    def __getitem__(self, level):
        if isinstance(level, slice):
            return [self[i] for i in range(*level.indices(len(self)))]
        if self._host[level] is None:
            self._host[level] = np.ascontiguousarray(self._tables[level].fetch()[0])
        return self._host[level]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class HaloLevel:
    """The links of one level of a Halo: `.ids`, `.handles`, and `.table` (the
    device table of a device halo: pattern_counts reads it in place)."""

    def __init__(self, halo, level):
        self.halo, self.level = halo, level

    @property
    def table(self):
        return self.halo._link_tables[self.level] if self.halo._link_tables is not None else None

    @property
    def ids(self):
        return self.halo.links[self.level]

    @property
    def handles(self):
        return self.halo.link_handles(self.level)

    def __len__(self):
        t = self.table
        return int(t.nrows) if t is not None else len(self.ids)


class Halo:
    """`.links[level]`: the links first found at that level; `.atoms[level]`:
    the atoms first reached through them (the next level's frontier).  Over a
    DB with atom ids (HipDB) both are numpy id arrays in ascending order and
    the handles are made on demand (`link_handles`, `atom_handles`); over any
    other DBInterface they are sorted arrays of handles."""

    def __init__(self, db, links, atoms, link_tables=None, by_id=True):
        self.db = db
        self.links = links
        self.atoms = atoms
        self.by_id = by_id
        self._link_tables = link_tables
        self.stopped = None          # halo_host with a time budget that ran out: where it stopped
        self._lh = {}
        self._ah = {}

    def __len__(self):
        return len(self.links)

    def level(self, level):
        return HaloLevel(self, level)

    def _hex(self, cache, arrays, level):
        if level not in cache:
            a = arrays[level]
            cache[level] = (self.db.hex_of(a) if len(a) else []) if self.by_id else [str(h) for h in a]
        return cache[level]

    def link_handles(self, level):
        return self._hex(self._lh, self.links, level)

    def atom_handles(self, level):
        return self._hex(self._ah, self.atoms, level)

    @property
    def universe_size(self):
        if self._link_tables is not None:
            return sum(int(t.nrows) for t in self._link_tables)
        return sum(len(a) for a in self.links)


def halo_host(db, seeds, length=2, budget_s=None):
    """Cell 6 through per-call API: get_links('*', None, t) for the five
    templates of every frontier atom, get_link_targets of every link found.
    Only the atoms not expanded before are expanded at a level: expanding an
    old one again finds the links it found then, which the notebook's
    `difference(all_links)` drops again.  budget_s: stop after that many
    seconds; `.stopped` of the result then says where (level, phase, done,
    of) and the last level is incomplete (measurement tools only)."""
    length = int(length)
    if length < 0:
        raise ValueError("halo: negative length")
    t0 = time.perf_counter()
    frontier = [h for h in dict.fromkeys(seeds) if _exists(db, h)]
    expanded = set(frontier)
    all_links = set()
    links, atoms = [], []
    stopped = None
    for lv in range(length):
        found = set()
        for k, h in enumerate(frontier):
            if budget_s is not None and time.perf_counter() - t0 > budget_s:
                stopped = {"level": lv, "phase": "get_links", "done": k, "of": len(frontier)}
                break
            for template in halo_templates(h):
                found.update(_links_of(db, None, template))
        new_links = found.difference(all_links)
        all_links.update(new_links)
        reached = set()
        for k, link in enumerate(new_links):
            if stopped is None and budget_s is not None and k % 64 == 0 and time.perf_counter() - t0 > budget_s:
                stopped = {"level": lv, "phase": "get_link_targets", "done": k, "of": len(new_links)}
            if stopped is not None:
                break
            reached.update(db.get_link_targets(link))
        reached.difference_update(expanded)
        expanded.update(reached)
        links.append(new_links)
        atoms.append(reached)
        if stopped is not None:
            break
        frontier = sorted(reached)
    if hasattr(db, "ids_of") and hasattr(db, "hex_of"):
        def ids(hs):
            return np.sort(np.asarray(db.ids_of(list(hs)), dtype=np.int64)).astype(np.uint32)
        out = Halo(db, [ids(x) for x in links], [ids(x) for x in atoms])
    else:
        out = Halo(db, [np.array(sorted(x), dtype=object) for x in links],
                   [np.array(sorted(x), dtype=object) for x in atoms], by_id=False)
    out.stopped = stopped
    return out


class PatternCounts:
    """The distinct templates of a set of links with their support.  Over a
    DB with atom ids the columns are `arity`, `type_id`, `targets` (m x 3,
    DAS_NONE = wildcard or unused) and `count` (uint64), ordered by (arity,
    type id, targets); `template(i)` is [type name, handle | '*', ...]."""

    def __init__(self, db, arity, type_id, targets, count, templates=None):
        self.db = db
        self.arity = arity
        self.type_id = type_id
        self.targets = targets
        self.count = count
        self.stopped = None          # pattern_counts_host with a time budget that ran out
        self._templates = templates

    def __len__(self):
        return len(self.count)

    def templates(self):
        if self._templates is None:
            m = len(self)
            tg = self.targets
            grounded = tg != DAS_NONE
            hexes = iter(self.db.hex_of(tg[grounded])) if grounded.any() else iter(())
            names = self.db.arrays.type_names
            out = []
            for i in range(m):
                row = [names[int(self.type_id[i])]]
                for p in range(int(self.arity[i])):
                    row.append(next(hexes) if grounded[i, p] else WILDCARD)
                out.append(row)
            self._templates = out
        return self._templates

    def template(self, i):
        return list(self.templates()[i])

    def handle(self, i):
        return ExpressionHasher.composite_hash(self.template(i))

    def pattern(self, i):
        """The Link build_pattern_from_template makes of template i."""
        from .pattern_matcher.pattern_matcher import Link, Node, Variable
        t = self.template(i)
        targets, k = [], 1
        for h in t[1:]:
            if h == WILDCARD:
                targets.append(Variable(f"V{k}"))
                k += 1
            else:
                targets.append(Node(self.db.get_node_type(h), self.db.get_node_name(h)))
        return Link(t[0], targets, t[0] not in UNORDERED_LINK_TYPES)

    def as_dict(self):
        return {ExpressionHasher.composite_hash(t): int(c) for t, c in zip(self.templates(), self.count)}


def _link_handles(db, links):
    """Handles of `links`: handles, an id array, a Halo level."""
    if isinstance(links, HaloLevel):
        return links.handles
    if isinstance(links, np.ndarray) and links.dtype != object:
        return db.hex_of(links) if links.size else []
    return [str(h) for h in links]


def pattern_counts_host(db, links, budget_s=None):
    """build_patterns through per-call API: per link get_link_targets and
    get_link_type, per template get_node_type / get_node_name of the grounded
    targets (a failure drops the template) and len(get_links(...)).
    budget_s: stop after that many seconds; `.stopped` = (links done, of)."""
    counts = {}
    t0 = time.perf_counter()
    stopped = None
    todo = list(dict.fromkeys(_link_handles(db, links)))
    for k, link in enumerate(todo):
        if budget_s is not None and time.perf_counter() - t0 > budget_s:
            stopped = {"done": k, "of": len(todo)}
            break
        targets = db.get_link_targets(link)
        link_type = db.get_link_type(link)
        for template in pattern_templates(link_type, list(targets)):
            key = tuple(template)
            if key in counts:
                continue
            try:
                for t in template[1:]:
                    if t != WILDCARD:
                        db.get_node_type(t)
                        db.get_node_name(t)
            except Exception:
                continue
            counts[key] = len(_links_of(db, template[0], template[1:]))
    keys = list(counts)
    if hasattr(db, "ids_of") and hasattr(db, "type_id"):
        grounded = list(dict.fromkeys(t for k in keys for t in k[1:] if t != WILDCARD))
        ids = dict(zip(grounded, np.asarray(db.ids_of(grounded)).tolist())) if grounded else {}
        rows = []
        for k in keys:
            tg = [ids[t] if t != WILDCARD else DAS_NONE for t in k[1:]]
            rows.append((len(k) - 1, db.type_id[k[0]], *(tg + [DAS_NONE] * (3 - len(tg))), counts[k], k))
        rows.sort(key=lambda r: r[:5])
        cols = np.array([r[:5] for r in rows], dtype=np.uint32).reshape(len(rows), 5)
        out = PatternCounts(db, cols[:, 0].copy(), cols[:, 1].copy(), cols[:, 2:5].copy(),
                            np.array([r[5] for r in rows], dtype=np.uint64), [list(r[6]) for r in rows])
    else:
        keys.sort(key=lambda k: (len(k), k))
        out = PatternCounts(db, np.array([len(k) - 1 for k in keys], dtype=np.uint32), None, None,
                            np.array([counts[k] for k in keys], dtype=np.uint64), [list(k) for k in keys])
    out.stopped = stopped
    return out


# ---------------------------------------------------------------------------
# the mining loop (cells c34c1d24 / efac9ac6): counts of And-combinations of
# templates and their I-surprisingness
# ---------------------------------------------------------------------------

def check_combos(combos, m):
    """`combos` as an (n, k) uint32 array of row indices into a PatternCounts
    of m templates.  ValueError: k outside 2..4, rows of unequal length, an
    index that is negative or >= m."""
    try:
        a = np.asarray(combos if isinstance(combos, np.ndarray) else list(combos))
    except ValueError as e:                       # numpy refuses ragged rows
        raise ValueError("conjunction counts: combinations of unequal length") from e
    if a.dtype == object:
        raise ValueError("conjunction counts: combinations of unequal length")
    if a.ndim == 1 and a.size == 0:               # no combination at all
        a = np.zeros((0, 2), dtype=np.int64)
    if a.ndim != 2 or not 2 <= a.shape[1] <= 4:
        raise ValueError("conjunction counts: combinations are rows of 2 to 4 template indices")
    if a.dtype.kind not in "iu":
        raise ValueError("conjunction counts: template indices are integers")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= m):
        raise ValueError("conjunction counts: template index out of range")
    return np.ascontiguousarray(a, dtype=np.uint32)


def build_composite_pattern(terms):
    """The notebook's fold: And([And([t0, t1]), t2]) ..."""
    from .pattern_matcher.pattern_matcher import And
    assert len(terms) > 1
    first = terms[0]
    for second in terms[1:]:
        first = And([first, second])
    return first


class HostCounts(np.ndarray):
    """conjunction_counts_host's counts; `.stopped` = {done, of} if its time
    budget ran out (the rows from `done` on are then 0)."""
    stopped = None


def conjunction_counts_host(db, pc, combos, budget_s=None):
    """compute_count(build_composite_pattern([pc.pattern(i) for i in combo]))
    per combination: one matched() each, answer.count() rows, 0 where it is
    false.  The definition of the answer, and the path of DAS_MINER=0, of a
    DB with stale pattern entries, of CONFIG['no_overload'], of Similarity /
    Set templates and of any DB without atom ids.  budget_s: stop after that
    many seconds (`.stopped`; measurement tools only)."""
    from .pattern_matcher.pattern_matcher import PatternMatchingAnswer
    combos = check_combos(combos, len(pc))
    out = np.zeros(len(combos), dtype=np.uint64).view(HostCounts)
    patterns = {}
    t0 = time.perf_counter()
    for c, combo in enumerate(combos.tolist()):
        if budget_s is not None and time.perf_counter() - t0 > budget_s:
            out.stopped = {"done": c, "of": len(combos)}
            break
        for i in combo:
            if i not in patterns:
                patterns[i] = pc.pattern(i)
        answer = PatternMatchingAnswer()
        if build_composite_pattern([patterns[i] for i in combo]).matched(db, answer):
            out[c] = answer.count()
    return out


_SUBSETS = {k: {s: list(itertools.combinations(range(k), s)) for s in range(2, k)} for k in (2, 3, 4)}


def sub_combinations(combos):
    """The proper sub-combinations compute_isurprisingness counts, merged
    over the batch: {size: (distinct, where)} with `distinct` the (u, size)
    sorted index rows, each once, and where[c, j] the row of `distinct` that
    is subset j of combination c, the subsets in itertools.combinations order
    of the positions.  k = 2: none; 3: the three pairs; 4: six pairs and four
    triples.  An index twice in a combination stays twice in its subsets."""
    combos = np.asarray(combos)
    n, k = combos.shape
    out = {}
    for size, subsets in _SUBSETS[k].items():
        rows = np.sort(np.stack([combos[:, list(s)] for s in subsets], axis=1).reshape(n * len(subsets), size), axis=1)
        if len(rows):
            distinct, where = np.unique(rows, axis=0, return_inverse=True)
        else:
            distinct, where = rows, np.zeros(0, dtype=np.int64)
        out[size] = (distinct.astype(np.uint32), where.reshape(n, len(subsets)))
    return out


def isurprisingness_from_counts(count, term_counts, universe_size, pair_counts=None, triple_counts=None,
                                normalized=False):
    """compute_isurprisingness over arrays, in float64 and in the notebook's
    order of operations.  count: (n,) the combinations' counts; term_counts:
    (n, k) the terms' own counts; pair_counts: (n, C(k, 2)) the counts of the
    pairs (0,1) (0,2) .. in itertools.combinations order (k >= 3);
    triple_counts: (n, 4) of (0,1,2) (0,1,3) (0,2,3) (1,2,3) (k = 4), as
    the notebook counts them: with a flat three-term And (`flat_triple_counts`).
    normalized divides by prob(count): where the count is 0 the notebook
    raises ZeroDivisionError; the value here is nan."""
    u = float(universe_size)

    def prob(x):
        return np.asarray(x, dtype=np.float64) / u

    t = prob(term_counts)
    k = t.shape[1]
    if k == 2:
        subset_probs = [t[:, 0] * t[:, 1]]
    elif k == 3:
        p = prob(pair_counts)                       # (0,1) (0,2) (1,2)
        subset_probs = [t[:, 0] * t[:, 1] * t[:, 2], p[:, 0] * t[:, 2], p[:, 1] * t[:, 1], p[:, 2] * t[:, 0]]
    elif k == 4:
        p = prob(pair_counts)                       # (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        q = prob(triple_counts)                     # (0,1,2) (0,1,3) (0,2,3) (1,2,3)
        subset_probs = [t[:, 0] * t[:, 1] * t[:, 2] * t[:, 3], p[:, 0] * p[:, 5], p[:, 1] * p[:, 4],
                        p[:, 2] * p[:, 3], q[:, 0] * t[:, 3], q[:, 1] * t[:, 2], q[:, 2] * t[:, 1], q[:, 3] * t[:, 0]]
    else:
        raise NotImplementedError()
    sp = np.stack(subset_probs, axis=1)
    pc = prob(count)
    value = np.maximum(pc - sp.max(axis=1), sp.min(axis=1) - pc)
    if normalized:
        with np.errstate(divide="ignore", invalid="ignore"):
            value = np.where(pc > 0, value / pc, np.nan)
    return value


def flat_triple_counts(term_counts, pair_counts, triple_counts):
    """The four triples of a 4-combination as compute_isurprisingness counts
    them.  It asks `And([ti, tj, tl])`, one flat And, not the nested fold of
    build_composite_pattern, and the reference's And starts over from the
    next term once its running join is empty (pattern_matcher.py:717-729):
    false, count 0, if a term has no rows; the third term's own count if the
    first two join to nothing; else the size of the join of the three.  The
    order of the terms matters, so this is derived per combination from
    counts that do not depend on it: term_counts (n, 4), pair_counts (n, 6)
    and triple_counts (n, 4), the join sizes in itertools.combinations order
    of the positions."""
    t = np.asarray(term_counts, dtype=np.uint64)
    p = np.asarray(pair_counts, dtype=np.uint64)
    out = np.array(triple_counts, dtype=np.uint64)
    pairs = _SUBSETS[4][2]
    for j, (a, b, c) in enumerate(_SUBSETS[4][3]):
        restart = p[:, pairs.index((a, b))] == 0
        out[restart, j] = t[restart, c]
        out[(t[:, a] == 0) | (t[:, b] == 0) | (t[:, c] == 0), j] = 0
    return out


class ISurprisingness:
    """`.count` (uint64) and `.value` (float64) per combination."""

    def __init__(self, count, value):
        self.count = count
        self.value = value

    def __len__(self):
        return len(self.count)


def isurprisingness(db, pc, combos, universe_size, normalized=False):
    """The mining loop's count and compute_isurprisingness of every
    combination (rows of 2 to 4 indices into `pc`): the combinations and
    their merged sub-combinations (`sub_combinations`) are counted with one
    conjunction_counts call per size, the terms' own counts are pc.count.
    The notebook counts the triples of a 4-combination with a flat And,
    which is not the join of the three where the first two join to nothing:
    `flat_triple_counts` turns the join sizes into what it gets.
    normalized=True with count 0 gives nan (the notebook divides by zero)."""
    combos = check_combos(combos, len(pc))

    def counts_of(rows):
        if hasattr(db, "conjunction_counts"):
            return np.asarray(db.conjunction_counts(pc, rows), dtype=np.uint64)
        return np.asarray(conjunction_counts_host(db, pc, rows), dtype=np.uint64)

    count = counts_of(combos)
    sub = {}
    for size, (distinct, where) in sub_combinations(combos).items():
        sub[size] = counts_of(distinct)[where] if len(distinct) else np.zeros(where.shape, dtype=np.uint64)
    terms = np.asarray(pc.count)[combos.astype(np.int64)]
    if 3 in sub:
        sub[3] = flat_triple_counts(terms, sub[2], sub[3])
    value = isurprisingness_from_counts(count, terms, universe_size, sub.get(2), sub.get(3), normalized)
    return ISurprisingness(count, value)


# ---------------------------------------------------------------------------
# the exhaustive cell (efac9ac6) as one call
# ---------------------------------------------------------------------------

MINE_MAX_TOP = _lib.MX_MAX_TOP


class MiningResult:
    """The best rows of a `mine` call, by value descending (ties in
    enumeration order): `.combos` (r, ngram) uint32 row indices into `.pc`,
    the basic first; `.count` uint64; `.value` float64; `.searched`, the rows
    of the search space; `.scored`, the combinations the path counted;
    `.tiles` (device path); `.pattern(i)`, the composite pattern of row i,
    ready for das.query.  `.stopped`: mine_host with a time budget that ran
    out (measurement tools only)."""

    def __init__(self, pc, combos, count, value, searched, scored, tiles=0):
        self.pc = pc
        self.combos = combos
        self.count = count
        self.value = value
        self.searched = int(searched)
        self.scored = int(scored)
        self.tiles = int(tiles)
        self.stopped = None

    def __len__(self):
        return len(self.count)

    def pattern(self, i):
        return build_composite_pattern([self.pc.pattern(int(j)) for j in self.combos[i]])


def _index_list(values, m, what):
    a = np.asarray(values if isinstance(values, np.ndarray) else list(values))
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"mine: {what} are a list of template indices")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= m:
        raise ValueError(f"mine: a template index of the {what} is out of range")
    if len(np.unique(a)) != len(a):
        raise ValueError(f"mine: the {what} are distinct")
    return a


def check_mine_args(pc, basics, universe_size, ngram, support, top, candidates):
    """(basics in the order given, candidates ascending) as int64 arrays.
    ValueError: ngram outside {2, 3}, an index out of range or twice, top
    outside 1..MINE_MAX_TOP, a universe size or support that is not a count."""
    if ngram not in (2, 3):
        raise ValueError("mine: ngram outside {2, 3}")
    basics = _index_list(basics, len(pc), "basics")
    candidates = np.arange(len(pc), dtype=np.int64) if candidates is None else \
        np.sort(_index_list(candidates, len(pc), "candidates"))
    if not isinstance(top, (int, np.integer)) or not 1 <= top <= MINE_MAX_TOP:
        raise ValueError(f"mine: top outside 1..{MINE_MAX_TOP}")
    if not universe_size > 0:
        raise ValueError("mine: universe size 0")
    if support < 0:
        raise ValueError("mine: negative support")
    return basics, candidates


def search_space_size(basics, candidates, ngram):
    """Rows of the search space: per basic the (ngram - 1)-subsets of the
    candidates other than itself."""
    total = 0
    for own in np.isin(basics, candidates).tolist():
        av = len(candidates) - int(own)
        total += av if ngram == 2 else av * (av - 1) // 2
    return total


def _keep_best(kept, new, top):
    """kept + new (tuples of combos, count, value; kept's rows enumerated
    first), stable by value descending, cut to top."""
    combos, count, value = (np.concatenate([a, b]) for a, b in zip(kept, new))
    order = np.argsort(-value, kind="stable")[:top]
    return combos[order], count[order], value[order]


def mine_host(db, pc, basics, universe_size, ngram=3, support=0, normalized=False, top=16, candidates=None,
              max_combinations=2**32, batch=1 << 15, budget_s=None):
    """The definition of `mine`: for each basic, in the order given, every
    strictly ascending (ngram - 1)-tuple of candidates that does not hold it,
    as the row (b, c1[, c2]); count and value of each row from
    `isurprisingness`, `batch` rows at a time; the rows with count >= support
    and value > 0 by value descending, ties in enumeration order, cut to
    `top`.  ValueError if the space has more than max_combinations rows.
    budget_s: stop after that many seconds (`.stopped` = {done, of})."""
    basics, candidates = check_mine_args(pc, basics, universe_size, ngram, support, top, candidates)
    searched = search_space_size(basics, candidates, ngram)
    if searched > max_combinations:
        raise ValueError(f"mine: {searched} combinations to score, more than max_combinations")
    kept = (np.zeros((0, ngram), dtype=np.uint32), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float64))
    t0 = time.perf_counter()
    done, stopped = 0, None

    def rows_of():
        for b in basics.tolist():
            for tup in itertools.combinations([c for c in candidates.tolist() if c != b], ngram - 1):
                yield (b, *tup)

    rows = rows_of()
    while stopped is None:
        chunk = np.array(list(itertools.islice(rows, batch)), dtype=np.uint32).reshape(-1, ngram)
        if not len(chunk):
            break
        if budget_s is not None and time.perf_counter() - t0 > budget_s:
            stopped = {"done": done, "of": searched}
            break
        res = isurprisingness(db, pc, chunk, universe_size, normalized)
        with np.errstate(invalid="ignore"):
            ok = (res.value > 0) & (res.count >= support)
        if ok.any():
            kept = _keep_best(kept, (chunk[ok], np.asarray(res.count)[ok], np.asarray(res.value)[ok]), top)
        done += len(chunk)
    out = MiningResult(pc, *kept, searched, done)
    out.stopped = stopped
    return out


def mine(db, pc, basics, universe_size, ngram=3, support=0, normalized=False, top=16, candidates=None,
         max_combinations=2**32):
    """The notebook's exhaustive cell as one call: the best `top` patterns
    And(b, c1[, c2]) over every basic b and every ascending tuple of
    candidates (default: every template of `pc`), a MiningResult; with top=1
    its row is the notebook's best_pattern.  A HipDB enumerates, counts,
    scores and selects on the device (`HipDB.mine`); any other DB runs
    `mine_host`."""
    if hasattr(db, "mine"):
        return db.mine(pc, basics, universe_size, ngram=ngram, support=support, normalized=normalized, top=top,
                       candidates=candidates, max_combinations=max_combinations)
    return mine_host(db, pc, basics, universe_size, ngram, support, normalized, top, candidates, max_combinations)
