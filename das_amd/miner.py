"""The two bulk steps of notebooks/SimplePatternMiner.ipynb.

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
"""
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
