"""Pattern matcher with the reference's API (das/pattern_matcher/pattern_matcher.py).

Same classes, constructor signatures and `matched(db, answer) -> bool`
contract; `answer.assignments` is the reference's set of `Assignment`
objects.  Evaluation is different: every term produces a *device* binding
relation (HipDB.match_link / match_template -> scan kernels), `And` folds
them with GPU natural joins and anti-joins, `Or` with GPU union/dedup and set
difference.  Python `Assignment` objects are only built when a caller reads
`answer.assignments`.

Semantics kept from the reference: reset-on-empty in
And (:725-729), skipped empty terms (:717-719), negated terms collected as a
forbidden set (:720-724, :741-746), Or with Not terms = And(negated) minus the
positive union with negation=True (:674-683), top-level Not flips the flag
(:627-631), `_typed_variable_matched` last-writer-wins (:491-500).

All assignment kinds are evaluated on the GPU: ordered natural joins, and
for unordered (Similarity/Set) operands the reference's Unordered /
CompositeAssignment algebra (:158-368: containment / coverage /
compatibility checks, XOR set identity), das_amd/csrc/composite.hip.
"""
import gc
import os
import re
import struct
from abc import ABC, abstractmethod
from collections import Counter
from copy import deepcopy
from enum import Enum, auto
from functools import cmp_to_key
from typing import Dict, FrozenSet, List, Optional, Set, Union

import numpy as np

from .. import _lib
from ..database.db_interface import UNORDERED_LINK_TYPES, WILDCARD, DBInterface
from ..database.hip_db import HipDB, Relation, RelationalDB

DEBUG_AND = False
DEBUG_OR = False
DEBUG_NOT = False
DEBUG_LINK = False
DEBUG_LINK_TEMPLATE = False

CONFIG = {
    'no_overload': False,   # distinct variables must take distinct values (ordered)
}


class CompatibilityStatus(int, Enum):
    INCOMPATIBLE = auto()
    NO_COVERING = auto()
    FIRST_COVERS_SECOND = auto()
    SECOND_COVERS_FIRST = auto()
    EQUAL = auto()


# ---------------------------------------------------------------------------
# variable ids (device tables carry small integer variable ids)
# ---------------------------------------------------------------------------
_VAR_ID: Dict[str, int] = {}
_VAR_NAME: List[str] = []


def _vid(name: str) -> int:
    v = _VAR_ID.get(name)
    if v is None:
        v = len(_VAR_NAME)
        _VAR_ID[name] = v
        _VAR_NAME.append(name)
    return v


def _var_name(v: int) -> str:
    return _VAR_NAME[v]


# ---------------------------------------------------------------------------
# Assignments: the reference's value objects (identity = hash equality)
# ---------------------------------------------------------------------------
class Assignment(ABC):

    def __init__(self):
        self.variables: Union[Set[str], FrozenSet] = set()
        self.hash: int = 0
        self.frozen = False

    def __hash__(self) -> int:
        assert self.hash
        return self.hash

    def __eq__(self, other) -> bool:
        assert self.hash and other.hash
        return self.hash == other.hash

    def __lt__(self, other) -> bool:
        assert self.hash and other.hash
        return self.hash < other.hash

    def freeze(self) -> bool:
        if self.frozen:
            return False
        self.frozen = True
        self.variables = frozenset(self.variables)
        return True

    @abstractmethod
    def assign(self, variable: str, value: str) -> bool: ...

    @abstractmethod
    def join(self, other: 'Assignment') -> 'Assignment': ...

    @abstractmethod
    def check_negation(self, negation: 'Assignment') -> bool: ...


def _bad_assign(variable, value, frozen):
    if variable is None or value is None or frozen:
        raise ValueError(f'Invalid assignment: variable = {variable} value = {value} frozen = {frozen}')


class OrderedAssignment(Assignment):

    def __init__(self):
        super().__init__()
        self.mapping: Dict[str, str] = {}
        self.values: Union[Set[str], FrozenSet] = set()

    def __repr__(self):
        return repr(self.mapping)

    def freeze(self):
        assert super().freeze()
        self.values = frozenset(self.values)
        self.hash = hash(frozenset(self.mapping.items()))
        return True

    def assign(self, variable: str, value: str) -> bool:
        _bad_assign(variable, value, self.frozen)
        if variable in self.variables:
            return self.mapping[variable] == value
        if CONFIG['no_overload'] and value in self.values:
            return False
        self.variables.add(variable)
        self.values.add(value)
        self.mapping[variable] = value
        return True

    def evaluate_compatibility(self, other) -> CompatibilityStatus:
        assert other is not None
        if self.hash == other.hash:
            return CompatibilityStatus.EQUAL
        if any(self.mapping[v] != other.mapping[v] for v in self.variables & other.variables):
            return CompatibilityStatus.INCOMPATIBLE
        if other.variables < self.variables:
            return CompatibilityStatus.FIRST_COVERS_SECOND
        if self.variables < other.variables:
            return CompatibilityStatus.SECOND_COVERS_FIRST
        return CompatibilityStatus.NO_COVERING

    def compatible(self, other) -> bool:
        return self.evaluate_compatibility(other) != CompatibilityStatus.INCOMPATIBLE

    def _join_ordered(self, other):
        status = self.evaluate_compatibility(other)
        if status == CompatibilityStatus.INCOMPATIBLE:
            return None
        if status in (CompatibilityStatus.EQUAL, CompatibilityStatus.FIRST_COVERS_SECOND):
            return self
        if status == CompatibilityStatus.SECOND_COVERS_FIRST:
            return other
        merged = OrderedAssignment()
        for var, val in list(self.mapping.items()) + list(other.mapping.items()):
            if not merged.assign(var, val):
                return None
        merged.freeze()
        return merged

    def join(self, other: Assignment) -> Assignment:
        assert self.frozen and other.frozen
        return self._join_ordered(other) if isinstance(other, OrderedAssignment) else other.join(self)

    def check_negation(self, negation: Assignment) -> bool:
        if isinstance(negation, OrderedAssignment):
            return self.evaluate_compatibility(negation) not in (
                CompatibilityStatus.EQUAL, CompatibilityStatus.FIRST_COVERS_SECOND)
        return not negation.is_covered_by_ordered(self)


class UnorderedAssignment(Assignment):

    def __init__(self):
        super().__init__()
        self.symbols: Dict[str, int] = {}
        self.values: Dict[str, int] = {}

    def __repr__(self):
        syms = [s for s, c in self.symbols.items() for _ in range(c)]
        vals = [v for v, c in self.values.items() for _ in range(c)]
        return '*' + repr(dict(zip(syms, vals)))

    def freeze(self):
        assert super().freeze()
        if sorted(self.symbols.values()) != sorted(self.values.values()):
            return False
        self.hash = hash((hash(frozenset(self.symbols.items())), hash(frozenset(self.values.items()))))
        return True

    def assign(self, variable: str, value: str) -> bool:
        _bad_assign(variable, value, self.frozen)
        if variable in self.variables:
            return False
        self.symbols[variable] = self.symbols.get(variable, 0) + 1
        self.values[value] = self.values.get(value, 0) + 1
        self.variables.add(variable)
        return True

    def join(self, other: Assignment) -> Assignment:
        assert self.frozen and other.frozen
        if isinstance(other, CompositeAssignment):
            return other.join(self)
        return CompositeAssignment(self).join(other)

    def check_negation(self, negation: Assignment) -> bool:
        if isinstance(negation, OrderedAssignment):
            return not self.contains_ordered(negation)
        if isinstance(negation, UnorderedAssignment):
            return not self.contains_unordered(negation)
        return all(not self.contains_unordered(u) for u in negation.unordered_mappings)

    def contains_ordered(self, ordered_assignment) -> bool:
        if not set(ordered_assignment.mapping) <= set(self.variables):
            return False
        need = Counter(ordered_assignment.mapping.values())
        return all(self.values.get(v, 0) >= c for v, c in need.items())

    def is_covered_by_ordered(self, ordered_assignment) -> bool:
        sym = Counter(self.symbols)
        val = Counter(self.values)
        sym.subtract(Counter(ordered_assignment.mapping.keys()))
        val.subtract(Counter(ordered_assignment.mapping.values()))
        return all(c <= 0 for c in sym.values()) and all(c <= 0 for c in val.values())

    def contains_unordered(self, unordered_assignment) -> bool:
        return all(self.symbols.get(s, 0) >= c for s, c in unordered_assignment.symbols.items()) and \
            all(self.values.get(v, 0) >= c for v, c in unordered_assignment.values.items())

    def compatible(self, other) -> bool:
        common_syms = set(self.variables) & set(other.variables)
        common_vals = set(self.values) & set(other.values)
        s_self = sum(self.symbols[s] for s in common_syms)
        s_other = sum(other.symbols[s] for s in common_syms)
        v_self = sum(self.values[v] for v in common_vals)
        v_other = sum(other.values[v] for v in common_vals)
        return v_other >= s_self and v_self >= s_other


class CompositeAssignment(Assignment):

    def __init__(self, assignment: UnorderedAssignment):
        super().__init__()
        self.unordered_mappings: List[UnorderedAssignment] = [assignment]
        self.ordered_mapping: Optional[OrderedAssignment] = None
        self.variables = deepcopy(assignment.variables)
        assert self._freeze()

    def __repr__(self):
        return f'Ordered = {self.ordered_mapping} | Unordered = {self.unordered_mappings}'

    def _freeze(self):
        assert super().freeze()
        self._recompute_hash()
        return True

    def freeze(self):
        assert False

    def assign(self, variable: str, value: str) -> bool:
        assert False

    def _recompute_hash(self) -> None:
        h = self.ordered_mapping.hash if self.ordered_mapping else 1
        for u in self.unordered_mappings:
            h ^= u.hash
        self.hash = h

    def _viable(self) -> bool:
        if not self.ordered_mapping:
            return bool(self.unordered_mappings)
        return all(u.contains_ordered(self.ordered_mapping) or u.is_covered_by_ordered(self.ordered_mapping)
                   for u in self.unordered_mappings)

    def _add_ordered_mapping(self, other: OrderedAssignment) -> bool:
        if self.ordered_mapping is None:
            self.ordered_mapping = other
        else:
            self.ordered_mapping = self.ordered_mapping.join(other)
            if self.ordered_mapping is None:
                return False
        if not self._viable():
            return False
        self._recompute_hash()
        return True

    def _add_unordered_mapping(self, u) -> bool:
        if self.ordered_mapping and not u.contains_ordered(self.ordered_mapping):
            return False
        if not all(x.compatible(u) for x in self.unordered_mappings):
            return False
        self.unordered_mappings.append(u)
        self._recompute_hash()
        return True

    def join(self, other: Assignment) -> Assignment:
        assert self.frozen and other.frozen
        out = deepcopy(self)
        if isinstance(other, OrderedAssignment):
            ok = out._add_ordered_mapping(other)
        elif isinstance(other, UnorderedAssignment):
            ok = out._add_unordered_mapping(other)
        else:
            ok = out._add_ordered_mapping(other.ordered_mapping) and \
                all(out._add_unordered_mapping(u) for u in other.unordered_mappings)
        return out if ok else None

    def check_negation(self, negation: Assignment) -> bool:
        if isinstance(negation, OrderedAssignment):
            return all(not u.contains_ordered(negation) for u in self.unordered_mappings)
        if isinstance(negation, UnorderedAssignment):
            return all(not u.contains_unordered(negation) for u in self.unordered_mappings)
        raise AttributeError("'CompositeAssignment' object has no attribute 'unordered_assignments'")

    def contains_ordered(self, ordered_assignment) -> bool:
        return all(u.contains_ordered(ordered_assignment) for u in self.unordered_mappings)

    def contains_unordered(self, unordered_assignment) -> bool:
        return all(u.contains_unordered(unordered_assignment) for u in self.unordered_mappings)


# ---------------------------------------------------------------------------
# Relational evaluation: the DB owns the device relation algebra
# (HipDB on one GPU, parallel.ShardedDB across ranks)
# ---------------------------------------------------------------------------

def _hip(db):
    if not isinstance(db, RelationalDB):
        raise TypeError(f"das_amd evaluates patterns on the MI355X index; got {db!r} (use HipDB)")
    return db


# ---------------------------------------------------------------------------
# Whole-expression plans: an And / Or / Not tree of ordered, flat Links is
# lowered once per (expression, index) to das_plan_node_t records and folded
# by das_plan_execute in a single native call (das_amd/csrc/plan.hip restates
# the And / Or / Not rules below).  Anything else -- unordered links,
# templates, nested link targets, sharded DBs -- takes the per-operator path.
# ---------------------------------------------------------------------------


class _Unsupported(Exception):
    pass


_RECORD = struct.Struct("<51I")
_WORDS = 51


def _node_record(op, nchild=0, value=0, spec=None, ij=None):
    """One das_plan_node_t as 204 bytes (51 u32 words, include/das_mi355x.h)."""
    words = [op, nchild, value, 0, 0] + [0] * 46
    if spec is not None:
        args, dedup = spec
        words[3] = 1 if dedup else 0
        words[5:28] = _scan_words(*args)
    if ij is not None:
        words[4] = 1
        words[28:51] = _scan_words(ij[0], ij[1], ij[2], ij[3], 0, True)
    return _RECORD.pack(*[w & 0xFFFFFFFF for w in words])


def _scan_words(arity, type_id, targets, var, n_vars, ordered, no_overload=False, emit_link=False, order_pos=-1):
    """das_link_scan_t as 23 words (field order of include/das_mi355x.h)."""
    t = list(targets) + [_lib.DAS_NONE] * (8 - len(targets))
    v = list(var) + [-1] * (8 - len(var))
    return [arity, _lib.DAS_NONE if type_id is None else type_id] + t + v + \
        [n_vars, 1 if ordered else 0, 1 if no_overload else 0, 1 if emit_link else 0, order_pos]


_HEADERS = {}


def _header(op, nchild=0, value=0):
    key = (op, nchild, value)
    r = _HEADERS.get(key)
    if r is None:
        r = _HEADERS[key] = _node_record(op, nchild, value)
    return r


def _link_signature(link):
    """What a Link's plan record depends on besides the index: its type,
    targets (variable names / node type and name) and join-order hint."""
    sig = [link.atom_type, getattr(link, '_order_var', None)]
    for t in link.targets:
        k = t._k
        if k == 'v':
            sig.append(t.name)
        elif k == 'n':
            sig.append((t.atom_type, t.name))
        else:
            raise _Unsupported()          # LinkTemplate / nested Link / typed targets
    return tuple(sig)


def _link_record(link, db, no_overload):
    """Link.matched (pattern_matcher.py:502-538) as one plan record: every
    target matched (node_exists), link_exists when nothing is a wildcard,
    else the match_link scan (+ the index-join form And may use)."""
    if not all(t.matched(db, None) for t in link.targets):
        return _header(_lib.PLAN_CONST, 0, 0)
    handles = [t.get_handle(db) for t in link.targets]
    if WILDCARD not in handles:
        return _header(_lib.PLAN_CONST, 0, 1 if db.link_exists(link.atom_type, handles) else 0)
    var_ids = [_vid(t.name) if t._k == 'v' else None for t in link.targets]
    hint = getattr(link, '_order_var', None)
    spec = db.link_scan_spec(link.atom_type, handles, var_ids, True, no_overload,
                             _vid(hint) if hint is not None else None)
    if spec is None:
        return _header(_lib.PLAN_CONST, 0, 0)
    ij = None if no_overload else db.index_join_spec(link.atom_type, handles, var_ids)
    return _node_record(_lib.PLAN_LINK, 0, 0, spec, ij)


def _template_record(tmpl, db, no_overload):
    """LinkTemplate.matched (pattern_matcher.py:603-614 over
    get_matched_type_template, redis_mongo_db.py:269-275) as one TEMPLATE
    record: the composite type's links, every target a typed variable."""
    ct, named = db._template_ctype([tmpl.link_type, *[v.type for v in tmpl.targets]])
    if named is not None:
        raise _Unsupported()                  # a template without targets (match_template's assertion case)
    if ct < 0:
        return _header(_lib.PLAN_CONST, 0, 0)
    var_ids = [_vid(v.name) for v in tmpl.targets]
    words = [_lib.PLAN_TEMPLATE, 0, 0, 1 if len(set(var_ids)) != len(var_ids) else 0, 0] + [0] * 46
    words[5:28] = _scan_words(len(var_ids), ct, [], var_ids, 0, True, no_overload)
    return _RECORD.pack(*[w & 0xFFFFFFFF for w in words])


def _walk(expr, out, links, root=True):
    """Prefix-order skeleton of `expr`: header records and Link slots."""
    k = expr._k
    if k == 'a' or k == 'o':
        if not expr.terms:
            out.append(_header(_lib.PLAN_CONST, 0, 0))
            return
        if k == 'a' and not getattr(expr, '_planned', False):
            expr._plan_orders()
            expr._planned = True
        out.append(_header(_lib.PLAN_AND if k == 'a' else _lib.PLAN_OR, len(expr.terms)))
        for t in expr.terms:
            _walk(t, out, links, False)
    elif k == 'x':
        out.append(_header(_lib.PLAN_NOT, 1))
        _walk(expr.term, out, links, False)
    elif k == 'l':
        if any(t._k == 't' for t in expr.targets):
            # Link._typed_variable_matched (:491-500); at the root its answer
            # after a failing target is observable: the host path keeps that
            if root:
                raise _Unsupported()
            if any(t._k in ('v', 'tv') for t in expr.targets):
                out.append(_header(_lib.PLAN_CONST, 0, 0))
                return
            out.append(_header(_lib.PLAN_TVM, len(expr.targets)))
            for t in expr.targets:
                _walk(t, out, links, False)
            return
        if not expr.ordered:
            raise _Unsupported()
        links.append((len(out), expr, _link_signature(expr)))
        out.append(None)
    elif k == 't':
        if not expr.ordered or root:
            raise _Unsupported()
        links.append((len(out), expr, ('t', expr.link_type, tuple((v.name, v.type) for v in expr.targets))))
        out.append(None)
    elif k == 'n' or k == 'v':
        links.append((len(out), expr, None))
        out.append(None)
    else:
        raise _Unsupported()


class _NoShape(Exception):
    pass


def _shape(expr, nodes):
    """Structure key of `expr` with its nodes' names left out (the nodes are
    appended to `nodes` in walk order).  Raises _NoShape for what a
    parameterised plan cannot carry: a Link whose targets are all grounded
    (its record is link_exists of those very handles) and the unordered link
    types (their scan keys are sorted by handle)."""
    k = expr._k
    if k == 'n':
        nodes.append(expr)
        return expr.atom_type
    if k == 'v':
        return ('v', expr.name)
    if k == 'tv':
        return ('tv', expr.name, expr.type)
    if k == 'l':
        if expr.atom_type in UNORDERED_LINK_TYPES or all(t._k == 'n' for t in expr.targets):
            raise _NoShape()
        return ('l', expr.atom_type, expr.ordered, tuple([_shape(t, nodes) for t in expr.targets]))
    if k == 't':
        return ('t', expr.link_type, expr.ordered, tuple([(v.name, v.type) for v in expr.targets]))
    if k == 'x':
        return ('x', _shape(expr.term, nodes))
    if k == 'a' or k == 'o':
        return (k, tuple([_shape(t, nodes) for t in expr.terms]))
    raise _NoShape()


def _node_ids(db, nodes):
    """Atom ids of `nodes` (one batched lookup), or None if one is not a node
    of the KB (its term's record would then be a constant)."""
    hs = [n.get_handle(db) for n in nodes]
    out = []
    for aid, cat, _ in db._resolve(hs):
        if aid < 0 or cat != 1:
            return None
        out.append(aid)
    return out


_UNORDERED = frozenset(UNORDERED_LINK_TYPES)


def _lower(expr, db, no_overload):
    """The das_plan_node_t array (51 u32 words per node) of `expr`, or None.

    A query shape seen before (the same tree with other node names, e.g. a
    fresh gene anchor) is answered from the shape cache: its words with each
    node's atom id patched into the scan / index-join target slots it
    occupies -- one batched handle lookup, no re-lowering.  Otherwise Link
    records are cached per (index, signature), so a repeated query re-lowers
    only the links whose anchors changed; their handles are resolved in one
    batched lookup."""
    shapes = db.__dict__.setdefault('_plan_shapes', {})
    if shapes and _assign is not None and hasattr(_assign, "plan_words"):
        # the shape-cache hit below, in C (das_amd/csrc/pyassign.c plan_words);
        # None: take the Python path
        nh, hc = getattr(db, "_node_handles", None), getattr(db, "_handle_cache", None)
        if type(nh) is dict and type(hc) is dict:
            w = _assign.plan_words(expr, shapes, no_overload, nh, hc, getattr(db, "_node_dir", None),
                                   _UNORDERED, db.get_node_handle)
            if w is not None:
                return w
    nodes = []
    try:
        skey = (no_overload, _shape(expr, nodes))
    except _NoShape:
        skey = None
    if skey is not None:
        hit = shapes.get(skey)
        if hit is not None:
            ids = _node_ids(db, nodes) if nodes else []
            if ids is not None:
                words, patches = hit
                w = words.copy()
                for wi, k in patches:
                    w[wi] = ids[k]
                return w
    out, links = [], []
    try:
        _walk(expr, out, links)
    except _Unsupported:
        return None
    cache = db.__dict__.setdefault('_plan_records', {})
    if len(cache) > (1 << 16):
        cache.clear()
    todo = []
    for pos, e, sig in links:
        if sig is not None:
            r = cache.get((no_overload, sig))
            if r is not None:
                out[pos] = r
                continue
        todo.append((pos, e, sig))
    if todo:
        try:
            _resolve(todo, out, cache, db, no_overload)
        except _Unsupported:
            return None
    words = np.frombuffer(b"".join(out), dtype=np.uint32)
    if skey is not None and (not nodes or _node_ids(db, nodes) is not None):
        # every node exists: each Link record's grounded targets are these
        # nodes' ids at fixed word offsets (scan targets at 7 + p, the index
        # join's at 30 + p; include/das_mi355x.h das_plan_node_t)
        ordinal = {id(n): i for i, n in enumerate(nodes)}
        patches = []
        for pos, e, _ in links:
            if e._k != 'l':
                continue
            base = _WORDS * pos
            if int(words[base]) != _lib.PLAN_LINK:
                continue
            for p, t in enumerate(e.targets):
                if t._k == 'n':
                    patches.append((base + 7 + p, ordinal[id(t)]))
                    if int(words[base + 4]):
                        patches.append((base + 30 + p, ordinal[id(t)]))
        if len(shapes) > (1 << 12):
            shapes.clear()
        shapes[skey] = (words, patches)
    return words


def _resolve(todo, out, cache, db, no_overload):
    """Records of the leaves _lower found no cached record for."""
    if todo:
        nodes = [t for _, e, _ in todo for t in (e.targets if e._k == 'l' else [e] if e._k == 'n' else [])
                 if t._k == 'n']
        if nodes:
            db.prefetch_handles([n.get_handle(db) for n in nodes])
        for pos, e, sig in todo:
            if e._k == 'n':
                out[pos] = _header(_lib.PLAN_CONST, 0, 1 if e.matched(db, None) else 0)
            elif e._k == 'v':
                out[pos] = _header(_lib.PLAN_CONST, 0, 1)
            elif e._k == 't':
                out[pos] = cache[(no_overload, sig)] = _template_record(e, db, no_overload)
            else:
                out[pos] = cache[(no_overload, sig)] = _link_record(e, db, no_overload)


def _try_plan(expr, db, answer):
    """Evaluates `expr` with one das_plan_execute call when it can; returns
    its matched() result, or None for the per-operator path."""
    if os.environ.get("DAS_PLAN") == "0" or answer.negation:
        return None
    if type(db) is not HipDB:
        # a sharded DB (das_amd.parallel.ShardedDB) plans across its GPUs
        sharded = getattr(db, "plan_sharded", None)
        return sharded(expr, answer) if sharded is not None else None
    if db._stale and db.touches_stale(expr):
        return None                             # stale_pattern_keys: the per-operator path adds them
    no_overload = bool(CONFIG['no_overload'])
    key = (db.generation, no_overload)          # generation: unique per load, any HipDB
    cached = getattr(expr, '_plan', None)
    if cached is None or cached[0] != key:
        cached = (key, _lower(expr, db, no_overload))
        expr._plan = cached
    nodes = cached[1]
    if nodes is None:
        return None
    matched, negation, tables = db.ctx.plan_execute(nodes, len(nodes) // 51, no_overload)
    answer._set(db, Relation(tables))
    answer.negation = negation
    return matched


def matched_many(db, exprs, tag=None):
    """[(matched, answer)] of independent expressions, each as
    `expr.matched(db, answer)` with a fresh PatternMatchingAnswer would give.
    On one HipDB the plannable ones go to ONE das_plan_execute_many call (the
    GPU runs an expression's fused chain while the host prepares the next);
    the rest, and every expression on other DBs, are evaluated one by one.
    tag = (index, name): the kernel scopes of exprs[index] are recorded as
    "<scope>@<name>" (das_prof_tag_plan; bench.py's in-step And join)."""
    res = [None] * len(exprs)
    batch = []
    if type(db) is HipDB and os.environ.get("DAS_PLAN") != "0":
        no_overload = bool(CONFIG['no_overload'])
        key = (db.generation, no_overload)
        for i, e in enumerate(exprs):
            # the operators whose matched() tries a whole-expression plan
            # first, with its prelude (And.matched / Or.matched / Not.matched)
            # (a root Link is one LINK / CONST plan node: Link.matched's scan
            # or link_exists, :502-538 -- batched too, e.g. bench Q1)
            if type(e) is Link:
                if not e.ordered:
                    continue
            elif type(e) not in (And, Or, Not) or (type(e) is not Not and not e.terms):
                continue
            if db._stale and db.touches_stale(e):
                continue
            cached = getattr(e, '_plan', None)
            if cached is None or cached[0] != key:
                cached = (key, _lower(e, db, no_overload))
                e._plan = cached
            if cached[1] is not None:
                batch.append((i, cached[1]))
        if batch:
            at = next((k for k, (i, _) in enumerate(batch) if tag and i == tag[0]), None)
            if at is not None:
                db.ctx.prof_tag_plan(at, tag[1])
            try:
                outs = db.ctx.plan_execute_many([(w, len(w) // _WORDS) for _, w in batch], no_overload)
            finally:
                if at is not None:
                    db.ctx.prof_tag_plan(None)
            for (i, _), (matched, negation, tables) in zip(batch, outs):
                ans = PatternMatchingAnswer()
                ans._set(db, Relation(tables))
                ans.negation = negation
                res[i] = (matched, ans)
    for i, e in enumerate(exprs):
        if res[i] is None:
            ans = PatternMatchingAnswer()
            tagged = tag is not None and i == tag[0] and type(db) is HipDB
            if tagged:
                db.ctx.prof_tag(tag[1])
            try:
                res[i] = (e.matched(db, ans), ans)
            finally:
                if tagged:
                    db.ctx.prof_tag(None)
    return res


# ---------------------------------------------------------------------------
# Answers
# ---------------------------------------------------------------------------
class PatternMatchingAnswer:

    def __init__(self):
        self._rel: Optional[Relation] = None
        self._db: Optional[HipDB] = None
        self._py = None
        self.negation: bool = False

    def __repr__(self):
        s = 'NOT\n' if self.negation else ''
        for a in self.assignments:
            s += str(a) + '\n'
        return s

    def _set(self, db, rel):
        self._db = db
        self._rel = rel
        self._py = None

    def _relation(self):
        if self._py is not None and self._rel is None:
            if self._py:
                raise NotImplementedError("host-built assignments cannot feed the device matcher")
            return Relation()
        return self._rel if self._rel is not None else Relation()

    def __len__(self):
        return len(self.assignments)

    @property
    def assignments(self):
        if self._py is None:
            self._py = _materialize(self._db, self._rel)
        return self._py

    @assignments.setter
    def assignments(self, value):
        self._py = set(value)
        self._rel = None

    def count(self) -> int:
        """Number of distinct assignments, without building Python objects
        (summed over ranks for a sharded DB)."""
        if self._py is not None and self._rel is None:
            return len(self._py)
        if self._db is None:
            return 0
        return self._db.rel_count(self._relation())

    def names(self, variable=None, strict=True, db=None):
        """The node names of the answer's values, get_node_name of each in
        one call: for one variable a list, one name per assignment; with no
        variable a dict variable -> list, the lists aligned row by row.  Row
        order is unspecified (the tables' row order on the device path, set
        order on the host path).  A value that is not a node raises
        ValueError("Invalid handle: ..."), or is None with strict=False; a
        variable the answer does not bind raises KeyError.

        Device path -- the answer still holds its device relation, every
        local table is ordered and the DB is a HipDB: one das_node_names
        call per column, read from the table where it lies (no fetch, no
        handle string, no Assignment object).  Everything else (unordered or
        composite tables, hand-set assignments, a sharded DB,
        DAS_NAME_FETCH=0, an index without a name heap, fewer rows than
        HipDB.NAME_FETCH_MIN) runs names_host.  `db.name_fetch_stats` counts
        the device calls and the host runs.  `db`: the DB
        of an answer whose assignments were set by hand."""
        db = db if db is not None else self._db
        if db is None:
            if self._py is None or self._py:
                raise ValueError("names: the answer holds no database")
            return {} if variable is None else []
        if self._rel is not None and db is self._db and isinstance(db, HipDB) and db._name_fetch_on_device():
            tables = [t for t in db.rel_local_tables(self._rel) if t.nrows]
            if (all(t.kind == _lib.TABLE_ORDERED for t in tables)
                    and db._name_fetch_on_device(sum(t.nrows for t in tables))):
                try:
                    return _names_device(db, tables, variable, strict)
                except NotImplementedError:     # no name heap for this index
                    pass
        if hasattr(db, "name_fetch_stats"):
            db.name_fetch_stats["host"] += 1
        return names_host(db, self, variable, strict)

    def value_counts(self, variable, db=None) -> "ValueCounts":
        """The answer's rows per value of one variable: a ValueCounts whose
        `total` is count().  A variable the answer does not bind raises
        KeyError.

        Device path -- the answer still holds its device relation, every
        local table is ordered and binds the variable and the DB is a HipDB:
        one das_group_counts call over the tables where they lie.  An
        unresolved answer (a deferred product, index join or scan view) is
        counted from what it keeps, without writing its rows; only a
        deferred index join grouped by a variable its expansion reads from
        the index writes them first.  Everything else (unordered or
        composite tables, hand-set assignments, a sharded DB, DAS_GROUP=0,
        fewer rows than HipDB.GROUP_MIN) runs value_counts_host.
        `db.group_stats` counts the calls of each path and the tables counted
        unwritten and settled.  `db`: the DB of an answer whose assignments
        were set by hand."""
        db = db if db is not None else self._db
        if db is None:
            if self._py is None or self._py:
                raise ValueError("value_counts: the answer holds no database")
            return ValueCounts(db, counter=Counter())
        if (self._rel is not None and db is self._db and isinstance(db, HipDB)
                and os.environ.get("DAS_GROUP", "1") != "0"):
            tables = [t for t in db.rel_local_tables(self._rel) if t.nrows]
            if (all(t.kind == _lib.TABLE_ORDERED for t in tables)
                    and sum(t.nrows for t in tables) >= db.GROUP_MIN):
                cols = []
                for t in tables:
                    bound = [_var_name(v) for v in t.vars]
                    if variable not in bound:
                        raise KeyError(variable)
                    cols.append(bound.index(variable))
                ids, counts, (unwritten, settled) = db.ctx.group_counts(tables, cols)
                db.group_stats["device"] += 1
                db.group_stats["unwritten"] += unwritten
                db.group_stats["settled"] += settled
                return ValueCounts(db, ids=ids, counts=counts)
        if hasattr(db, "group_stats"):
            db.group_stats["host"] += 1
        return ValueCounts(db, counter=value_counts_host(db, self, variable))

    def distinct(self, variable, db=None) -> List[str]:
        """The handles of the distinct values of one variable; order
        unspecified (ascending atom id on the device path of value_counts,
        sorted by handle on the host path)."""
        return list(self.value_counts(variable, db=db).handles)

    def _text_plan(self, db, max_bytes):
        """The device path's (table, literals) list, or None where text()
        takes the host path (the rules are rows_text_plan's)."""
        if (self._rel is None or self._py is not None or db is None or db is not self._db
                or not isinstance(db, HipDB) or os.environ.get("DAS_QUERY_TEXT", "1") == "0"):
            return None
        return rows_text_plan(db.rel_local_tables(self._rel), db.QUERY_TEXT_MIN, max_bytes)

    def text(self, db=None) -> str:
        """str(self.assignments), the string DistributedAtomSpace.query
        returns: "{" + ", ".join(repr(a.mapping) ...) + "}", or "set()" for
        an empty answer.  The order of the rows is unspecified (set order on
        the host path; table row order, table after table, on the device
        path); each row is byte for byte the same on both.

        Device path -- the answer still holds its device relation and no
        Assignment objects, the DB is a HipDB, DAS_QUERY_TEXT is not "0",
        every non-empty local table is ordered with at least one column, no
        two tables bind the same set of variables (so no row repeats across
        tables), and the answer has at least HipDB.QUERY_TEXT_MIN rows and at
        most HipDB.QUERY_TEXT_MAX_BYTES bytes of text: one
        das_table_rows_text call per table writes the rows' text where the
        string is assembled -- no fetch, no handle string, no Assignment
        object; a deferred product or scan view is not written.  Everything
        else (empty answers, unordered or composite tables, hand-set
        assignments, a sharded DB, a row beyond ROWS_TEXT_MAX_ROW, a value
        that is no atom) formats the set as before.  `db.query_text_stats`
        counts the calls of each path."""
        db = db if db is not None else self._db
        plan = self._text_plan(db, db.QUERY_TEXT_MAX_BYTES if isinstance(db, HipDB) else None)
        if plan is not None:
            out = _rows_text_device(db, plan)
            if out is not None:
                db.query_text_stats["device"] += 1
                return out
        if hasattr(db, "query_text_stats"):
            db.query_text_stats["host"] += 1
        from ..distributed_atom_space import _format_assignments
        return _format_assignments(self.assignments)

    def iter_text(self, chunk_rows=1 << 20, db=None):
        """text() in pieces: a generator of str whose concatenation is
        text(), for an answer too large to hold as one string (write each
        piece to a socket or file).  On the device path one
        das_table_rows_text call renders each chunk of `chunk_rows` rows;
        braces and the ", " between chunks and tables are added here; a
        deferred product is never written; there is no byte ceiling.  An
        answer the device path does not take is one piece, the host text.  A
        value that is no atom raises ValueError at its chunk."""
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("iter_text: chunk_rows must be positive")
        db = db if db is not None else self._db
        plan = self._text_plan(db, None)
        if plan is None:
            yield self.text(db=db)
            return
        db.query_text_stats["device"] += 1
        yield from iter_rows_text(plan, chunk_rows, lambda t, lits, row0, n: _rows_text_chunk(db, t, lits, row0, n))


ROW_SEP = b", "                      # between the rows of str(set)


def row_literals(names):
    """The literal pieces of repr({name: handle, ...}) around the handles, as
    UTF-8 bytes: len(names) + 1 of them.  repr(name) is taken here, so a name
    holding ' switches to double quotes, a backslash is doubled and a
    printable non-ASCII letter stays as it is; a handle is 32 hex characters,
    whose repr is the handle between single quotes."""
    names = list(names)
    if not names:
        raise ValueError("row_literals: no variable")
    lits = ["{" + repr(names[0]) + ": '"]
    lits += ["', " + repr(n) + ": '" for n in names[1:]]
    lits.append("'}")
    return [s.encode("utf-8") for s in lits]


def rows_text_plan(tables, min_rows=0, max_bytes=None):
    """[(table, its row literals)] over the non-empty tables where
    das_table_rows_text can render the answer, else None: every non-empty
    table ordered with at least one column, the tables' variable sets
    pairwise distinct, at least `min_rows` rows (and one), no row with its
    separator beyond ROWS_TEXT_MAX_ROW bytes, and -- max_bytes not None -- a
    text of at most that many bytes."""
    tables = [t for t in tables if t.nrows]
    if not tables or sum(t.nrows for t in tables) < min_rows:
        return None
    if any(t.kind != _lib.TABLE_ORDERED or len(t.vars) < 1 for t in tables):
        return None
    if len({frozenset(t.vars) for t in tables}) != len(tables):
        return None
    plan = [(t, row_literals(_var_name(v) for v in t.vars)) for t in tables]
    if any(_lib.rows_text_size(lits, ROW_SEP, 1) + len(ROW_SEP) > _lib.ROWS_TEXT_MAX_ROW for _, lits in plan):
        return None
    if max_bytes is not None and rows_text_bytes(plan) > max_bytes:
        return None
    return plan


def rows_text_bytes(plan):
    """Bytes of the text of a rows_text_plan: the braces, every table's rows
    and the separators between the tables."""
    return 2 + sum(_lib.rows_text_size(lits, ROW_SEP, t.nrows) for t, lits in plan) + len(ROW_SEP) * (len(plan) - 1)


def iter_rows_text(plan, chunk_rows, render):
    """The pieces of a plan's text: "{", render(table, literals, row0, n) for
    every chunk of at most chunk_rows rows, table after table, each but the
    first led by ", ", and "}"."""
    yield "{"
    sep = ""
    for t, lits in plan:
        for row0 in range(0, t.nrows, chunk_rows):
            yield sep + render(t, lits, row0, min(chunk_rows, t.nrows - row0))
            sep = ROW_SEP.decode()
    yield "}"


def _rows_text_chunk(db, t, lits, row0, n):
    res = db.ctx.rows_text(t, lits, ROW_SEP, row0=row0, nrows=n)
    if res is None:
        raise ValueError("iter_text: a row beyond ROWS_TEXT_MAX_ROW bytes")
    data, total, bad = res
    if bad or total != data.size:
        raise ValueError(f"iter_text: {bad} values of rows {row0}..{row0 + n} are no atoms")
    return str(memoryview(data), "utf-8")


def _rows_text_device(db, plan):
    """text() over a rows_text_plan: every table's rows written by one
    das_table_rows_text call into its place in one buffer, decoded once.
    None where a call refuses a row or meets a value that is no atom."""
    buf = np.empty(rows_text_bytes(plan), dtype=np.uint8)
    buf[0] = ord("{")
    at = 1
    for i, (t, lits) in enumerate(plan):
        if i:
            buf[at:at + len(ROW_SEP)] = np.frombuffer(ROW_SEP, dtype=np.uint8)
            at += len(ROW_SEP)
        size = _lib.rows_text_size(lits, ROW_SEP, t.nrows)
        res = db.ctx.rows_text(t, lits, ROW_SEP, out=buf[at:at + size])
        if res is None or res[1] != size or res[2]:
            return None
        at += size
    buf[at] = ord("}")
    return str(memoryview(buf), "utf-8")


def value_counts_host(db, answer, variable):
    """The definition of PatternMatchingAnswer.value_counts, over any
    DBInterface: Counter(a.mapping[variable] for a in answer.assignments),
    handle -> rows.  An assignment without a `mapping` (unordered, composite)
    raises AttributeError and a row that does not bind the variable
    KeyError(variable), as names_host does."""
    out = Counter()
    for a in answer.assignments:
        out[a.mapping[variable]] += 1
    return out


class ValueCounts:
    """Distinct values of one variable of an answer and the rows that hold
    each.  Built from atom ids (the device path: `ids` uint32 ascending,
    `counts` uint64) or from a Counter handle -> rows (the host path: `ids`
    is None, the handles sorted)."""

    def __init__(self, db, ids=None, counts=None, counter=None):
        self._db = db
        if counter is not None:
            self.ids = None
            self._handles = sorted(counter)
            self.counts = np.array([counter[h] for h in self._handles], dtype=np.uint64)
        else:
            self.ids = np.asarray(ids, dtype=np.uint32)
            self.counts = np.asarray(counts, dtype=np.uint64)
            self._handles = None

    @property
    def handles(self) -> List[str]:
        """The values as 32-hex handles (db.hex_of), built on first access."""
        if self._handles is None:
            self._handles = list(self._db.hex_of(self.ids)) if len(self.ids) else []
        return self._handles

    def __len__(self):
        return len(self.counts)

    @property
    def total(self) -> int:
        return int(self.counts.sum(dtype=np.uint64)) if len(self.counts) else 0

    def names(self, strict=True) -> List[Optional[str]]:
        """get_node_name of every value, in the order of `handles`: one bulk
        db.get_node_names call where the DB has it."""
        if not len(self):
            return []
        if hasattr(self._db, "get_node_names"):
            return list(self._db.get_node_names(self.ids if self.ids is not None else self.handles, strict=strict))
        out = []
        for h in self.handles:
            try:
                out.append(self._db.get_node_name(h))
            except ValueError:
                if strict:
                    raise
                out.append(None)
        return out

    def _order(self, k=None):
        # by count descending, ties by handle ascending
        handles = self.handles
        order = sorted(range(len(handles)), key=lambda i: (-int(self.counts[i]), handles[i]))
        return order if k is None else order[:max(int(k), 0)]

    def most_common(self, k=None, names=False):
        """(handle, count) pairs by count descending, ties by handle
        ascending (the same on both paths); the first k of them.  names:
        (node name, count) pairs instead."""
        order = self._order(k)
        if names:
            if self.ids is not None and hasattr(self._db, "get_node_names"):
                keys = list(self._db.get_node_names(self.ids[order], strict=True)) if order else []
            else:
                keys = [self._db.get_node_name(self.handles[i]) for i in order]
        else:
            keys = [self.handles[i] for i in order]
        return [(key, int(self.counts[i])) for key, i in zip(keys, order)]

    def as_dict(self) -> Dict[str, int]:
        return {h: int(n) for h, n in zip(self.handles, self.counts)}


def names_host(db, answer, variable=None, strict=True):
    """The definition of PatternMatchingAnswer.names, over any DBInterface:
    [db.get_node_name(a.mapping[variable]) for a in answer.assignments], the
    notebooks' get_mappings loop; with no variable, that list for every
    variable an assignment binds, over one pass of the assignments.  An
    assignment without a `mapping` (unordered, composite) raises
    AttributeError, as that loop does."""
    rows = list(answer.assignments)
    if variable is not None:
        variables = [variable]
    else:
        variables = sorted(set().union(*[a.variables for a in rows])) if rows else []
    out = {v: [] for v in variables}
    for a in rows:
        for v in variables:
            h = a.mapping[v]
            try:
                out[v].append(db.get_node_name(h))
            except ValueError:
                if strict:
                    raise
                out[v].append(None)
    return out[variable] if variable is not None else out


def _names_device(db, tables, variable, strict):
    """names over ordered device tables: das_node_names per column."""
    if variable is not None:
        variables = [variable]
    else:
        variables = sorted({_var_name(v) for t in tables for v in t.vars})
    out = {v: [] for v in variables}
    for t in tables:
        bound = [_var_name(v) for v in t.vars]
        for v in variables:
            if v not in bound:
                raise KeyError(v)
    for t in tables:
        bound = [_var_name(v) for v in t.vars]
        for v in variables:
            c = bound.index(v)
            off, data, kind = db.ctx.node_names(table=t, col=c)
            db.name_fetch_stats["device"] += 1
            if strict and not kind.all():
                row = int(np.flatnonzero(kind == 0)[0])
                raise ValueError(f"Invalid handle: {db.hex_of(t.fetch(row, 1)[c])[0]}")
            out[v] += _lib.decode_names(off, data, kind)
    return out[variable] if variable is not None else out


try:
    from .. import _assign          # C builder of the answer's Assignment objects (csrc/pyassign.c)
except ImportError:                 # not built: the same objects through assign() / freeze() below
    _assign = None


def _handle_strings(db, fetched):
    """One handle string per distinct atom id of the fetched tables: (lut,
    strs, fetched') with strs[lut[v]] = the 32-hex handle of value v of the
    (possibly re-coded) columns in fetched'.  Dense id ranges index a lookup
    table directly; a few values over a wide id range are re-coded to their
    rank among the distinct ids (no id-sized allocation)."""
    parts = [c.ravel() for _, c in fetched if c.size]
    if not parts:
        return np.zeros(1, np.uint32), [], fetched
    total = sum(p.size for p in parts)
    hi = int(max(int(p.max()) for p in parts))
    if hi < (1 << 27) and 8 * total >= hi:
        present = np.zeros(hi + 1, dtype=bool)
        for p in parts:
            present[p] = True
        ids = np.flatnonzero(present).astype(np.uint32)
        lut = np.zeros(hi + 1, dtype=np.uint32)
        lut[ids] = np.arange(ids.size, dtype=np.uint32)
        return lut, list(db.hex_of(ids)), fetched
    ids = np.unique(np.concatenate(parts))
    recoded = [(t, np.searchsorted(ids, c).astype(np.uint32)) for t, c in fetched]
    return np.arange(ids.size, dtype=np.uint32), list(db.hex_of(ids)), recoded


def _materialize(db, rel, limit=None):
    """answer.assignments: the reference's set of Assignment objects for the
    device relation (lazy: built when a caller reads it).  `limit`: only the
    first `limit` rows (bench.py's materialisation rate on large answers)."""
    out = set()
    if rel is None or not rel:
        return out
    fetched = []
    for t in db.rel_local_tables(rel):
        if limit is not None:
            if limit <= 0:
                break
            fetched.append((t, t.fetch(0, limit)))
            limit -= fetched[-1][1].shape[1]
        else:
            fetched.append((t, t.fetch()))
    fast = _assign is not None and all(t.kind != _lib.TABLE_COMPOSITE for t, _ in fetched)
    if fast:
        lut, strs, fetched = _handle_strings(db, fetched)
        # the objects hold strings and frozensets only (no reference cycles):
        # the cyclic collector's passes over millions of young objects would
        # cost more than building them
        gc_on = gc.isenabled()
        gc.disable()
        try:
            for t, cols in fetched:
                if not t.nrows:
                    continue
                names = tuple(_var_name(v) for v in t.vars)
                cls, kind = (OrderedAssignment, 0) if t.kind == _lib.TABLE_ORDERED else (UnorderedAssignment, 1)
                _assign.add_rows(out, cls, kind, names, np.ascontiguousarray(cols, np.uint32), lut, strs)
        finally:
            if gc_on:
                gc.enable()
        return out
    for t, cols in fetched:
        names = [_var_name(v) for v in t.vars]
        hexcols = [db.hex_of(c) for c in cols]
        if t.kind == _lib.TABLE_COMPOSITE:
            o_cols = [k for k, m in enumerate(t.members) if m < 0]
            m_cols = {}
            for k, m in enumerate(t.members):
                if m >= 0:
                    m_cols.setdefault(m, []).append(k)
        for i in range(cols.shape[1] if cols.ndim == 2 else 0):
            if t.kind == _lib.TABLE_ORDERED:
                a = _ordered(names, hexcols, range(len(names)), i)
            elif t.kind == _lib.TABLE_UNORDERED:
                a = _unordered(names, hexcols, range(len(names)), i)
            else:
                us = [_unordered(names, hexcols, m_cols[m], i) for m in sorted(m_cols)]
                a = CompositeAssignment(us[0])
                a.unordered_mappings = us
                a.ordered_mapping = _ordered(names, hexcols, o_cols, i) if o_cols else None
                a._recompute_hash()
            out.add(a)
    return out


def _ordered(names, hexcols, cols, i):
    a = OrderedAssignment()
    for k in cols:
        a.assign(names[k], hexcols[k][i])
    a.freeze()
    return a


def _unordered(names, hexcols, cols, i):
    a = UnorderedAssignment()
    for k in cols:
        a.assign(names[k], hexcols[k][i])
    a.freeze()
    return a


# ---------------------------------------------------------------------------
# Expressions
# ---------------------------------------------------------------------------
class LogicalExpression(ABC):
    # class tag for the hot lowering / planning walks (isinstance through
    # ABCMeta costs ~0.5 us per call): 'n' Node, 'l' Link, 'v' Variable,
    # 'tv' TypedVariable, 't' LinkTemplate, 'a' And, 'o' Or, 'x' Not,
    # 'm' NameMatch
    _k = ''

    @abstractmethod
    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool: ...

    def __repr__(self):
        return '<LogicalExpression>'


class Atom(LogicalExpression, ABC):

    def __init__(self, atom_type: str):
        self.atom_type = atom_type
        self.handle = None

    def __repr__(self):
        return f'{self.atom_type}'

    @abstractmethod
    def get_handle(self, db: DBInterface) -> str: ...


class Node(Atom):
    _k = 'n'

    def __init__(self, node_type: str, node_name: str):
        super().__init__(node_type)
        self.name = node_name

    def __repr__(self):
        return f'<{super().__repr__()}: {self.name}>'

    def get_handle(self, db: DBInterface) -> str:
        if not self.handle:
            self.handle = db.get_node_handle(self.atom_type, self.name)
        return self.handle

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        return db.node_exists(self.atom_type, self.name)


def _variables_last(t1, t2):
    """Link.__init__'s comparator for unordered links (pattern_matcher.py:442-448)."""
    if isinstance(t1, Variable):
        return 1
    if isinstance(t2, Variable):
        return -1
    return 0


class Link(Atom):
    _k = 'l'

    def __init__(self, link_type: str, targets: List[Atom], ordered: bool):
        assert not any(isinstance(target, TypedVariable) for target in targets)
        super().__init__(link_type)
        self.ordered = ordered
        self.targets = targets if ordered else sorted(targets, key=cmp_to_key(_variables_last))

    def __repr__(self):
        return f'<{super().__repr__()}: {self.targets}>'

    def get_handle(self, db: DBInterface) -> str:
        if not self.handle:
            hs = [t.get_handle(db) for t in self.targets]
            if any(h is None for h in hs):
                return None
            self.handle = db.get_link_handle(self.atom_type, hs)
        return self.handle

    def _typed_variable_matched(self, db, answer) -> bool:
        if any(isinstance(t, Variable) for t in self.targets):
            return False
        return all(t.matched(db, answer) for t in self.targets)

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        db = _hip(db)
        if any(isinstance(t, LinkTemplate) for t in self.targets):
            return self._typed_variable_matched(db, answer)
        if not all(t.matched(db, answer) for t in self.targets):
            return False
        handles = [t.get_handle(db) for t in self.targets]
        if WILDCARD not in handles:
            return db.link_exists(self.atom_type, handles)
        var_ids = [_vid(t.name) if isinstance(t, Variable) else None for t in self.targets]
        hint = getattr(self, '_order_var', None)
        if hint is not None:
            rel = db.match_link(self.atom_type, handles, var_ids, self.ordered, CONFIG['no_overload'],
                                order_var=_vid(hint))
        else:
            rel = db.match_link(self.atom_type, handles, var_ids, self.ordered, CONFIG['no_overload'])
        found = db.rel_nonempty(rel)
        if db.tuple_targets and not self.ordered and found and any(v is None for v in var_ids):
            # reference DB path: list.remove on a tuple (pattern_matcher.py:484)
            raise AttributeError("'tuple' object has no attribute 'remove'")
        answer._set(db, rel)
        return found


    def _index_join(self, db, acc):
        """rel_join(acc, this term's relation) through the pattern index, or
        None when the shape does not allow it (And.matched scans instead)."""
        if not self.ordered or CONFIG['no_overload'] or not hasattr(db, 'rel_index_join'):
            return None
        if getattr(db, '_stale', None) and db.touches_stale(self):
            return None                         # the scan adds the stale entries (HipDB.match_link)
        if not all(isinstance(t, Variable) or type(t) is Node for t in self.targets):
            return None
        if any(isinstance(t, TypedVariable) for t in self.targets):
            return None
        handles = [t.get_handle(db) for t in self.targets]
        var_ids = [_vid(t.name) if isinstance(t, Variable) else None for t in self.targets]
        return db.rel_index_join(acc, self.atom_type, handles, var_ids)


class Variable(Atom):
    _k = 'v'

    def __init__(self, variable_name: str):
        super().__init__('ANY')
        self.name = variable_name

    def __repr__(self):
        return f'{self.name}'

    def get_handle(self, db: DBInterface) -> str:
        return WILDCARD

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        return True


class TypedVariable(Variable):
    _k = 'tv'

    def __init__(self, variable_name: str, variable_type: str):
        super().__init__(variable_name)
        self.type = variable_type

    def __repr__(self):
        return f'{self.name}: {self.type}'


class LinkTemplate(LogicalExpression):
    _k = 't'

    def __init__(self, link_type: str, targets: List[TypedVariable], ordered: bool):
        assert all(isinstance(target, TypedVariable) for target in targets)
        self.link_type = link_type
        self.targets = targets
        self.ordered = ordered
        self.handle = None

    def __repr__(self):
        return f'<{self.link_type}: {self.targets}>'

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        db = _hip(db)
        rel = db.match_template(self.link_type, [v.type for v in self.targets],
                                [_vid(v.name) for v in self.targets], self.ordered, CONFIG['no_overload'])
        answer._set(db, rel)
        return db.rel_nonempty(rel)


class NameMatch(LogicalExpression):
    """A variable constrained by the name of the node it binds (no reference
    counterpart; the notebooks loop over get_matched_node_name instead).

    Definition: the term's assignments are {OrderedAssignment{variable: h}}
    for h in db.get_matched_node_name(node_type, pattern) -- re.search of
    the pattern over the names of the nodes of that type -- and matched() is
    True iff there is one; an unknown type has none.  Inside And / Or / Not
    it folds as any term with that assignment set.  The whole-expression
    plan has no leaf for it: an expression that holds one takes the
    per-operator fold (_walk raises _Unsupported).

    Evaluation: HipDB.match_node_names_rel (the matcher's ids as a device
    table), and in And, where the running result already binds the variable
    in ordered tables, HipDB.rel_name_filter instead of scan + join.
    DAS_NAME_TERM=0, or a pattern the DFA compiler declines for the type,
    takes the ids from the host `re` loop; the fold is the same."""
    _k = 'm'

    def __init__(self, variable_name: str, node_type: str, pattern: str):
        self.name = variable_name
        self.node_type = node_type
        self.pattern = pattern
        self.regex = re.compile(pattern)        # an invalid pattern raises re.error here

    def __repr__(self):
        return f'<NameMatch {self.name}: {self.node_type} ~ {self.pattern!r}>'

    @staticmethod
    def _db(db):
        db = _hip(db)
        if not isinstance(db, HipDB):
            raise NotImplementedError("NameMatch on a sharded DB")
        return db

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        db = self._db(db)
        rel = db.match_node_names_rel(self.node_type, self.pattern, _vid(self.name))
        answer._set(db, rel)
        return db.rel_nonempty(rel)

    def _filter(self, db, acc):
        """rel_join(acc, this term's relation) as a filter of acc's rows, or
        None when acc does not bind the variable in ordered tables only
        (And.matched evaluates the term and joins instead)."""
        return self._db(db).rel_name_filter(acc, self.node_type, self.pattern, _vid(self.name))


class Not(LogicalExpression):
    _k = 'x'

    def __init__(self, term: LogicalExpression):
        self.term = term

    def __repr__(self):
        return f'NOT({self.term})'

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        r = _try_plan(self, db, answer)
        if r is not None:
            return r
        self.term.matched(db, answer)
        answer.negation = not answer.negation
        return True


def _nodes_of(expr, out):
    k = expr._k
    if k == 'n':
        out.append(expr)
    elif k == 'l':
        for t in expr.targets:
            _nodes_of(t, out)
    elif k == 'x':
        _nodes_of(expr.term, out)
    elif k == 'a' or k == 'o':
        for t in expr.terms:
            _nodes_of(t, out)
    return out


def _prefetch(expr, db):
    """One batched handle lookup for every grounded node under an And / Or
    (instead of one device round trip per node_exists)."""
    nodes = getattr(expr, '_nodes', None)
    if nodes is None:
        nodes = expr._nodes = _nodes_of(expr, [])
    if nodes:
        db.prefetch_handles([n.get_handle(db) for n in nodes])


class Or(LogicalExpression):
    _k = 'o'

    def __init__(self, terms: List[LogicalExpression]):
        self.terms = terms

    def __repr__(self):
        return f'OR({self.terms})'

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        db = _hip(db)
        if not self.terms:
            return False
        r = _try_plan(self, db, answer)
        if r is not None:
            return r
        _prefetch(self, db)
        union = None
        any_matched = False
        negated = [t for t in self.terms if isinstance(t, Not)]
        for term in self.terms:
            if isinstance(term, Not):
                continue
            sub = PatternMatchingAnswer()
            if not term.matched(db, sub):
                continue
            any_matched = True
            rel = sub._relation()
            if db.rel_nonempty(rel):
                union = rel if union is None else db.rel_union(union, rel)
        union = union if union is not None else db.rel_empty()
        if negated:
            sub = PatternMatchingAnswer()
            And([t.term for t in negated]).matched(db, sub)
            answer._set(db, db.rel_minus(sub._relation(), union))
            answer.negation = True
        else:
            answer._set(db, union)
        return any_matched


class And(LogicalExpression):
    _k = 'a'

    def __init__(self, terms: List[LogicalExpression]):
        self.terms = terms

    def __repr__(self):
        return f'AND({self.terms})'

    def post_process(self, assignment) -> Assignment:
        return assignment

    def _plan_orders(self):
        """Scan-order hints: each positive Link term is asked for its rows
        sorted by its first variable that another term also binds (the join
        key), so joins probe sorted keys.  Answers are unchanged."""
        def names(t):
            if t._k == 'm':
                return [t.name]                 # a NameMatch binds its variable: a join key like any other
            return [x.name for x in t.targets if x._k == 'v' or x._k == 'tv'] if t._k == 'l' else []
        vs = [set(names(t)) for t in self.terms]
        for i, t in enumerate(self.terms):
            if t._k != 'l':
                continue
            others = set().union(*(v for j, v in enumerate(vs) if j != i)) if len(vs) > 1 else set()
            t._order_var = next((n for n in names(t) if n in others), None)

    def matched(self, db: DBInterface, answer: PatternMatchingAnswer) -> bool:
        db = _hip(db)
        if not self.terms:
            return False
        # (the scan-order hints: _walk sets them when it lowers the And, and a
        # query shape seen before needs none)
        r = _try_plan(self, db, answer)
        if r is not None:
            return r
        if not getattr(self, '_planned', False):
            self._plan_orders()
            self._planned = True
        _prefetch(self, db)
        acc = None
        forbidden = []
        for term in self.terms:
            if acc is not None and isinstance(term, Link) and db.rel_nonempty(acc):
                # index join (das_index_join): the term's rows are looked up
                # from the running result's keys instead of scanned; an empty
                # result takes the scan path, which tells a failing term
                # (And -> False) from an empty join (reset-on-empty)
                rel = term._index_join(db, acc)
                if rel is not None and db.rel_nonempty(rel):
                    acc = rel
                    continue
            elif acc is not None and term._k == 'm' and db.rel_nonempty(acc):
                # name filter (das_table_name_filter): where every row binds
                # the term's variable the join keeps a row iff its value is
                # a match; an empty result takes the term's own matched(),
                # which tells "no name of the type matches" (And -> False)
                # from an empty join (reset-on-empty)
                rel = term._filter(db, acc)
                if rel is not None and db.rel_nonempty(rel):
                    acc = rel
                    continue
            sub = PatternMatchingAnswer()
            if not term.matched(db, sub):
                return False
            rel = sub._relation()
            if not db.rel_nonempty(rel):
                continue
            if sub.negation:
                forbidden.append(rel)
                continue
            # reset-on-empty (pattern_matcher.py:725-729): an empty running
            # result takes the next term's assignments as they are
            acc = rel if acc is None or not db.rel_nonempty(acc) else db.rel_join(acc, rel)
        if acc is None:
            acc = db.rel_empty()
        for f in forbidden:
            if db.rel_nonempty(acc):
                acc = db.rel_antijoin(acc, f)
        acc = db.rel_normalize(acc)
        answer._set(db, acc)
        return db.rel_nonempty(acc)
