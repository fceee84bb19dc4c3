"""Node-name regex -> byte DFA for the device matcher (das_match_node_names).

`get_matched_node_name(node_type, pattern)` is `re.search(pattern, name)` over
the names of one node type (redis_mongo_db.py:287-293).  For the regular part
of Python's syntax that yes/no answer is membership in a regular language, so
it can be decided by a table walk over the name's UTF-8 bytes: the pattern is
parsed with the parser `re` itself uses, turned into an NFA over bytes and
determinised.  The unanchored search is part of the automaton (a self-loop on
every byte before the pattern; a match found before the end of the name leads
to one absorbing accepting state), so the kernel knows nothing about regex:
it feeds the bytes, then the end-of-name symbol once, and reports whether the
state it ends in accepts.

Exactness.  A `str` pattern matches code points, the walk sees bytes.  Each
construct is therefore classified:

  byte-safe   literals (their UTF-8 bytes; UTF-8 is self-synchronising, so a
              bytewise literal match is a code-point match), positive classes
              whose members are all ASCII, `^`, `\\A`, `\\Z`, repeats,
              alternation, groups;
  ASCII-only  `.`, `\\d` `\\w` `\\s` and their negations (they match non-ASCII
              code points: `re.search(r'\\d', '\\u0663')` is true), negated
              classes and NOT_LITERAL (one code point, not one byte), classes
              with a non-ASCII member, and `$` (it also matches before a
              trailing newline).

A pattern that uses an ASCII-only construct compiles only with
`ascii_only=True`: the caller's promise that every byte of every name it will
be run on is below 0x80 and is not a newline.  Under that promise the ASCII
restriction of each construct is its exact meaning.  Everything else --
back-references, look-around, word boundaries, any flag but the default
re.UNICODE, possessive repeats and atomic groups, automata over the state cap
-- returns None and the caller matches on the host.
"""
import re
from typing import NamedTuple, Optional

import numpy as np

try:                                    # Python >= 3.11
    import re._parser as _sre_parse
    import re._constants as _sre
except ImportError:                     # Python <= 3.10
    import sre_parse as _sre_parse
    import sre_constants as _sre

# limits of the device matcher (include/das_mi355x.h)
MAX_STATES = 1024                       # DAS_NAME_DFA_MAX_STATES
MAX_TABLE = 8192                        # DAS_NAME_DFA_MAX_TABLE: n_states * n_classes
MAX_NFA = 4096                          # NFA states a pattern may expand to (bounded repeats are unrolled)

_ASCII = (1 << 128) - 1
_NL = 1 << 0x0A
_ALL = (1 << 256) - 1


def _ascii_set(category_pattern):
    """The ASCII bytes a one-character pattern matches, asked of `re` itself."""
    rx = re.compile(category_pattern)
    m = 0
    for c in range(128):
        if rx.match(chr(c)):
            m |= 1 << c
    return m


_CATEGORY = {
    _sre.CATEGORY_DIGIT: _ascii_set(r"\d"),
    _sre.CATEGORY_SPACE: _ascii_set(r"\s"),
    _sre.CATEGORY_WORD: _ascii_set(r"\w"),
}
_NOT_CATEGORY = {
    _sre.CATEGORY_NOT_DIGIT: _sre.CATEGORY_DIGIT,
    _sre.CATEGORY_NOT_SPACE: _sre.CATEGORY_SPACE,
    _sre.CATEGORY_NOT_WORD: _sre.CATEGORY_WORD,
}

# epsilon-edge conditions
_ALWAYS, _AT_START, _AT_END = 0, 1, 2


class NameDFA(NamedTuple):
    """next[s * n_classes + c]: the state after class c in state s; the class
    of byte b is byte_class[b], the end of the name is class eot_class.
    Accepting states are absorbing."""
    n_states: int
    n_classes: int
    start: int
    eot_class: int
    byte_class: np.ndarray              # uint8[256]
    next: np.ndarray                    # uint16[n_states * n_classes]
    accept: np.ndarray                  # uint8[n_states]

    def matches(self, data: bytes) -> bool:
        """The table walk the device kernel does (tests, documentation)."""
        s, k = self.start, self.n_classes
        for b in data:
            s = int(self.next[s * k + self.byte_class[b]])
        return bool(self.accept[int(self.next[s * k + self.eot_class])])


# One accepting state and one class: every name matches (HipDB.get_all_nodes
# lists a type's node ids through the matcher with it).
ACCEPT_ALL = NameDFA(1, 1, 0, 0, np.zeros(256, dtype=np.uint8), np.zeros(1, dtype=np.uint16),
                     np.ones(1, dtype=np.uint8))


class _Decline(Exception):
    pass


class _NFA:
    """Thompson construction: byte edges carry a 256-bit set, epsilon edges a
    condition (always / only before the first byte / only after the last)."""

    def __init__(self, ascii_only):
        self.ascii_only = ascii_only
        self.byte_edges = []            # per state: [(mask, target)]
        self.eps = []                   # per state: [(condition, target)]

    def state(self):
        if len(self.eps) >= MAX_NFA:
            raise _Decline
        self.byte_edges.append([])
        self.eps.append([])
        return len(self.eps) - 1

    def need_ascii(self):
        if not self.ascii_only:
            raise _Decline

    # every builder returns the state reached after the fragment, given the state before it
    def seq(self, items, a):
        for op, av in items:
            a = self.node(op, av, a)
        return a

    def byte_set(self, mask, a):
        if not mask:
            return self.state()         # matches nothing: an unreachable continuation
        b = self.state()
        self.byte_edges[a].append((mask, b))
        return b

    def literal(self, cp, a):
        try:
            enc = chr(cp).encode("utf-8")
        except UnicodeEncodeError:      # a lone surrogate: no name holds one
            raise _Decline
        for byte in enc:
            a = self.byte_set(1 << byte, a)
        return a

    def class_mask(self, items):
        negate, mask = False, 0
        for op, av in items:
            if op is _sre.NEGATE:
                negate = True
            elif op is _sre.LITERAL:
                if av < 128:
                    mask |= 1 << av
                else:
                    self.need_ascii()   # never matches an ASCII name
            elif op is _sre.RANGE:
                lo, hi = av
                if hi >= 128:
                    self.need_ascii()
                for c in range(lo, min(hi, 127) + 1):
                    mask |= 1 << c
            elif op is _sre.CATEGORY:
                self.need_ascii()
                if av in _CATEGORY:
                    mask |= _CATEGORY[av]
                elif av in _NOT_CATEGORY:
                    mask |= _ASCII & ~_CATEGORY[_NOT_CATEGORY[av]]
                else:
                    raise _Decline
            else:
                raise _Decline
        if negate:
            self.need_ascii()
            mask = _ASCII & ~mask
        return mask

    def repeat(self, lo, hi, sub, a):
        for _ in range(lo):
            a = self.seq(sub, a)
        if hi == _sre.MAXREPEAT:
            # a -> (sub)* -> out
            loop, out = self.state(), self.state()
            self.eps[a].append((_ALWAYS, loop))
            end = self.seq(sub, loop)
            self.eps[end].append((_ALWAYS, loop))
            self.eps[loop].append((_ALWAYS, out))
            return out
        out = self.state()
        self.eps[a].append((_ALWAYS, out))
        for _ in range(hi - lo):
            a = self.seq(sub, a)
            self.eps[a].append((_ALWAYS, out))
        return out

    def node(self, op, av, a):
        if op is _sre.LITERAL:
            return self.literal(av, a)
        if op is _sre.NOT_LITERAL:
            self.need_ascii()
            return self.byte_set(_ASCII & ~(1 << av) if av < 128 else _ASCII, a)
        if op is _sre.ANY:
            self.need_ascii()
            return self.byte_set(_ASCII & ~_NL, a)
        if op is _sre.IN:
            return self.byte_set(self.class_mask(av), a)
        if op is _sre.BRANCH:
            out = self.state()
            for alt in av[1]:
                self.eps[self.seq(alt, a)].append((_ALWAYS, out))
            return out
        if op is _sre.SUBPATTERN:
            _group, add_flags, del_flags, sub = av
            if add_flags or del_flags:
                raise _Decline
            return self.seq(sub, a)
        if op is _sre.MAX_REPEAT or op is _sre.MIN_REPEAT:
            lo, hi, sub = av
            return self.repeat(lo, hi, sub, a)
        if op is _sre.AT:
            if av is _sre.AT_BEGINNING or av is _sre.AT_BEGINNING_STRING:
                cond = _AT_START
            elif av is _sre.AT_END_STRING:
                cond = _AT_END
            elif av is _sre.AT_END:
                self.need_ascii()       # `$` also matches before a trailing newline
                cond = _AT_END
            else:
                raise _Decline
            b = self.state()
            self.eps[a].append((cond, b))
            return b
        raise _Decline

    def closure(self, states, at_start, at_end):
        seen = set(states)
        stack = list(states)
        while stack:
            s = stack.pop()
            for cond, t in self.eps[s]:
                if cond == _AT_START and not at_start:
                    continue
                if cond == _AT_END and not at_end:
                    continue
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _byte_classes(masks):
    """Bytes that no edge set tells apart share a class."""
    sig = [0] * 256
    for i, m in enumerate(masks):
        for b in range(256):
            if m >> b & 1:
                sig[b] |= 1 << i
    ids = {}
    byte_class = np.zeros(256, dtype=np.uint8)
    rep = []                            # one byte of each class
    for b in range(256):
        k = ids.get(sig[b])
        if k is None:
            k = ids[sig[b]] = len(rep)
            rep.append(b)
        byte_class[b] = k
    return byte_class, rep


def compile_name_pattern(pattern: str, *, ascii_only: bool) -> Optional[NameDFA]:
    """The DFA deciding `bool(re.search(pattern, name))` from the UTF-8 bytes
    of `name`, or None where that cannot be guaranteed (module docstring).
    `ascii_only`: every byte of every name is < 0x80 and not a newline.
    An invalid pattern raises re.error, as re.compile does."""
    re.compile(pattern)
    if not isinstance(pattern, str):
        return None
    parsed = _sre_parse.parse(pattern)
    state = getattr(parsed, "state", None) or getattr(parsed, "pattern")
    if state.flags != _sre.SRE_FLAG_UNICODE:
        return None
    nfa = _NFA(ascii_only)
    try:
        loop = nfa.state()              # the search: any prefix is skipped here
        nfa.byte_edges[loop].append((_ALL, loop))
        first = nfa.state()
        nfa.eps[loop].append((_ALWAYS, first))
        final = nfa.seq(parsed, first)
    except _Decline:
        return None

    masks = sorted({m for edges in nfa.byte_edges for m, _ in edges})
    byte_class, rep = _byte_classes(masks)
    n_classes = len(rep) + 1
    eot = len(rep)
    cap = min(MAX_STATES, MAX_TABLE // n_classes)

    # states 0 and 1: the absorbing accept and the dead state (after the end of a name that did not match)
    ACC, DEAD = 0, 1
    rows = [[ACC] * n_classes, [DEAD] * n_classes]
    start_set = nfa.closure([loop], True, False)
    if final in start_set:
        start = ACC
    else:
        # a DFA state: (NFA states, still before the first byte)
        ids = {(start_set, True): 2}
        order = [(start_set, True)]
        rows.append(None)
        start = 2
        i = 0
        while i < len(order):
            cur, pos0 = order[i]
            row = []
            for c in range(n_classes - 1):
                b = rep[c]
                moved = {t for s in cur for m, t in nfa.byte_edges[s] if m >> b & 1}
                nxt = nfa.closure(moved, False, False)
                if final in nxt:
                    row.append(ACC)
                    continue
                key = (nxt, False)
                k = ids.get(key)
                if k is None:
                    k = ids[key] = len(rows)
                    if k >= cap:
                        return None     # over the device table: abort here, not after 2^n states
                    rows.append(None)
                    order.append(key)
                row.append(k)
            row.append(ACC if final in nfa.closure(cur, pos0, True) else DEAD)
            rows[2 + i] = row
            i += 1
    n_states = len(rows)
    accept = np.zeros(n_states, dtype=np.uint8)
    accept[ACC] = 1
    return NameDFA(n_states, n_classes, start, eot, byte_class,
                   np.array(rows, dtype=np.uint16).reshape(-1), accept)
