"""das_amd.name_search: node-name regex -> byte DFA, against `re` itself.
Host code only (the device matcher walks the same table: test_gpu_name_search.py)."""
import os
import re
import time

import numpy as np
import pytest

from das_amd import _lib, loader
from das_amd.name_search import MAX_STATES, MAX_TABLE, NameDFA, compile_name_pattern
from tests import name_search_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = C.names()
ASCII_NAMES = [n for n in NAMES if C.is_plain_ascii(n)]
ENC = {n: n.encode("utf-8") for n in NAMES}


def simulate(dfa: NameDFA, data: bytes) -> bool:
    """Feed the UTF-8 bytes, then the end-of-name class once."""
    s = dfa.start
    for b in data:
        s = int(dfa.next[s * dfa.n_classes + int(dfa.byte_class[b])])
        assert s < dfa.n_states
    s = int(dfa.next[s * dfa.n_classes + dfa.eot_class])
    return bool(dfa.accept[s])


def check_shape(dfa):
    assert 1 <= dfa.n_states <= MAX_STATES
    assert dfa.n_states * dfa.n_classes <= MAX_TABLE
    assert dfa.start < dfa.n_states and dfa.eot_class < dfa.n_classes
    assert dfa.byte_class.dtype == np.uint8 and dfa.byte_class.shape == (256,)
    assert dfa.next.dtype == np.uint16 and dfa.next.shape == (dfa.n_states * dfa.n_classes,)
    assert dfa.accept.dtype == np.uint8 and dfa.accept.shape == (dfa.n_states,)
    assert int(dfa.byte_class.max()) < dfa.n_classes
    assert int(dfa.next.max()) < dfa.n_states
    # accepting states are absorbing: the kernel stops at the first one
    rows = dfa.next.reshape(dfa.n_states, dfa.n_classes)
    for s in np.nonzero(dfa.accept)[0]:
        assert dfa.accept[rows[s]].all()


def test_names_cover_the_cases():
    assert "" in NAMES and "a\n" in NAMES and "é" in NAMES and "٣" in NAMES
    assert any(len(ENC[n]) == 300 for n in NAMES)
    assert len(NAMES) > 2000 and len(ASCII_NAMES) > 2000 and len(ASCII_NAMES) < len(NAMES)


@pytest.mark.parametrize("pattern", C.MUST_COMPILE_ASCII)
def test_must_compile_ascii(pattern):
    dfa = compile_name_pattern(pattern, ascii_only=True)
    assert dfa is not None
    check_shape(dfa)


@pytest.mark.parametrize("pattern", C.MUST_COMPILE_ANY)
def test_must_compile_any_names(pattern):
    dfa = compile_name_pattern(pattern, ascii_only=False)
    assert dfa is not None
    check_shape(dfa)


@pytest.mark.parametrize("pattern", C.DECLINE_NON_ASCII)
def test_declines_without_the_ascii_promise(pattern):
    assert compile_name_pattern(pattern, ascii_only=False) is None
    assert compile_name_pattern(pattern, ascii_only=True) is not None


@pytest.mark.parametrize("pattern", C.DECLINE_ALWAYS)
def test_declines_always(pattern):
    t0 = time.perf_counter()
    assert compile_name_pattern(pattern, ascii_only=True) is None
    assert compile_name_pattern(pattern, ascii_only=False) is None
    # (a|b)*a(a|b){16} needs > 2^16 states: the subset construction stops at the cap
    assert time.perf_counter() - t0 < 5.0


@pytest.mark.parametrize("pattern", C.ALL_PATTERNS)
def test_dfa_equals_re_search(pattern):
    rx = re.compile(pattern)
    a = compile_name_pattern(pattern, ascii_only=True)
    if a is not None:
        check_shape(a)
        for n in ASCII_NAMES:
            assert simulate(a, ENC[n]) == bool(rx.search(n)), (pattern, n)
            assert a.matches(ENC[n]) == bool(rx.search(n))
    u = compile_name_pattern(pattern, ascii_only=False)
    if u is not None:
        assert a is not None            # byte-safe for any names: byte-safe for ASCII names
        check_shape(u)
        for n in NAMES:
            assert simulate(u, ENC[n]) == bool(rx.search(n)), (pattern, n)


def test_escaped_names_match_exactly():
    """'^' + re.escape(name) + '$' (the GPU test's probe of the heap bytes);
    `$` is not byte-safe, so names outside ASCII are probed with \\Z."""
    for n in ["a", "a.b", "n17", "x y", "é", "naïve", "a" * 40]:
        p = "^" + re.escape(n) + ("$" if C.is_plain_ascii(n) else r"\Z")
        dfa = compile_name_pattern(p, ascii_only=C.is_plain_ascii(n))
        assert dfa is not None, p
        for m in NAMES + [n]:
            if C.is_plain_ascii(n) and not C.is_plain_ascii(m):
                continue
            assert simulate(dfa, m.encode("utf-8")) == bool(re.search(p, m)), (p, m)


def test_invalid_pattern_raises_re_error():
    for ascii_only in (True, False):
        with pytest.raises(re.error):
            compile_name_pattern("(", ascii_only=ascii_only)


def test_limits_match_the_header():
    src = open(os.path.join(ROOT, "include", "das_mi355x.h")).read()
    assert int(re.search(r"#define DAS_NAME_DFA_MAX_STATES (\d+)", src).group(1)) == MAX_STATES
    assert int(re.search(r"#define DAS_NAME_DFA_MAX_TABLE (\d+)", src).group(1)) == MAX_TABLE
    assert int(re.search(r"#define DAS_NAME_STAGE_BYTES (\d+)", src).group(1)) == _lib.NAME_STAGE_BYTES


def test_over_the_table_declines():
    # a literal longer than the state cap
    assert compile_name_pattern("a" * (MAX_STATES + 1), ascii_only=True) is None
    assert compile_name_pattern("a" * 100, ascii_only=True) is not None


def _node_leaves(arrays):
    return [i for i in range(arrays.n_leaf) if arrays.leaf_kind[i] == loader.LEAF_NODE]


@pytest.mark.parametrize("reader", ["metta", "canonical", "native"])
def test_name_start_is_type_name_plus_one(reader):
    """The device heap derives a name's start inside its "Type name" leaf as
    len(type name) + 1; AtomArrays.node_name() uses name_start: the two agree
    on every loader."""
    canonical = ('(: Concept Type)\n(: Vé Type)\n(: Inheritance Type)\n(: "a" Concept)\n(: "naïve b" Vé)\n'
                 '(: "long name x" Concept)\n(Inheritance "Concept a" "Vé naïve b")\n'
                 '(Inheritance "Concept long name x" "Concept a")\n')
    metta = ('(: Concept Type)\n(: Vé Type)\n(: Inheritance Type)\n(: "a" Concept)\n(: "naïve b" Vé)\n'
             '(: "long name x" Concept)\n(Inheritance "a" "naïve b")\n(Inheritance "long name x" "a")\n')
    if reader == "metta":
        arrays = loader.parse_metta(metta).finish()
    elif reader == "canonical":
        arrays = loader.parse_canonical(canonical).finish()
    else:
        arrays = _lib.parse_canonical(canonical)
    nodes = _node_leaves(arrays)
    assert len(nodes) == 3
    seen = set()
    for i in nodes:
        whole = bytes(arrays.leaf_bytes[int(arrays.leaf_off[i]):int(arrays.leaf_off[i + 1])]).decode("utf-8")
        # the node's named type, as the index build finds it: through its composite-type leaf
        t = arrays.type_names[int(arrays.leaf_type_id[int(arrays.leaf_ctype[i])])]
        assert whole.startswith(t + " ")
        assert int(arrays.name_start[i]) == len(t.encode("utf-8")) + 1
        assert arrays.node_name(i) == whole[len(t) + 1:]
        seen.add(arrays.node_name(i))
    assert seen == {"a", "naïve b", "long name x"}
