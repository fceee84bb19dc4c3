"""answer.text / iter_text without a GPU: the row literals
against repr(dict), the rules that send an answer to das_table_rows_text, the
joining of the chunks, the mirrored constants, and das_amd/csrc/rows_text.h --
the size, tile and hex rules host and device share -- run on the host by
tests/native/rows_text_check.cpp, plain and under AddressSanitizer / UBSan (a
stand-alone program: nothing loaded into Python is sanitized)."""
import os
import re
import shutil
import subprocess

import pytest

from das_amd import _lib
from das_amd.pattern_matcher import pattern_matcher as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TRICKY = ["V", "v1", "it's", 'say "hi"', "both ' and \"", "back\\slash", "né", "日本", "tab\there", "", "x" * 300]
HANDLES = ["0" * 32, "af12f10f9ae2002a1607ba0b47ba8407", "f" * 32]


class _T:
    def __init__(self, kind, names, nrows):
        self.kind, self.vars, self.nrows = kind, tuple(pm._vid(n) for n in names), nrows


def _row(lits, handles):
    out = lits[0]
    for h, lit in zip(handles, lits[1:]):
        out += h.encode() + lit
    return out.decode("utf-8")


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_row_literals_are_repr_of_the_mapping(k):
    for shift in range(len(TRICKY)):
        names = [TRICKY[(shift + i) % len(TRICKY)] for i in range(k)]
        if len(set(names)) != k:
            continue
        lits = pm.row_literals(names)
        assert len(lits) == k + 1 and all(isinstance(x, bytes) for x in lits)
        handles = [HANDLES[i % len(HANDLES)] for i in range(k)]
        assert _row(lits, handles) == repr(dict(zip(names, handles)))
        assert _lib.rows_text_size(lits, pm.ROW_SEP, 1) == len(repr(dict(zip(names, handles))).encode("utf-8"))
    with pytest.raises(ValueError):
        pm.row_literals([])


def test_rows_text_size():
    lits = pm.row_literals(["a", "b"])
    row = len(repr({"a": HANDLES[0], "b": HANDLES[1]}))
    assert _lib.rows_text_size(lits, b", ", 0) == 0
    assert _lib.rows_text_size(lits, b", ", 1) == row
    assert _lib.rows_text_size(lits, b", ", 5) == 5 * row + 4 * 2
    assert _lib.rows_text_size(lits, b"", 5) == 5 * row


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "das_mi355x.h")).read()
    stage = int(re.search(r"#define DAS_ROWS_TEXT_STAGE_BYTES (\d+)", src).group(1))
    assert stage == _lib.ROWS_TEXT_STAGE_BYTES
    assert re.search(r"#define DAS_ROWS_TEXT_MAX_ROW \(DAS_ROWS_TEXT_STAGE_BYTES - 16\)", src)
    assert _lib.ROWS_TEXT_MAX_ROW == stage - 16


def test_plan_rules():
    O, U, C = _lib.TABLE_ORDERED, _lib.TABLE_UNORDERED, _lib.TABLE_COMPOSITE
    a, b = _T(O, ["p1", "p2"], 10), _T(O, ["p1", "p3"], 5)
    plan = pm.rows_text_plan([a, _T(O, ["p9"], 0), b])
    assert [t for t, _ in plan] == [a, b]                        # empty tables left out, order kept
    assert plan[0][1] == pm.row_literals(["p1", "p2"])
    assert pm.rows_text_bytes(plan) == len("{" + ", ".join([repr({"p1": HANDLES[0], "p2": HANDLES[0]})] * 10 +
                                                          [repr({"p1": HANDLES[0], "p3": HANDLES[0]})] * 5) + "}")
    assert pm.rows_text_plan([]) is None and pm.rows_text_plan([_T(O, ["p1"], 0)]) is None      # "set()": host
    assert pm.rows_text_plan([a, _T(U, ["p1", "p3"], 5)]) is None
    assert pm.rows_text_plan([a, _T(C, ["p1", "p3"], 5)]) is None
    assert pm.rows_text_plan([a, _T(O, [], 1)]) is None
    assert pm.rows_text_plan([a, _T(O, ["p2", "p1"], 3)]) is None                               # equal variable sets
    assert pm.rows_text_plan([a, _T(U, ["p1", "p3"], 0)]) is not None                           # ... but it is empty
    assert pm.rows_text_plan([a, b], min_rows=15) is not None and pm.rows_text_plan([a, b], min_rows=16) is None
    size = pm.rows_text_bytes(plan)
    assert pm.rows_text_plan([a, b], max_bytes=size) is not None
    assert pm.rows_text_plan([a, b], max_bytes=size - 1) is None
    # a row and its separator at the limit, and one byte beyond
    base = _lib.rows_text_size(pm.row_literals([""]), pm.ROW_SEP, 1) + len(pm.ROW_SEP)
    fits = "n" * (_lib.ROWS_TEXT_MAX_ROW - base)
    assert pm.rows_text_plan([_T(O, [fits], 2)]) is not None
    assert pm.rows_text_plan([_T(O, [fits + "n"], 2)]) is None


def test_iter_joins_chunks_and_tables():
    O = _lib.TABLE_ORDERED
    a, b = _T(O, ["q1"], 5), _T(O, ["q2"], 3)
    plan = pm.rows_text_plan([a, b])
    calls = []

    def render(t, lits, row0, n):
        calls.append((t, row0, n))
        return ", ".join(f"<{pm._var_name(t.vars[0])}:{r}>" for r in range(row0, row0 + n))

    want = "{" + ", ".join([f"<q1:{r}>" for r in range(5)] + [f"<q2:{r}>" for r in range(3)]) + "}"
    for chunk in (1, 2, 3, 5, 100):
        calls.clear()
        pieces = list(pm.iter_rows_text(plan, chunk, render))
        assert "".join(pieces) == want
        assert pieces[0] == "{" and pieces[-1] == "}" and len(pieces) == len(calls) + 2
        assert calls == [(t, r0, min(chunk, t.nrows - r0)) for t in (a, b) for r0 in range(0, t.nrows, chunk)]


def test_hand_set_and_empty_answers_take_the_host_path():
    ans = pm.PatternMatchingAnswer()
    assert ans.text() == "set()" and list(ans.iter_text()) == ["set()"]
    x = pm.OrderedAssignment()
    x.assign("V", HANDLES[1])
    x.freeze()
    ans.assignments = {x}
    assert ans.text() == "{" + repr({"V": HANDLES[1]}) + "}" == str(ans.assignments)
    assert "".join(ans.iter_text(chunk_rows=1)) == ans.text()
    with pytest.raises(ValueError):
        list(ans.iter_text(chunk_rows=0))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_rows_text_header_on_the_host(tmp_path, flags):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "rows_text_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe,
                    os.path.join(HERE, "native", "rows_text_check.cpp")], check=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
    assert out.split() == ["ok", "stage", str(_lib.ROWS_TEXT_STAGE_BYTES), "max_row", str(_lib.ROWS_TEXT_MAX_ROW)]
