"""Atom documents in bulk, the parts that need no GPU: the text rules of
das_amd/csrc/json_text.h against json.dumps (a stand-alone native program,
also under the address and undefined-behaviour sanitizers), and the size rule
of docs.hip -- a piece takes A + 4 d L bytes at indent depth d -- restated in
Python and rendered from offsets alone, against json.dumps(..., indent=4)."""
import json
import os
import re
import shutil
import struct
import subprocess

import pytest

from das_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ----------------------------------------------------------------- json_text.h
def _good_names():
    names = [chr(c) for c in range(0x80)]
    names += [f"ab{chr(c)}cd" for c in range(0x80)]
    edges = [chr(c) for c in (0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF)]
    names += edges + [f"x{e}y" for e in edges] + ["".join(edges), "é٣", "naïve", ""]
    names.append("".join(chr(c) for c in range(0x80)) * 3 + "".join(edges) * 5 + 'path/to "q" \\ end\n\t' * 40)
    return [n.encode("utf-8") for n in names]


MALFORMED = {
    "overlong 2": b"\xc0\xaf", "overlong 2 (C1)": b"\xc1\xbf", "overlong 3": b"\xe0\x80\xaf",
    "overlong 4": b"\xf0\x80\x80\xaf", "surrogate high": b"\xed\xa0\x80", "surrogate low": b"\xed\xbf\xbf",
    "above U+10FFFF": b"\xf4\x90\x80\x80", "F5 lead": b"\xf5\x80\x80\x80", "FF": b"\xff",
    "stray continuation": b"a\x80b", "truncated 2": b"ab\xc3", "truncated 3": b"\xe2\x82",
    "truncated 4": b"\xf0\x9f\x98",
    "bad continuation": b"\xe2\x28\xa1", "lead then ASCII": b"\xc3(",
}


def _run_check(exe, tmp_path, names):
    src = tmp_path / "names.bin"
    src.write_bytes(b"".join(struct.pack("<I", len(n)) + n for n in names))
    r = subprocess.run([exe, str(src)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split(b"\n")
    assert lines[-1] == b"" and len(lines) == len(names) + 1
    out = []
    for line in lines[:-1]:
        bad, n, text = line.split(b" ", 2)
        assert int(n) == len(text)
        out.append((int(bad), text))
    return out


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_json_text_header_on_the_host(tmp_path, flags):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "json_text_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe,
                    os.path.join(HERE, "native", "json_text_check.cpp")], check=True, timeout=300)
    good = _good_names()
    for name, (bad, text) in zip(good, _run_check(exe, tmp_path, good)):
        assert bad == 0, name
        assert text == json.dumps(name.decode("utf-8"))[1:-1].encode("ascii"), name
    for (what, name), (bad, _) in zip(MALFORMED.items(), _run_check(exe, tmp_path, list(MALFORMED.values()))):
        with pytest.raises(UnicodeDecodeError):
            name.decode("utf-8")
        assert bad > 0, what


def test_depth_limit_matches_the_header():
    src = open(os.path.join(ROOT, "include", "das_mi355x.h")).read()
    assert int(re.search(r"#define DAS_DOC_MAX_DEPTH (\d+)", src).group(1)) == _lib.DOC_MAX_DEPTH


# --------------------------------------------------------------- the size rule
def _piece(doc):
    """(A, L) of a document's piece (its indentation and itself): it takes
    A + 4 d L bytes at indent depth d; L is its number of lines."""
    t = len(json.dumps(doc["type"]))
    if "name" in doc:
        # {\n | "type": T,\n | "name": "..."\n | }   at d, d + 1, d + 1, d
        return 8 + len('{\n"type": ,\n"name": ""\n}') + t + len(json.dumps(doc["name"])) - 2, 4
    kids = doc["targets"]
    if not kids:
        return 8 + len('{\n"type": ,\n"targets": []\n}') + t, 4
    # {\n | "type": T,\n | "targets": [\n | children two deeper, ",\n" between, "\n" after | ]\n | }
    a, lines = 12 + len('{\n"type": ,\n"targets": [\n]\n}') + t + 2 * len(kids) - 1, 5
    for ca, cl in map(_piece, kids):
        a += ca + 8 * cl
        lines += cl
    return a, lines


def _size(doc, d):
    a, lines = _piece(doc)
    return a + 4 * d * lines


def _put(out, at, text):
    assert all(b == 0 for b in out[at:at + len(text)]), "a byte written twice"
    out[at:at + len(text)] = text
    return at + len(text)


def _write(doc, d, out, at, sep):
    """The item's own fragments from `at`; children at offsets that come from sizes alone."""
    ind, ind1 = b" " * (4 * d), b" " * (4 * (d + 1))
    p = _put(out, at, ind + b"{\n" + ind1 + b'"type": ' + json.dumps(doc["type"]).encode() + b",\n" + ind1)
    if "name" in doc:
        p = _put(out, p, b'"name": ' + json.dumps(doc["name"]).encode() + b"\n")
    elif not doc["targets"]:
        p = _put(out, p, b'"targets": []\n')
    else:
        p = _put(out, p, b'"targets": [\n')
        kids = doc["targets"]
        for k, kid in enumerate(kids):
            s = b",\n" if k + 1 < len(kids) else b"\n"
            _write(kid, d + 2, out, p, s)
            p += _size(kid, d + 2) + len(s)
        p = _put(out, p, ind1 + b"]\n")
    p = _put(out, p, ind + b"}" + sep)
    assert p == at + _size(doc, d) + len(sep)


def _render(docs, as_list):
    if not as_list:
        out = bytearray(_size(docs, 0))
        _write(docs, 0, out, 0, b"")
        return bytes(out)
    if not docs:
        return b"[]"
    seps = [b",\n"] * (len(docs) - 1) + [b"\n"]
    out = bytearray(2 + sum(_size(doc, 1) + len(s) for doc, s in zip(docs, seps)) + 1)
    p = _put(out, 0, b"[\n")
    for doc, s in zip(docs, seps):
        _write(doc, 1, out, p, s)
        p += _size(doc, 1) + len(s)
    _put(out, p, b"]")
    return bytes(out)


def _node(name="n", type_="Concept"):
    return {"type": type_, "name": name}


def _link(kids, type_="Similarity"):
    return {"type": type_, "targets": list(kids)}


def _nested(depth):
    doc = _node("leaf")
    for k in range(depth):
        doc = _link([_node(f"n{k}"), doc], f"T{k}")
    return doc


CASES = {
    "node": _node(), "escaped name": _node('a"b\\c\né\U00010000'), "arity 0": _link([]),
    "null type": _link([_node("x", None), _link([], None)], None),
    **{f"arity {k}": _link([_node(f"n{i}") for i in range(k)]) for k in (1, 2, 3, 9)},
    **{f"nesting {k}": _nested(k) for k in (1, 2, 3, 4, 5)},
    "links of links": _link([_link([_link([]), _node()]), _link([_node("a"), _node("b"), _node("c")])]),
}


@pytest.mark.parametrize("what", list(CASES))
def test_size_rule_renders_what_json_dumps_writes(what):
    doc = CASES[what]
    assert _render(doc, False).decode("ascii") == json.dumps(doc, sort_keys=False, indent=4)
    for docs in ([doc], [doc, _node("other"), doc], [_link([]), doc]):
        assert _render(docs, True).decode("ascii") == json.dumps(docs, sort_keys=False, indent=4)


def test_size_rule_empty_list():
    assert _render([], True).decode("ascii") == json.dumps([], sort_keys=False, indent=4)
