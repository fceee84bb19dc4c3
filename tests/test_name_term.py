"""NameMatch, the node-name regex term of the pattern language, on the CPU: the
value object, that the whole-expression plan declines every expression that
holds one (they take the per-operator fold), and the two C entry points in the
header and the binding's export list."""
import os
import re

import pytest

from das_amd import _lib
from das_amd.pattern_matcher import pattern_matcher as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _link():
    return pm.Link("Inheritance", [pm.Variable("V1"), pm.Variable("V2")], True)


def test_constructor_and_repr():
    t = pm.NameMatch("V2", "Verbatim", r"^mus\d\d\d$")
    assert isinstance(t, pm.LogicalExpression)
    assert (t.name, t.node_type, t.pattern) == ("V2", "Verbatim", r"^mus\d\d\d$")
    assert t._k not in {c._k for c in (pm.Node, pm.Link, pm.Variable, pm.TypedVariable, pm.LinkTemplate, pm.And,
                                       pm.Or, pm.Not)}
    r = repr(t)
    assert "NameMatch" in r and "V2" in r and "Verbatim" in r and repr(r"^mus\d\d\d$") in r
    assert repr(pm.And([_link(), t])).startswith("AND(")


def test_invalid_pattern_raises_in_the_constructor():
    with pytest.raises(re.error):
        pm.NameMatch("V1", "Concept", "(")


@pytest.mark.parametrize("expr", [
    lambda: pm.And([_link(), pm.NameMatch("V2", "Concept", "ma")]),
    lambda: pm.Or([_link(), pm.NameMatch("V2", "Concept", "ma")]),
    lambda: pm.Not(pm.NameMatch("V2", "Concept", "ma")),
    lambda: pm.NameMatch("V2", "Concept", "ma"),
    lambda: pm.And([_link(), pm.Or([_link(), pm.Not(pm.NameMatch("V1", "Concept", "ma"))])]),
], ids=["and", "or", "not", "root", "nested"])
def test_the_plan_declines_the_term(expr):
    with pytest.raises(pm._Unsupported):
        pm._walk(expr(), [], [])
    with pytest.raises(pm._NoShape):
        pm._shape(expr(), [])


def test_the_term_holds_no_node_and_is_a_join_key():
    t = pm.NameMatch("V2", "Concept", "ma")
    link = _link()
    e = pm.And([link, t])
    assert pm._nodes_of(e, []) == []
    e._plan_orders()
    assert link._order_var == "V2"              # the link's rows are asked for sorted by the shared variable


def test_non_relational_db_raises_what_the_links_raise():
    with pytest.raises(TypeError):
        pm.NameMatch("V1", "Concept", "ma").matched(object(), pm.PatternMatchingAnswer())


def test_header_and_export_list_hold_the_two_calls():
    src = open(os.path.join(ROOT, "include", "das_mi355x.h")).read()
    for name in ("das_scan_node_names", "das_table_name_filter"):
        assert re.search(r"^int\s+" + name + r"\(", src, re.M), name
        assert name in _lib.exported_symbols()
    for name, v in (("AUTO", 0), ("WALK", 1), ("FLAGS", 2)):
        assert re.search(rf"#define DAS_NAME_FILTER_{name} {v}\b", src)
        assert getattr(_lib, "NAME_FILTER_" + name) == v
