"""das_amd.miner's per-call loops (halo_host, pattern_counts_host) against a
literal restatement of notebooks/SimplePatternMiner.ipynb cells 6 and 5, over
the oracle's DB-path restatement: the loops are the definition the device
path (tests/test_gpu_miner.py) is held to."""
import json
import os

import pytest

import bench
from das_amd import miner, synthetic
from das_amd.expression_hasher import ExpressionHasher
from oracle import das_oracle as O

W = "*"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def notebook_halo(das, seed_handles, halo_length):
    """Cell 6: cumulative node_handle_list, every template around every node
    handle, then `difference(all_links)` level by level."""
    node_handle_list = set(seed_handles)
    links = [set() for _ in range(halo_length)]
    for level in range(halo_length):
        new_level_node_handles = set()
        for node_handle in node_handle_list:
            template_list = [[node_handle, W], [W, node_handle], [node_handle, W, W], [W, node_handle, W],
                             [W, W, node_handle]]
            for template in template_list:
                link_list = set(das.get_links(None, None, template))
                for link in link_list:
                    for h in das.get_link_targets(link):
                        new_level_node_handles.add(h)
                links[level].update(link_list)
        node_handle_list.update(new_level_node_handles)
    all_links = set()
    for level in range(halo_length):
        if level == 0:
            all_links = set(links[level])
        else:
            links[level] = links[level].difference(all_links)
            all_links.update(links[level])
    return links, len(all_links)


def notebook_build_patterns(das, links):
    """Cell 5's build_patterns: {composite_hash(template): count}; a link of
    another arity contributes nothing (the notebook raises there)."""
    pattern_count = {}
    for link in links:
        targets = das.get_link_targets(link)
        link_type = das.get_link_type(link)
        if len(targets) == 2:
            templates = [[link_type, W, targets[1]], [link_type, targets[0], W]]
        elif len(targets) == 3:
            templates = [[link_type, W, targets[1], targets[2]], [link_type, targets[0], W, targets[2]],
                         [link_type, targets[0], targets[1], W], [link_type, W, W, targets[2]],
                         [link_type, W, targets[1], W], [link_type, targets[0], W, W]]
        else:
            continue
        for template in templates:
            try:                                    # build_pattern_from_template
                for t in template[1:]:
                    if t != W:
                        das.get_node_type(t)
                        das.get_node_name(t)
            except Exception:
                continue
            pattern_count[ExpressionHasher.composite_hash(template)] = len(das.get_links(template[0], None,
                                                                                         template[1:]))
    return pattern_count


def _animals():
    with open(os.path.join(GOLDEN, "kb_animals.json")) as f:
        d = json.load(f)
    kb = O.KB.from_tables(d["nodes"], d["links"])
    seeds = [h for h, t, n in d["nodes"] if n in ("mammal", "human")]
    return kb, seeds


def _similarity():
    kb = O.KB.from_arrays(synthetic.similarity_kb())
    return kb, sorted(kb.nodes)[:3]


def _flybase():
    kb = O.KB.from_arrays(synthetic.flybase_kb(400, 10, 600, n_loc=30, n_do=40))
    gene = next(h for h, (t, n) in sorted(kb.nodes.items()) if t == "Verbatim" and n == "FBgn0000007")
    return kb, [gene]


KBS = {"animals": _animals, "similarity": _similarity, "flybase": _flybase}


@pytest.fixture(scope="module", params=list(KBS))
def case(request):
    kb, seeds = KBS[request.param]()
    das = bench.OracleFacade(O.RedisMongoSemantics(kb))
    want_links, want_universe = notebook_halo(das, seeds, 2)
    return das, seeds, want_links, want_universe


def test_halo_host_is_the_notebook(case):
    das, seeds, want_links, want_universe = case
    halo = miner.halo_host(das, seeds + seeds[:1] + ["0" * 32], 2)        # a repeat and an unknown handle
    assert len(halo) == 2 and not halo.by_id
    assert [set(halo.link_handles(lv)) for lv in range(2)] == want_links
    assert all(len(halo.links[lv]) == len(want_links[lv]) for lv in range(2))
    assert halo.universe_size == want_universe and want_universe > 0
    # atoms[level]: the targets of the level's links that were in no frontier before
    expanded = set(seeds)
    for lv in range(2):
        reached = {t for link in want_links[lv] for t in das.get_link_targets(link)} - expanded
        assert set(halo.atom_handles(lv)) == reached
        assert list(halo.atoms[lv]) == sorted(reached)
        expanded |= reached
    assert [len(x) for x in miner.halo_host(das, seeds, 0).links] == []
    one = miner.halo_host(das, seeds, 1)
    assert [set(one.link_handles(0))] == want_links[:1]
    assert miner.halo_host(das, [], 2).universe_size == 0


def test_pattern_counts_host_is_build_patterns(case):
    das, seeds, want_links, _ = case
    links = sorted(want_links[0]) + sorted(want_links[1])[::7]
    want = notebook_build_patterns(das, links)
    pc = miner.pattern_counts_host(das, links + links[:3])                  # repeated links change nothing
    assert pc.as_dict() == want and len(pc) == len(want) > 0
    for i in range(len(pc)):
        t = pc.template(i)
        assert len(t) == int(pc.arity[i]) + 1 and W in t[1:] and t[0] != W
        assert pc.handle(i) == ExpressionHasher.composite_hash(t)
        assert int(pc.count[i]) == want[pc.handle(i)] == len(das.get_links(t[0], None, t[1:]))
        p = pc.pattern(i)
        assert p.atom_type == t[0] and p.ordered == (t[0] not in ("Similarity", "Set"))
        names = [f"V{t[1:k + 1].count(W)}" if h == W else das.get_node_name(h) for k, h in enumerate(t[1:], 1)]
        got = [getattr(x, "name", None) for x in p.targets]
        # (an unordered Link keeps its variables last, pattern_matcher.py:457)
        assert got == names if p.ordered else sorted(got) == sorted(names)
    assert len(miner.pattern_counts_host(das, [])) == 0


def test_unordered_templates_count_under_the_sorted_key():
    """[Similarity, *, b] and [Similarity, a, *] stay two templates; each is
    counted under the reference's key (grounded targets sorted, '*' first)."""
    kb, _ = _similarity()
    das = bench.OracleFacade(O.RedisMongoSemantics(kb))
    sim = [h for h, (t, tg, _) in sorted(kb.links.items()) if t == "Similarity"][:20]
    st = [h for h, (t, tg, _) in sorted(kb.links.items()) if t == "Set"][:20]
    pc = miner.pattern_counts_host(das, sim + st)
    d = pc.as_dict()
    for h in sim:
        a, b = kb.links[h][1]
        assert d[ExpressionHasher.composite_hash(["Similarity", W, b])] == \
            len(das.db.patterns.get((O.named_type_hash("Similarity"), W, b), ()))
        assert d[ExpressionHasher.composite_hash(["Similarity", a, W])] == \
            len(das.db.patterns.get((O.named_type_hash("Similarity"), W, a), ()))
    for h in st:
        a, b, c = kb.links[h][1]
        assert d[ExpressionHasher.composite_hash(["Set", a, W, c])] == \
            len(das.db.patterns.get((O.named_type_hash("Set"), W, *sorted([a, c])), ()))


def test_black_listed_type_is_never_found_and_counts_zero():
    kb, seeds = _animals()
    das = bench.OracleFacade(O.RedisMongoSemantics(kb, pattern_black_list=["Similarity"]))
    halo = miner.halo_host(das, seeds, 2)
    found = [h for lv in range(2) for h in halo.link_handles(lv)]
    assert found and all(kb.links[h][0] != "Similarity" for h in found)
    sim = [h for h, (t, _, _) in kb.links.items() if t == "Similarity"]
    pc = miner.pattern_counts_host(das, sim)
    assert len(pc) > 0 and not pc.count.any()
