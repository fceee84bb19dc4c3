"""The host side of the mining loop's bulk call (das_amd/miner.py): which
sub-combinations compute_isurprisingness needs and how a batch merges them,
the formula itself against the notebook's written out on literal counts, and
the input checks.  No GPU."""
import itertools
import math

import numpy as np
import pytest

from das_amd import miner


class _PC:
    """A PatternCounts as far as the input checks read it."""

    def __init__(self, count):
        self.count = np.asarray(count, dtype=np.uint64)

    def __len__(self):
        return len(self.count)


def _rows(distinct, where, c):
    return [tuple(int(v) for v in distinct[w]) for w in where[c]]


def test_sub_combinations_k2_has_none():
    assert miner.sub_combinations(np.array([[0, 1], [4, 2]], dtype=np.uint32)) == {}


def test_sub_combinations_k3_pairs_merged_over_the_batch():
    combos = np.array([[5, 1, 3], [3, 1, 9], [7, 7, 2]], dtype=np.uint32)
    sub = miner.sub_combinations(combos)
    assert sorted(sub) == [2]
    distinct, where = sub[2]
    assert distinct.dtype == np.uint32 and where.shape == (3, 3)
    # pairs of positions (0,1) (0,2) (1,2), each sorted: a sub-combination is a set
    assert _rows(distinct, where, 0) == [(1, 5), (3, 5), (1, 3)]
    assert _rows(distinct, where, 1) == [(1, 3), (3, 9), (1, 9)]
    # an index twice in a combination stays twice
    assert _rows(distinct, where, 2) == [(7, 7), (2, 7), (2, 7)]
    # (1, 3) of rows 0 and 1 and (2, 7) twice in row 2 are counted once each
    assert sorted(map(tuple, distinct.tolist())) == [(1, 3), (1, 5), (1, 9), (2, 7), (3, 5), (3, 9), (7, 7)]
    assert where[0, 2] == where[1, 0] and where[2, 1] == where[2, 2]


def test_sub_combinations_k4_pairs_and_triples():
    combos = np.array([[8, 2, 6, 4], [2, 4, 6, 0]], dtype=np.uint32)
    sub = miner.sub_combinations(combos)
    assert sorted(sub) == [2, 3]
    d2, w2 = sub[2]
    d3, w3 = sub[3]
    assert w2.shape == (2, 6) and w3.shape == (2, 4)
    assert _rows(d2, w2, 0) == [(2, 8), (6, 8), (4, 8), (2, 6), (2, 4), (4, 6)]
    assert _rows(d3, w3, 0) == [(2, 6, 8), (2, 4, 8), (4, 6, 8), (2, 4, 6)]
    assert _rows(d3, w3, 1) == [(2, 4, 6), (0, 2, 4), (0, 2, 6), (0, 4, 6)]
    assert len(d2) == 6 + 6 - 3 and len(d3) == 4 + 4 - 1          # {2,4,6} is shared
    assert w3[0, 3] == w3[1, 0]


def test_sub_combinations_of_an_empty_batch():
    sub = miner.sub_combinations(np.zeros((0, 3), dtype=np.uint32))
    assert sub[2][0].shape == (0, 2) and sub[2][1].shape == (0, 3)


# compute_isurprisingness of the notebook (cell 3fa7b2ec), the counts of the
# sub-combinations looked up in a table instead of queried
def _notebook(count, counts, pair, triple, universe_size, normalized):
    def prob(c):
        return c / universe_size
    n = len(counts)
    if n == 2:
        subset_probs = [prob(counts[0]) * prob(counts[1])]
    elif n == 3:
        subset_probs = [
            prob(counts[0]) * prob(counts[1]) * prob(counts[2]),
            prob(pair[0, 1]) * prob(counts[2]),
            prob(pair[0, 2]) * prob(counts[1]),
            prob(pair[1, 2]) * prob(counts[0]),
        ]
    else:
        subset_probs = [
            prob(counts[0]) * prob(counts[1]) * prob(counts[2]) * prob(counts[3]),
            prob(pair[0, 1]) * prob(pair[2, 3]),
            prob(pair[0, 2]) * prob(pair[1, 3]),
            prob(pair[0, 3]) * prob(pair[1, 2]),
            prob(triple[0, 1, 2]) * prob(counts[3]),
            prob(triple[0, 1, 3]) * prob(counts[2]),
            prob(triple[0, 2, 3]) * prob(counts[1]),
            prob(triple[1, 2, 3]) * prob(counts[0]),
        ]
    p = prob(count)
    isurprisingness = max([p - max(subset_probs), min(subset_probs) - p])
    return isurprisingness / p if normalized else isurprisingness


UNIVERSE = 7919
PAIR = {(0, 1): 211, (0, 2): 17, (0, 3): 1, (1, 2): 389, (1, 3): 0, (2, 3): 97}
TRIPLE = {(0, 1, 2): 13, (0, 1, 3): 0, (0, 2, 3): 1, (1, 2, 3): 5}
TERMS = [1031, 4099, 523, 97]
PAIR_ORDER = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
TRIPLE_ORDER = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_formula_matches_the_notebook(k, normalized):
    counts = [3, 211, 1] if k == 2 else [3, 13, 40] if k == 3 else [1, 5, 2]
    terms = np.array([TERMS[:k]] * len(counts), dtype=np.uint64)
    pairs = [p for p in PAIR_ORDER if max(p) < k]
    pair_counts = np.array([[PAIR[p] for p in pairs]] * len(counts), dtype=np.uint64) if k > 2 else None
    triple_counts = np.array([[TRIPLE[t] for t in TRIPLE_ORDER]] * len(counts), dtype=np.uint64) if k > 3 else None
    got = miner.isurprisingness_from_counts(np.array(counts, dtype=np.uint64), terms, UNIVERSE, pair_counts,
                                            triple_counts, normalized=normalized)
    assert got.dtype == np.float64 and got.shape == (len(counts),)
    want = [_notebook(c, TERMS[:k], PAIR, TRIPLE, UNIVERSE, normalized) for c in counts]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert (got != 0).all()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_count_zero(k):
    terms = np.array([TERMS[:k]], dtype=np.uint64)
    pairs = [p for p in PAIR_ORDER if max(p) < k]
    pair_counts = np.array([[PAIR[p] for p in pairs]], dtype=np.uint64) if k > 2 else None
    triple_counts = np.array([[TRIPLE[t] for t in TRIPLE_ORDER]], dtype=np.uint64) if k > 3 else None
    zero = np.zeros(1, dtype=np.uint64)
    plain = miner.isurprisingness_from_counts(zero, terms, UNIVERSE, pair_counts, triple_counts)
    np.testing.assert_allclose(plain, [_notebook(0, TERMS[:k], PAIR, TRIPLE, UNIVERSE, False)], rtol=1e-12, atol=0)
    with pytest.raises(ZeroDivisionError):
        _notebook(0, TERMS[:k], PAIR, TRIPLE, UNIVERSE, True)
    norm = miner.isurprisingness_from_counts(zero, terms, UNIVERSE, pair_counts, triple_counts, normalized=True)
    assert math.isnan(norm[0])


def test_formula_over_a_mixed_batch():
    """Different rows, different counts: nothing is shared between rows."""
    count = np.array([0, 7, 7919], dtype=np.uint64)
    terms = np.array([[10, 20, 30], [7919, 7919, 7], [7919, 7919, 7919]], dtype=np.uint64)
    pair_counts = np.array([[0, 1, 2], [7919, 7, 7], [7919, 7919, 7919]], dtype=np.uint64)
    got = miner.isurprisingness_from_counts(count, terms, UNIVERSE, pair_counts)
    want = [_notebook(int(count[i]), terms[i].tolist(), {(0, 1): int(pair_counts[i, 0]), (0, 2): int(pair_counts[i, 1]),
                                                         (1, 2): int(pair_counts[i, 2])}, None, UNIVERSE, False)
            for i in range(3)]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("combos", [
    [(0,)],                              # k = 1
    [(0, 1, 2, 3, 4)],                   # k = 5
    [(0, 1), (0, 1, 2)],                 # ragged
    [(0, -1)],                           # negative
    [(0, 5)],                            # too large
    np.array([[0, 1], [2, 5]]),
    np.array([[0.5, 1.0]]),
])
def test_bad_combinations_raise(combos):
    pc = _PC([1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        miner.check_combos(combos, len(pc))
    with pytest.raises(ValueError):
        miner.conjunction_counts_host(None, pc, combos)
    with pytest.raises(ValueError):
        miner.isurprisingness(None, pc, combos, 10)


def test_good_combinations_pass():
    got = miner.check_combos([(0, 4), (4, 4)], 5)
    assert got.dtype == np.uint32 and got.tolist() == [[0, 4], [4, 4]]
    assert miner.check_combos(np.array([[1, 2, 3, 0]], dtype=np.int8), 4).shape == (1, 4)
    assert miner.check_combos([], 5).shape[0] == 0
    assert miner.check_combos(np.zeros((0, 3), dtype=np.int64), 0).shape == (0, 3)


def _reference_flat_and(terms):
    """And.matched of the reference (pattern_matcher.py:705-748) over terms
    that each bind V1 only, as sets of values: the size of the answer."""
    running = set()
    for values in terms:
        if not values:                     # an empty Link answers False
            return 0
        if not running:                    # :725-729, also after an empty join
            running = set(values)
            continue
        running = running & values
    return len(running)


def test_flat_triples_of_a_4_combination():
    """The notebook counts the triples of n == 4 with a flat And: where the
    first two terms join to nothing it gets the third term's own count."""
    rng = np.random.default_rng(5)
    pairs, triples = list(itertools.combinations(range(4), 2)), list(itertools.combinations(range(4), 3))
    cases = [[set(np.flatnonzero(rng.random(6) < p).tolist()) for p in rng.choice([0.0, 0.3, 0.7], size=4)]
             for _ in range(300)]
    cases += [[{1}, {2}, {3, 4}, {1, 5}], [{1}, {1, 2}, set(), {1}], [{1, 2}, {2, 3}, {3}, {2}]]
    join = lambda sets, idx: len(set.intersection(*(sets[i] for i in idx)))        # noqa: E731
    terms = [[len(s) for s in sets] for sets in cases]
    pair_counts = [[join(sets, p) for p in pairs] for sets in cases]
    triple_counts = [[join(sets, t) for t in triples] for sets in cases]
    got = miner.flat_triple_counts(terms, pair_counts, triple_counts)
    want = [[_reference_flat_and([sets[i] for i in t]) for t in triples] for sets in cases]
    assert got.dtype == np.uint64 and got.tolist() == want
    assert got.tolist() != triple_counts                                  # the two queries do differ
    assert got[-3].tolist() == [2, 2, 2, 2] and got[-2].tolist() == [0, 1, 0, 0] and got[-1].tolist() == [0, 1, 1, 0]
