"""The Bracken weights model (tests/bracken_model.py): the vectorised form against the line-by-line restatement of
BrackenWeights.scala, on adversarial pieces; and a case where the reference's trailing-hit ordinal (:230) makes a read's
counts differ from its window's true counts, so that the reproduced quirk is exercised."""
import numpy as np
import pytest

import bracken_model as bm
from bracken_cases import Case

SPLITTERS = [dict(k=35, m=31, spaces=7, canonical=True), dict(k=21, m=11, spaces=0, canonical=False),
             dict(k=31, m=15, spaces=3, canonical=True)]


@pytest.mark.parametrize("read_len_kind", ["k", "k+1", "100", "150"])
@pytest.mark.parametrize("split", range(len(SPLITTERS)))
def test_fast_equals_literal(orc, split, read_len_kind):
    sp = SPLITTERS[split]
    p = orc.params(**sp)
    k = p.k
    read_len = {"k": k, "k+1": k + 1, "100": 100, "150": 150}[read_len_kind]
    case = Case(orc, p, seed=100 + split, n_genomes=4, genome_len=1500, read_len=read_len)
    for max_fragment in (1024 * 1024, 700):   # 700: records cross pieces
        if max_fragment < read_len:
            continue
        args = (orc, p, case.index, case.parents, case.records, case.sources, read_len, max_fragment)
        want = bm.literal(*args)
        assert bm.fast(*args) == want
        total = sum(want.values())
        assert total == sum(max(0, len(x) - read_len + 1) for r in case.records
                            for x in bm.split_to_max_length(r, max_fragment, read_len))


def test_split_to_max_length():
    # every read window belongs to exactly one piece (:152-164)
    seq = bytes(range(256)) * 10
    L = 100
    pieces = bm.split_to_max_length(seq, 700, L)
    starts = list(range(0, len(seq) - L + 1, 700 - (L - 1)))
    assert [len(x) for x in pieces][:-1] == [700] * (len(pieces) - 1)
    assert sum(len(x) - L + 1 for x in pieces) == len(seq) - L + 1
    assert all(seq[s:s + len(x)] == x for s, x in zip(starts, pieces))
    assert bm.split_to_max_length(seq[:700], 700, L) == [seq[:700]]


def test_quirk_is_exercised(orc):
    """A piece that starts with a short SEQUENCE segment, an N run, then a segment whose last super-mer covers k-mer W of the
    first window: the literal window credits the k-mers [W, t0) of that super-mer to NONE as they enter."""
    p = orc.params(k=21, m=11, spaces=0, canonical=False)
    case = Case(orc, p, seed=5, n_genomes=2, genome_len=2000, read_len=100, extra_short=False)
    k, L = p.k, 100
    W = L - k + 1
    g = np.frombuffer(case.records[0], np.uint8).copy()
    found = False
    for a in range(25, 60):   # an N at a; a SEQUENCE segment [a + 1, ...) ending soon after k-mer W
        for end in range(W + k, W + k + 30):
            h = g.copy()
            h[a] = ord("N")
            h[end] = ord("N")
            piece = h[:600].tobytes()
            tax, _, _, _, qt, qe = bm.piece_arrays(orc, p, case.index, piece, L)
            if qt == 0 or qe <= W + 1:
                continue
            lit = bm.literal_window_counts(orc, p, case.index, piece, L)
            pure = bm.window_counts_pure(orc, p, case.index, piece, L)
            if lit != pure:
                found = True
                # the only difference: taxon qt, short in the reads right after the first
                diff = [q for q in range(len(lit)) if lit[q] != pure[q]]
                assert diff[0] >= 1
                for q in diff:
                    assert set(lit[q]) <= set(pure[q]) | {qt}
                    assert all(lit[q].get(t) == pure[q].get(t) for t in pure[q] if t != qt)
                    assert lit[q].get(qt, 0) < pure[q][qt]
                args = (orc, p, case.index, case.parents, [piece], [case.sources[0]], L)
                assert bm.fast(*args) == bm.literal(*args)
                break
        if found:
            break
    assert found, "no piece of this form showed the quirk"
