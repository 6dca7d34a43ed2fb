"""The premise of library merging on the oracle alone: a record's taxon is the LCA of the taxa of all sequences that hold
the minimizer, LCA is associative, commutative and idempotent, so the records of the parts, folded per key by LCA, are the records of
the whole -- however the sequences are split.  And the taxon translation of merge.hpp, restated in merge_model.py, on a hand-written
table."""
import numpy as np
import pytest

import merge_model as mm
import taxgen


@pytest.fixture(scope="module")
def world(orc):
    rng = np.random.default_rng(2310)
    parents = taxgen.taxonomy(40, rng)
    seqs, taxa = mm.sequences(rng, 18, parents)
    p = orc.params()
    return dict(p=p, parents=parents, seqs=seqs, taxa=taxa, whole=mm.build_records(p, parents, seqs, taxa))


def part(w, idx):
    return mm.build_records(w["p"], w["parents"], [w["seqs"][i] for i in idx], [w["taxa"][i] for i in idx])


SPLITS = {
    "two": [range(0, 9), range(9, 18)],
    "three": [range(0, 5), range(5, 11), range(11, 18)],
    "interleaved": [range(0, 18, 3), range(1, 18, 3), range(2, 18, 3)],
    "overlapping": [range(0, 12), range(6, 18)],
}


@pytest.mark.parametrize("name", list(SPLITS))
def test_merge_of_the_parts_is_the_whole(world, name):
    parts = [part(world, idx) for idx in SPLITS[name]]
    shared = sum(len(p[0]) for p in parts) - len(np.unique(np.concatenate([p[0] for p in parts])))
    assert len(world["whole"][0]) > 3000
    assert shared >= 0.10 * len(world["whole"][0]), (shared, len(world["whole"][0]))      # (the case is not vacuous)
    for order in (parts, parts[::-1], parts[1:] + parts[:1]):
        assert mm.same(mm.merge(world["parents"], order), world["whole"])
    # some shared key ends above both parts' taxa: a merge that kept the first or the last taxon would fail here
    first = dict(zip(*[a.tolist() for a in parts[0]]))
    whole = dict(zip(*[a.tolist() for a in world["whole"]]))
    assert any(k in first and whole[k] not in (first[k], t) for k, t in zip(*[a.tolist() for a in parts[1]]))


def test_merge_is_idempotent_and_skips_none(world):
    parents, whole = world["parents"], world["whole"]
    assert mm.same(mm.merge(parents, [whole, whole]), whole)
    keys = np.array([5, 5, 6, 7], np.int64)
    taxa = np.array([0, 3, 0, 1], np.int32)
    assert mm.merge(parents, [(keys, taxa)]) == {5: 3, 7: 1}
    assert mm.merge(parents, []) == {}


def test_merge_drops_what_the_destination_does_not_define():
    parents = np.array([0, 0, 1, 1, 2, 0, 3], np.int32)        # 5 is undefined
    keys = np.arange(7, dtype=np.int64)
    taxa = np.array([4, 5, 6, 7, -3, 2, 0], np.int32)
    assert mm.merge(parents, [(keys, taxa)]) == {0: 4, 2: 6, 5: 2}
    assert mm.refused(parents, keys, taxa) == [5, 7, -3]
    remap = np.array([0, 1, 4, 4, 0], np.int32)                 # 2 and 3 to one node, 4 to nothing, 5.. beyond the table
    got = mm.merge(parents, [(keys, np.array([2, 3, 4, 1, 6, 2, 0], np.int32))], remaps=[remap])
    assert got == {0: 4, 1: 4, 3: 1, 5: 4}
    assert mm.refused(parents, keys, np.array([2, 3, 4, 1, 6, 2, 0], np.int32), remap) == [4, 6]


def test_taxon_remap_table():
    #            0  1  2  3  4  5  6  7
    src = mm.Tax([0, 0, 1, 1, 2, 2, 0, 3])                      # defines 1 2 3 4 5 7
    same_tree = mm.Tax([0, 0, 1, 1, 2, 2, 0, 3])
    m, identity = mm.taxon_remap(src, same_tree)
    assert identity and m.tolist() == [0, 1, 2, 3, 4, 5, 0, 7]
    larger = mm.Tax([0, 0, 1, 1, 2, 2, 3, 3, 1])                 # a superset of the nodes: still the identity on src's
    m, identity = mm.taxon_remap(src, larger)
    assert identity and m.tolist() == [0, 1, 2, 3, 4, 5, 0, 7]
    merged = mm.Tax([0, 0, 1, 1, 2, 0, 0, 3], merged=[(5, 4)])   # 5 went into 4 by merged.dmp
    m, identity = mm.taxon_remap(src, merged)
    assert not identity and m.tolist() == [0, 1, 2, 3, 4, 4, 0, 7]
    missing = mm.Tax([0, 0, 1, 1, 2, 0, 0, 3])                   # 5 is gone and nothing says where
    m, identity = mm.taxon_remap(src, missing)
    assert not identity and m.tolist() == [0, 1, 2, 3, 4, 0, 0, 7]
    short = mm.Tax([0, 0, 1, 1, 2, 2])                           # 7 lies beyond the destination's array
    m, identity = mm.taxon_remap(src, short)
    assert not identity and m.tolist() == [0, 1, 2, 3, 4, 5, 0, 0]
    onto_undefined = mm.Tax([0, 0, 1, 1, 2, 0, 0, 3], merged=[(5, 6)])   # merged into a node the destination does not define
    assert mm.taxon_remap(src, onto_undefined)[0].tolist() == [0, 1, 2, 3, 4, 0, 0, 7]
