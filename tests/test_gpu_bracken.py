"""Bracken weights on the device (slk_bracken_*, bracken.hip) against the model of BrackenWeights.scala (tests/bracken_model.py):
the reference's read totals for its tiny dataset, triples against literal() and fast() over random taxonomies, splitters and
read lengths, invariance under how the records are split into calls, and the refusals."""
import numpy as np
import pytest

import bracken_model as bm
from bracken_cases import Case

pytestmark = pytest.mark.gpu

slacken_amd = pytest.importorskip("slacken_amd")


def device_index(p, keys, taxa, parents, spaces, canonical, xor_mask=None):
    mask = {} if xor_mask is None else dict(xor_mask=xor_mask)
    ix = slacken_amd.Index(k=p.k, m=p.m, spaces=spaces, canonical=canonical, expected_records=len(keys) + 1000,
                           max_taxon=len(parents) - 1, **mask)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    return ix


def weights(ix, read_len, calls, max_fragment=0):
    bw = slacken_amd.BrackenWeights(ix, read_len, max_fragment)
    for bases, off, src in calls:
        bw.add(bases, off, src)
    out = bw.result()
    bw.close()
    return out


def as_dict(triples):
    d, s, c = triples
    return {(int(a), int(b)): int(n) for a, b, n in zip(d, s, c)}


# testData/slacken/slacken_tinydata.fna.fai of the reference (its .fna is not available): the 17 record lengths, labelled as in
# testData/slacken/seqid2taxid.map; the three-taxon taxonomy of T/slacken/Testing.scala:147-156 (all children of ROOT)
TINY = {455631: [4094363, 517, 568, 811, 860, 869, 873, 1057, 1230, 1234, 1277, 1575, 3015, 5351, 14150],
        526997: [3070512], 9606: [799920]}
TINY_TOTALS = {455631: 4126265, 526997: 3070413, 9606: 799821}   # Testing.scala:167-169 (BrackenWeightsTest.scala:30-46)


def test_reference_read_totals(orc):
    rng = np.random.default_rng(2048)
    parents = np.zeros(526998, np.int32)
    for t in TINY:
        parents[t] = 1
    recs, src = [], []
    for t, lens in TINY.items():
        for n in lens:
            g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
            for a in rng.integers(0, n - 50, max(1, n // 200_000)):   # scattered N runs
                g[a:a + int(rng.integers(1, 40))] = ord("N")
            recs.append(g)
            src.append(t)
    bases = np.concatenate(recs)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    ix = slacken_amd.Index(k=35, m=31, spaces=7, expected_records=int(off[-1]) // 2, max_taxon=len(parents) - 1)
    ix.set_taxonomy(parents)
    ix.add_sequences(bases, off, np.array(src, np.int32))
    ix.finalize()
    d, s, c = weights(ix, 100, [(bases, off, np.array(src, np.int32))])
    totals = {int(t): int(c[s == t].sum()) for t in np.unique(s)}
    assert totals == TINY_TOTALS
    # against the model, on the records other than the 4 Mbp ones (the model is Python)
    p = orc.params(k=35, m=31, spaces=7)
    keys, taxa = ix.export()
    small = [i for i, r in enumerate(recs) if len(r) < 1_000_000]
    model = bm.fast(orc, p, orc.Index(1, keys, taxa), parents, [recs[i].tobytes() for i in small], [src[i] for i in small], 100)
    sb = np.concatenate([recs[i] for i in small])
    so = np.concatenate([[0], np.cumsum([len(recs[i]) for i in small])]).astype(np.uint64)
    got = as_dict(weights(ix, 100, [(sb, so, np.array([src[i] for i in small], np.int32))]))
    assert got == model


SPLITS = [dict(k=35, m=31, spaces=7, canonical=True), dict(k=21, m=11, spaces=0, canonical=False),
          dict(k=31, m=15, spaces=3, canonical=True)]


@pytest.mark.parametrize("read_len", [35, 100, 150])
@pytest.mark.parametrize("split", range(len(SPLITS)))
def test_against_literal(orc, split, read_len):
    sp = SPLITS[split]
    p = orc.params(**sp)
    case = Case(orc, p, seed=7 + split * 11 + read_len, n_genomes=6, genome_len=4000, read_len=read_len)
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    for max_fragment in (0, 900):
        want = bm.literal(orc, p, case.index, case.parents, case.records, case.sources, read_len,
                          max_fragment or 1024 * 1024)
        got = as_dict(weights(ix, read_len, [case.packed()], max_fragment))
        assert got == want, (max_fragment, sorted(set(got.items()) ^ set(want.items()))[:10])


def test_against_fast_megabases(orc):
    sp = SPLITS[0]
    p = orc.params(**sp)
    case = Case(orc, p, seed=99, n_genomes=8, genome_len=250_000, read_len=100)
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    for max_fragment in (0, 60_000):
        want = bm.fast(orc, p, case.index, case.parents, case.records, case.sources, 100, max_fragment or 1024 * 1024)
        got = as_dict(weights(ix, 100, [case.packed()], max_fragment))
        assert got == want
        assert len({d for d, _ in got} - {0} - set(case.sources)) > 0   # ancestor destinations occur


def test_invariance(orc):
    sp = SPLITS[1]
    p = orc.params(**sp)
    case = Case(orc, p, seed=3, n_genomes=6, genome_len=20_000, read_len=100)
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    one = weights(ix, 100, [case.packed()], 5000)
    per_record = weights(ix, 100, [case.packed([i]) for i in range(len(case.records))], 5000)
    order = np.random.default_rng(1).permutation(len(case.records))
    shuffled = weights(ix, 100, [case.packed(order)], 5000)
    for other in (per_record, shuffled):
        for a, b in zip(one, other):
            assert np.array_equal(a, b)


def test_refusals(orc):
    p = orc.params()
    case = Case(orc, p, seed=4, n_genomes=2, genome_len=2000, read_len=100, extra_short=False)
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, 7, True)
    with pytest.raises(slacken_amd.SlackenError) as e:
        slacken_amd.BrackenWeights(ix, p.k - 1)
    assert e.value.code == slacken_amd.E_INVALID
    wide = slacken_amd.Index(k=45, m=40, spaces=0, expected_records=1000, max_taxon=len(case.parents) - 1)
    wide.set_taxonomy(case.parents)
    wide.finalize()
    with pytest.raises(slacken_amd.SlackenError) as e:
        slacken_amd.BrackenWeights(wide, 100)
    assert e.value.code == slacken_amd.E_UNSUPPORTED
