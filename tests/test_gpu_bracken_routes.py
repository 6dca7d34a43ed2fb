"""Bracken weights on the device along the kernel's rare routes, against literal() (tests/bracken_model.py):
  - the reference's trailing-hit ordinal quirk (BrackenWeights.scala:230) -- quirk detection in the expand kernel,
    the clamped deficit, its seeding at a later chunk start, stolen k-mers entering as NONE;
  - windows of more than 16 taxa -- the window lane's hand-over to the launch with its map in HBM, while the first window is
    built and in mid-slide, and with the deficit still open at the hand-over.
Each case first asserts, on the model, that it really takes its route."""
import numpy as np
import pytest

import bracken_hard as bh
import bracken_model as bm
from bracken_cases import Case
from test_gpu_bracken import SPLITS, as_dict, device_index, weights

pytestmark = pytest.mark.gpu

# (splitter, read length) pairs where the search of quirk_record finds a quirk (with read_len == k no segment after the first can
# have its last super-mer start before k-mer W = 1)
QUIRKS = [(0, 100), (1, 35), (1, 100), (1, 150), (2, 100), (2, 150)]


@pytest.mark.parametrize("split,read_len", QUIRKS)
def test_quirk_against_literal(orc, split, read_len):
    sp = SPLITS[split]
    p = orc.params(**sp)
    case = Case(orc, p, seed=40 + split, n_genomes=3, genome_len=3000, read_len=read_len, extra_short=False)
    found = bh.quirk_record(orc, p, case.index, np.frombuffer(case.records[0], np.uint8), read_len, 1400)
    assert found is not None
    rec, qt, d = found
    _, _, _, _, qt2, _ = bm.piece_arrays(orc, p, case.index, rec, read_len)
    assert qt2 == qt != 0 and d.max() > 0          # the literal counts differ from the true ones
    if split == 2:
        assert d[bh.CHUNK] > 0                     # ... still at the second chunk's first read: a seeded deficit
    records = [rec] + case.records[1:]
    sources = case.sources
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    packed = (np.frombuffer(b"".join(records), np.uint8),
              np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64), np.array(sources, np.int32))
    want = bm.literal(orc, p, case.index, case.parents, records, sources, read_len)
    got = as_dict(weights(ix, read_len, [packed]))
    assert got == want, sorted(set(got.items()) ^ set(want.items()))[:10]


def _check_many(orc, mt, records, max_fragments):
    p, L = mt.p, mt.read_len
    ix = device_index(p, mt.keys, mt.rec_taxa, mt.parents, 7, True)
    src = [mt.tb] * len(records)
    packed = (np.frombuffer(b"".join(records), np.uint8),
              np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64), np.array(src, np.int32))
    for mf in max_fragments:
        want = bm.literal(orc, p, mt.index, mt.parents, records, src, L, mf or 1024 * 1024)
        got = as_dict(weights(ix, L, [packed], mf))
        assert got == want, (mf, sorted(set(got.items()) ^ set(want.items()))[:10])


@pytest.mark.parametrize("read_len", [100, 150])
def test_many_taxa_against_literal(orc, read_len):
    mt = bh.ManyTaxa(orc, orc.params(), 3, read_len)
    records = mt.records(orc, quirk=True)
    initial = mid = False
    for rec in records[:3]:
        n = [len(c) for c in bm.window_counts_pure(orc, mt.p, mt.index, rec, read_len)]
        for c0 in range(0, len(n), bh.CHUNK):
            chunk = n[c0:c0 + bh.CHUNK]
            initial |= chunk[0] > bh.MAPCAP
            mid |= chunk[0] <= bh.MAPCAP and max(chunk) > bh.MAPCAP
    assert initial and mid          # both hand-over points of the window lane are taken
    _check_many(orc, mt, records, (0, 1000))


def test_many_taxa_with_open_deficit(orc):
    mt = bh.ManyTaxa(orc, orc.params(), 3, 150, b_every=2)
    rec = mt.records(orc, quirk=True)[-1]
    _, _, _, _, qt, _ = bm.piece_arrays(orc, mt.p, mt.index, rec, 150)
    assert qt != 0
    d = bh.deficits(orc, mt.p, mt.index, rec, 150, qt)
    n = [len(c) for c in bm.window_counts_pure(orc, mt.p, mt.index, rec, 150)]
    assert any(n[q] > bh.MAPCAP and d[q] > 0 for q in range(len(n)))   # a hand-over while the quirk's deficit is open
    _check_many(orc, mt, [rec], (0,))
