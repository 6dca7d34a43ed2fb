"""Randomised differential test of the Bracken weights pipeline (slk_bracken_*, bracken.hip) against literal()
(tests/bracken_model.py) over the parameter space of tests/bracken_fuzz_cases.py: splitters with k == m up to windows of 48 m-mers
(fused and staged scanner), spaced and unspaced, canonical or not, XOR masks, read lengths k .. 1000, max_fragment from read_len
(one read per piece) to the default, dense and sparse taxon ids.  Odd seeds also run with 1 MiB batches and two add calls.  Every
comparison is exact equality of the (dest, source, count) triples.  tests/test_bracken_fuzz_model.py asserts, on the model, what
the default seed set covers."""
import numpy as np
import pytest

import bracken_fuzz_cases as fz
import bracken_model as bm
from test_gpu_bracken import as_dict, device_index

pytestmark = pytest.mark.gpu

slacken_amd = pytest.importorskip("slacken_amd")


def run(ix, cfg, calls):
    bw = slacken_amd.BrackenWeights(ix, cfg.read_len, cfg.max_fragment)
    try:
        for bases, off, src in calls:
            bw.add(bases, off, src)
        return bw.result()
    finally:
        bw.close()


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_differential(orc, seed, monkeypatch):
    cfg = fz.config(seed)
    p, case = cfg.case(orc)
    want = bm.literal(orc, p, case.index, case.parents, case.records, case.sources, cfg.read_len, cfg.fragment)
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, cfg.spaces, cfg.canonical, cfg.xor_mask)
    triples = run(ix, cfg, [case.packed()])
    got = as_dict(triples)
    assert got == want, (cfg, sorted(set(got.items()) ^ set(want.items()))[:10])
    assert len(got) == len(triples[0])                                    # no pair twice
    order = list(zip(triples[0].tolist(), triples[1].tolist()))
    assert order == sorted(order)                                         # dest ascending, then source
    if seed % 2:   # small batches and two calls: the same arrays
        monkeypatch.setenv("SLK_BRACKEN_BATCH_MB", "1")
        half = len(case.records) // 2
        split = run(ix, cfg, [case.packed(range(half)), case.packed(range(half, len(case.records)))])
        for a, b in zip(triples, split):
            assert np.array_equal(a, b), (cfg, sorted(set(as_dict(split).items()) ^ set(want.items()))[:10])
