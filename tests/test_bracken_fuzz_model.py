"""The Bracken fuzz space (tests/bracken_fuzz_cases.py) on the model alone: for every seed the vectorised fast() equals the line by
line literal() and every read position of every piece is counted once; and the default seed set covers the corners it is there
for, asserted, so that the device sweep (tests/test_gpu_bracken_fuzz.py) cannot quietly go soft."""
import pytest

import bracken_fuzz_cases as fz
import bracken_model as bm

_ancestors = {}   # seed -> whether literal() gave a destination that is neither NONE nor a source (for the coverage test)


def check(orc, seed):
    cfg = fz.config(seed)
    p, case = cfg.case(orc)
    args = (orc, p, case.index, case.parents, case.records, case.sources, cfg.read_len, cfg.fragment)
    want = bm.literal(*args)
    got = bm.fast(*args)
    assert got == want, (cfg, sorted(set(got.items()) ^ set(want.items()))[:10])
    positions = sum(max(0, len(x) - cfg.read_len + 1) for r in case.records
                    for x in bm.split_to_max_length(r, cfg.fragment, cfg.read_len))
    assert positions > 0 and sum(want.values()) == positions, cfg
    _ancestors[seed] = bool({d for d, _ in want} - {0} - set(case.sources))


@pytest.mark.parametrize("seed", fz.SEEDS)
def test_fast_equals_literal(orc, seed):
    check(orc, seed)


def test_config_is_a_function_of_the_seed():
    for seed in fz.DEFAULT_SEEDS:
        assert fz.config(seed) == fz.config(seed)
        c = fz.config(seed)
        assert 8 <= c.m <= 32 and c.m <= c.k and c.read_len >= c.k and c.fragment >= c.read_len and 0 <= c.spaces <= c.m // 2


def test_pinned_seeds_are_what_they_say():
    c = {s: fz.config(s) for s in fz.PINNED}
    assert sorted(x.read_len for x in c.values() if x.w == 1) == [50, 150]           # k == m at two read lengths
    assert {33, 48} <= {x.w for x in c.values() if x.m <= 32}
    assert any(x.read_len == x.k and x.max_fragment == x.read_len for x in c.values())
    assert set(fz.PINNED) <= set(fz.SEEDS)                                            # whatever SLK_BRACKEN_FUZZ_SEEDS says


def test_default_seeds_cover_the_space(orc):
    cfgs = [fz.config(s) for s in fz.DEFAULT_SEEDS]
    assert any(c.w == 1 for c in cfgs)
    assert any(c.w > 32 for c in cfgs)
    assert any(c.w > 32 for c in cfgs if c.seed not in fz.PINNED)        # the random part reaches the staged scanner too
    assert any(c.read_len >= 600 for c in cfgs)
    assert any(c.read_len == c.k + 1 for c in cfgs)
    assert any(c.max_fragment == c.read_len for c in cfgs)
    assert any(c.max_fragment == c.read_len + 1 for c in cfgs)
    assert any(not c.canonical for c in cfgs)
    assert any(c.spaces > 0 for c in cfgs)
    assert any(c.xor_mask != fz.DEFAULT_MASK for c in cfgs)
    assert any(c.sparse for c in cfgs) and any(not c.sparse for c in cfgs)
    for s in fz.DEFAULT_SEEDS:
        if s not in _ancestors:   # this test run on its own
            check(orc, s)
    ancestors = sum(_ancestors[s] for s in fz.DEFAULT_SEEDS)
    assert 2 * ancestors >= len(fz.DEFAULT_SEEDS), ancestors   # a destination that is neither NONE nor a source: LCAs resolved
