"""The respace model (respace_model.py) and its generator on the CPU: the generator makes what the GPU tests need -- classes whose
LCA is ROOT, an interior node nobody held, a member's own taxon, and one class with every fill -- and the model has the properties
KeyValueIndex.respace has by construction (a projection, independent of the order of the records)."""
import numpy as np
import pytest

import respace_model as rm


@pytest.fixture(scope="module")
def gen(orc):
    return rm.generate(3000, np.random.default_rng(712))


def test_generator_preconditions(gen):
    m, a, b = gen["m"], gen["s_old"], gen["s_new"]
    keys = gen["keys"].view(np.uint64)
    assert len(np.unique(keys)) == len(keys)                                    # a library: unique keys
    assert np.all(keys & ~np.uint64(rm.mask(m, a)) == 0)                        # ... at s_old spaces
    assert gen["taxa"].min() >= 1
    mk, _ = rm.respace(gen["keys"], gen["taxa"], gen["parents"], m, b)
    assert len(mk) == 3000 and len(keys) > 3 * len(mk)
    out = rm.outcomes(gen)
    print(len(keys), "records ->", len(mk), out)
    assert min(out["root"], out["interior"], out["member"]) >= 50 and out["single"] >= 50
    full = gen["full_class"].view(np.uint64)
    assert len(full) == 4 ** (b - a) == len(np.unique(full))
    assert len(np.unique(full & np.uint64(rm.mask(m, b)))) == 1
    sizes = np.bincount(gen["class_of"])
    assert sizes[1:].max() <= 64 and sizes[1:].min() == 1


def test_masks_nest():
    for m in (31, 24, 16):
        for s in range(0, m // 2):
            lo, hi = rm.mask(m, s), rm.mask(m, s + 1)
            assert hi & lo == hi and hi != lo and bin(lo ^ hi).count("1") == 2
    assert len(rm.free_bits(31, 7, 12)) == 10


def test_respace_is_a_projection(gen):
    m, parents = gen["m"], gen["parents"]
    for a, b in ((8, 12), (10, 12), (11, 12), (10, 15)):
        direct = rm.respace(gen["keys"], gen["taxa"], parents, m, b)
        step = rm.respace(*rm.respace(gen["keys"], gen["taxa"], parents, m, a), parents, m, b)
        assert np.array_equal(direct[0], step[0]) and np.array_equal(direct[1], step[1])


def test_respace_ignores_record_order(gen):
    want = rm.respace(gen["keys"], gen["taxa"], gen["parents"], gen["m"], 12)
    rng = np.random.default_rng(3)
    for _ in range(3):
        o = rng.permutation(len(gen["keys"]))
        got = rm.respace(gen["keys"][o], gen["taxa"][o], gen["parents"], gen["m"], 12)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(rm.respace([], [], gen["parents"], gen["m"], 12)[0]) == 0
