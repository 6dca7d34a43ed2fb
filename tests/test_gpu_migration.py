"""Minimizer migration on the GPU (slk_migration_*, slacken_amd/csrc/migration.hip) through capi.MinimizerMigration against the
plain-Python join of migration_model.py: every size at which the kernel's waves and blocks are partly filled, any chunking, the
three routes a record can take to the device-wide pair map (wave ballot, LDS map, direct), the map's growth and its capacity
failure, renumbered reference ids, refusals and lifetimes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import migration_model as mm
import synth
import taxgen
from test_host_classify2_gpu import write_ranked_taxonomy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unique_keys(n, rng, but=()):
    """n distinct left-aligned 31-mers (the low two bits clear), none of them 0 or in `but`"""
    out, seen = [], set(int(b) for b in but) | {0}
    while len(out) < n:
        for k in (rng.integers(-2**63, 2**63, size=n, dtype=np.int64) & ~np.int64(3)):
            if int(k) not in seen and len(out) < n:
                seen.add(int(k))
                out.append(int(k))
    return np.array(out, np.int64)


def check(mig, subject_keys, subject_taxa, ref, tax, with_depths=True):
    pairs, matched, unmatched = mm.join(zip(subject_keys.tolist(), subject_taxa.tolist()), ref)
    want = mm.triples(pairs, tax, with_depths)
    t1, t2, steps, count, got_matched, got_unmatched = mig.result()
    got = list(zip(t1.tolist(), t2.tolist(), steps.tolist(), count.tolist()))
    assert got == want
    assert (got_matched, got_unmatched) == (matched, unmatched)
    assert count.dtype == np.uint64 and t1.dtype == np.int32
    return want


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import slacken_amd
    rng = np.random.default_rng(41)
    parents = taxgen.taxonomy(96, rng)
    tax = write_ranked_taxonomy(str(tmp_path_factory.mktemp("mig") / "taxonomy"), parents)
    depths = np.array([mm.depth(tax, t) for t in range(len(tax.parents))], np.int32)
    defined = np.array(taxgen.defined_taxa(parents), np.int32)
    rk = np.concatenate([unique_keys(19999, rng), [0]]).astype(np.int64)   # key 0 is a record like any other
    rt = rng.choice(defined, size=len(rk)).astype(np.int32)
    ix = slacken_amd.Index(expected_records=len(rk), max_taxon=len(parents) - 1, device=0)
    ix.append(rk, rt)
    ix.finalize()
    ref = dict(zip(rk.tolist(), rt.tolist()))
    # subject: 70 % of the reference's keys (key 0 among them, once) and 2000 keys it lacks
    pick = np.concatenate([rng.choice(len(rk) - 1, size=13999, replace=False), [len(rk) - 1]])
    sk = np.concatenate([rk[pick], unique_keys(2000, rng, but=rk)])
    st1 = np.concatenate([rt[pick], rng.choice(defined, size=2000).astype(np.int32)])
    moved = rng.random(len(sk)) < 0.4                     # most records keep their taxon, the others get any
    st1[moved] = rng.choice(defined, size=int(moved.sum()))
    st1[rng.random(len(sk)) < 0.05] = 0                   # NONE: no record
    order = rng.permutation(len(sk))
    sk, st1 = sk[order], st1[order].astype(np.int32)
    st1[sk == 0] = defined[3]
    assert (sk == 0).sum() == 1
    return dict(ix=ix, st=ix.stream(), ref=ref, tax=tax, depths=depths, sk=sk, st1=st1, rng=rng, parents=parents, defined=defined)


@pytest.fixture(scope="module")
def big():
    """240 000 reference records: 200 000 for the skewed subject, 40 000 whose taxa are uniform over 300 ids"""
    import slacken_amd
    rng = np.random.default_rng(43)
    rk = unique_keys(240000, rng)
    rt = np.empty(len(rk), np.int32)
    n = 200000
    hot, warm = int(n * 0.95), int(n * 0.049)
    rt[:hot] = 77
    rt[hot:hot + warm] = 100 + rng.integers(0, 15, size=warm)
    rt[hot + warm:n] = rng.integers(1, 5000, size=n - hot - warm)
    rt[n:] = rng.integers(1, 301, size=len(rk) - n)
    ix = slacken_amd.Index(expected_records=len(rk), max_taxon=5000, device=0)
    ix.append(rk, rt)
    ix.finalize()
    return dict(ix=ix, st=ix.stream(), rk=rk, rt=rt, ref=dict(zip(rk.tolist(), rt.tolist())), rng=rng, n=n, hot=hot, warm=warm)


def test_sizes_in_one_add(world):
    import slacken_amd
    sk, st1 = world["sk"], world["st1"]
    seen = set()
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 5000, len(sk)):
        mig = slacken_amd.capi.MinimizerMigration(world["ix"], world["depths"], stream=world["st"])
        mig.add(sk[:n], st1[:n])
        want = check(mig, sk[:n], st1[:n], world["ref"], world["tax"])
        seen |= {s for _, _, s, _ in want}
        mig.close()
    assert len(seen) >= 4 and min(seen) < 0 < max(seen)     # taxa moved up and down in the full set


def test_chunking_order_and_device_entry(world):
    import slacken_amd
    import torch
    rng = np.random.default_rng(5)
    sk, st1 = world["sk"], world["st1"]
    order = rng.permutation(len(sk))
    sk, st1 = sk[order], st1[order]
    cuts = [0, 0, 1, 1, 64, 700, 701, 5000, 5000, 12345, len(sk), len(sk)]
    mig = slacken_amd.capi.MinimizerMigration(world["ix"], world["depths"], stream=world["st"])
    dev = slacken_amd.capi.MinimizerMigration(world["ix"], world["depths"], stream=world["st"])
    d_k, d_t = torch.from_numpy(sk).cuda(), torch.from_numpy(st1).cuda()
    for a, b in zip(cuts[:-1], cuts[1:]):
        mig.add(sk[a:b], st1[a:b])
        dev.add_device(d_k.data_ptr() + 8 * a, d_t.data_ptr() + 4 * a, b - a)
        if b in (1, 701, 12345, len(sk)):     # result between adds: the model of the prefix
            check(mig, sk[:b], st1[:b], world["ref"], world["tax"])
            check(dev, sk[:b], st1[:b], world["ref"], world["tax"])
    check(mig, world["sk"], world["st1"], world["ref"], world["tax"])   # the order of the records does not matter
    mig.close()
    dev.close()


def test_skewed_pairs(big):
    """95 % of 200 000 records on one pair, 4.9 % on 15 others, the rest on pairs of their own: the wave's ballot rounds take the
    hot pair, the LDS map the others; fed three times, every count is three-fold"""
    import slacken_amd
    n, hot, warm, rng = big["n"], big["hot"], big["warm"], big["rng"]
    sk = big["rk"][:n].copy()
    st1 = np.empty(n, np.int32)
    st1[:hot] = 76
    st1[hot:hot + warm] = big["rt"][hot:hot + warm] + 1000     # one t1 per t2: 15 pairs
    st1[hot + warm:] = 10000 + np.arange(n - hot - warm)      # pairs of their own
    order = rng.permutation(n)
    sk, st1 = sk[order], st1[order]
    mig = slacken_amd.capi.MinimizerMigration(big["ix"], None, stream=big["st"])
    mig.add(sk, st1)
    want = check(mig, sk, st1, big["ref"], None, with_depths=False)
    counts = sorted((c for _, _, _, c in want), reverse=True)
    assert counts[0] == hot and len(want) == 1 + 15 + (n - hot - warm)
    mig.add(sk[:70000], st1[:70000])
    mig.add(sk[70000:], st1[70000:])
    mig.add(sk, st1)
    t1, t2, steps, count, matched, unmatched = mig.result()
    assert list(zip(t1.tolist(), t2.tolist(), count.tolist())) == [(a, b, 3 * c) for a, b, _, c in want]
    assert (matched, unmatched) == (3 * n, 0) and not steps.any()
    mig.close()


def test_more_pairs_than_a_block_map_holds(big, monkeypatch):
    """40 000 records over 300 x 300 pairs: more distinct pairs than 160 KiB of LDS holds at 8 bytes a slot.  With the default grid
    every block sees a few hundred of them; with SLK_MIGRATION_BLOCKS=2 (read when the handle is created) each of two blocks sees
    far more pairs than its LDS map has slots, so records reach the device-wide map both directly and through the flush."""
    import slacken_amd
    n, rng = big["n"], big["rng"]
    sk = big["rk"][n:].copy()
    st1 = rng.integers(1, 301, size=len(sk)).astype(np.int32)
    pairs, _, _ = mm.join(zip(sk.tolist(), st1.tolist()), big["ref"])
    assert len(pairs) >= 30000 > 160 * 1024 // 8
    for blocks in (None, "2"):
        if blocks:
            monkeypatch.setenv("SLK_MIGRATION_BLOCKS", blocks)
        mig = slacken_amd.capi.MinimizerMigration(big["ix"], None, stream=big["st"])
        mig.add(sk, st1)
        check(mig, sk, st1, big["ref"], None, with_depths=False)
        mig.close()


CAPACITY_SCRIPT = """
import os, sys
os.environ["SLK_MIGRATION_MAP_LOG2"] = "10"
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import slacken_amd
from slacken_amd import capi
import migration_model as mm
rng = np.random.default_rng(3)
rk = np.unique(rng.integers(1, 2**62, size=6000, dtype=np.int64) & ~np.int64(3))[:5100]
assert len(rk) == 5100
rt = rng.integers(1, 50, size=len(rk)).astype(np.int32)
ix = slacken_amd.Index(expected_records=len(rk), max_taxon=64, device=0)
ix.append(rk, rt); ix.finalize()
st = ix.stream()
ref = dict(zip(rk.tolist(), rt.tolist()))
t1 = (1000 + np.arange(len(rk))).astype(np.int32)          # a pair of its own per key

def same(mig, keys, taxa):
    pairs, matched, unmatched = mm.join(zip(keys.tolist(), taxa.tolist()), ref)
    a, b, s, c, gm, gu = mig.result()
    assert list(zip(a.tolist(), b.tolist(), s.tolist(), c.tolist())) == mm.triples(pairs, None, False)
    assert (gm, gu) == (matched, unmatched)
    return len(pairs)

# exactly 1024 distinct pairs fill the 2^10 slots: once with one record each, once with 64 each
for reps in (1, 64):
    mig = capi.MinimizerMigration(ix, None, stream=st)
    k, t = np.tile(rk[:1024], reps), np.tile(t1[:1024], reps)
    mig.add(k, t)
    assert same(mig, k, t) == 1024
    # the policy: between calls a map more than half full doubles, so a 1025th pair in a LATER add finds room
    mig.add(rk[1024:1025], t1[1024:1025])
    assert same(mig, np.concatenate([k, rk[1024:1025]]), np.concatenate([t, t1[1024:1025]])) == 1025
    mig.close()
# ... while one add that brings 1025 new pairs by itself fills the map: SLK_E_CAPACITY, and the handle is spent
mig = capi.MinimizerMigration(ix, None, stream=st)
try:
    mig.add(rk[:1025], t1[:1025])
    raise SystemExit("1025 pairs in one add: no error")
except slacken_amd.SlackenError as e:
    assert e.code == capi.E_CAPACITY, e
for call in (lambda: mig.add(rk[:1], t1[:1]), lambda: mig.add(rk[:0], t1[:0]), mig.result,
             lambda: mig.add_device(0, 0, 0)):
    try:
        call()
        raise SystemExit("a spent handle took a call")
    except slacken_amd.SlackenError as e:
        assert e.code == capi.E_STATE, e
mig.close()
# growth: 5000 pairs from the initial 2^10, 500 new ones per add
mig = capi.MinimizerMigration(ix, None, stream=st)
for a in range(0, 5000, 500):
    mig.add(rk[a:a + 500], t1[a:a + 500])
assert same(mig, rk[:5000], t1[:5000]) == 5000
mig.close()
print("MIGRATION-CAP-OK")
"""


def test_pair_map_capacity_and_growth(tmp_path):
    """SLK_MIGRATION_MAP_LOG2=10 in a child process of its own (the variable is read when a handle is created; the child keeps it away
    from the other tests).  The policy (include/slacken_amd.h): the map doubles between calls while more than half full; one call
    that by itself brings more new pairs than the map has free slots gets SLK_E_CAPACITY and spends the handle."""
    script = tmp_path / "capacity.py"
    script.write_text(CAPACITY_SCRIPT.format(root=ROOT))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MIGRATION-CAP-OK" in p.stdout, (p.stdout + p.stderr)[-3000:]


class SparseTax:
    """what migration_model.depth reads of a taxonomy, for ids spread over 2^22: parents as an array, ranks by id"""

    class _Ranks(dict):
        def __missing__(self, key):
            return None

    def __init__(self, parents, ranks):
        self.parents, self.ranks = parents, SparseTax._Ranks(ranks)


def test_renumbered_reference_gives_the_callers_ids(world):
    import slacken_amd
    rng = np.random.default_rng(9)
    small, tax0 = world["parents"], world["tax"]
    extent = (1 << 22) + 5000
    parents, remap = taxgen.sparse_relabel(small, extent, rng)
    tax = SparseTax(parents, {remap[t]: tax0.ranks[t] for t in remap if t})
    depths = np.full(extent, -1, np.int32)
    for old, new in remap.items():
        depths[new] = mm.depth(tax0, old)
    assert all(mm.depth(tax, t) == depths[t] for t in list(remap.values()) + [5, extent - 1])
    ids = np.array(sorted(v for v in remap.values() if v), np.int32)
    rk = unique_keys(3000, rng)
    rt = rng.choice(ids, size=len(rk)).astype(np.int32)
    rt[:20] = ids.max()
    ix = slacken_amd.Index(expected_records=len(rk), max_taxon=extent - 1, device=0)
    ix.append(rk, rt)
    ix.set_taxonomy(parents)
    ix.finalize()
    assert ix.info().dense_taxa > 0                       # finalize renumbered the table's taxa
    st = ix.stream()
    ref = dict(zip(rk.tolist(), rt.tolist()))
    st1 = rng.choice(ids, size=len(rk)).astype(np.int32)
    st1[:4] = (1, 2**31 - 1, extent, extent + 12345)      # ROOT, the largest int32, ids past the taxonomy
    st1[4:8] = (-1, -2**31, 7, 1)                         # (the subject's taxon is never looked at: any int32 but 0 counts)
    for d, t in ((depths, tax), (None, None)):
        mig = slacken_amd.capi.MinimizerMigration(ix, d, stream=st)
        mig.add(rk, st1)
        want = check(mig, rk, st1, ref, t, with_depths=d is not None)
        by_t1 = {a: s for a, _, s, _ in want}
        assert all(by_t1[a] == (-100 if d is not None else 0) for a in (2**31 - 1, extent, extent + 12345, -1, -2**31))
        assert {b for _, b, _, _ in want} <= set(ids.tolist())
        mig.close()
    st.close()
    ix.close()


def test_refusals(world):
    import slacken_amd
    from slacken_amd import capi
    rng = np.random.default_rng(2)
    ix = slacken_amd.Index(expected_records=1000, max_taxon=50, device=0)
    ix.append(unique_keys(100, rng), np.full(100, 5, np.int32))
    with pytest.raises(slacken_amd.SlackenError) as e:     # not finalized
        capi.MinimizerMigration(ix, None, stream=world["st"])
    assert e.value.code == capi.E_STATE
    ix.close()
    wide = slacken_amd.Index(k=50, m=40, expected_records=1000, max_taxon=50, device=0)   # two id columns
    wide.append(rng.integers(1, 2**62, size=200, dtype=np.int64), np.full(100, 5, np.int32))
    wide.finalize()
    with pytest.raises(slacken_amd.SlackenError) as e:
        capi.MinimizerMigration(wide, None, stream=world["st"])
    assert e.value.code == capi.E_UNSUPPORTED
    wide.close()
    shard = slacken_amd.Index(expected_records=1000, max_taxon=50, device=0)
    shard.set_shard(0, 2)
    shard.append(unique_keys(100, rng), np.full(100, 5, np.int32))
    shard.finalize()
    with pytest.raises(slacken_amd.SlackenError) as e:
        capi.MinimizerMigration(shard, None, stream=world["st"])
    assert e.value.code == capi.E_UNSUPPORTED
    shard.close()
    # NULL arrays with n > 0: refused, nothing counted, the handle goes on
    mig = capi.MinimizerMigration(world["ix"], world["depths"], stream=world["st"])
    L = slacken_amd.lib()
    sk, st1 = world["sk"][:300], world["st1"][:300]
    mig.add(sk[:100], st1[:100])
    assert L.slk_migration_add(mig.h, world["st"].h, None, None, 5) == capi.E_INVALID
    assert L.slk_migration_add(mig.h, world["st"].h, sk.ctypes.data, None, 5) == capi.E_INVALID
    assert L.slk_migration_add_device(mig.h, world["st"].h, None, None, 5) == capi.E_INVALID
    assert L.slk_migration_add(mig.h, None, sk.ctypes.data, st1.ctypes.data, 5) == capi.E_INVALID
    n = C.c_uint64(0)
    assert L.slk_migration_result(mig.h, C.byref(n), None, None, None, None, 1, None, None) == capi.E_INVALID
    mig.add(sk[100:], st1[100:])
    want = check(mig, sk, st1, world["ref"], world["tax"])
    # a capacity below the number of triples is refused, the handle goes on
    assert len(want) > 3
    a = np.zeros(3, np.int32)
    c = np.zeros(3, np.uint64)
    assert L.slk_migration_result(mig.h, C.byref(n), a.ctypes.data, a.ctypes.data, a.ctypes.data, c.ctypes.data, 3, None,
                                  None) == capi.E_CAPACITY
    assert n.value == len(want)
    check(mig, sk, st1, world["ref"], world["tax"])
    mig.close()
    mig.close()


def test_lifetimes_and_a_shared_classify_stream(orc):
    import slacken_amd
    rng = np.random.default_rng(17)
    parents = taxgen.taxonomy(8 * 8, rng)
    p = orc.params()
    lib = synth.Library(orc, p, parents, n_genomes=4, genome_len=6000, pad_records=2000)
    ix = slacken_amd.Index(expected_records=len(lib.keys), max_taxon=len(parents) - 1, device=0)
    ix.append(lib.keys, lib.taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    st = ix.stream()
    reads = synth.make_reads(lib, 500, rng)
    bases, offsets = synth.pack(reads)
    before = st.classify_batch(bases, offsets, thresholds=(0.0,), with_hits=True)
    mig = slacken_amd.capi.MinimizerMigration(ix, None, stream=st)
    keys, taxa = np.asarray(lib.keys, np.int64), np.asarray(lib.taxa, np.int32)
    mig.add(keys[::2], taxa[::2])
    during = st.classify_batch(bases, offsets, thresholds=(0.0,), with_hits=True)
    mig.add(keys[1::2], taxa[1::2])
    t1, t2, steps, count, matched, unmatched = mig.result()
    mig.close()
    after = st.classify_batch(bases, offsets, thresholds=(0.0,), with_hits=True)
    for got in (during, after):
        for key in ("taxon", "classified", "num_distinct", "total_kmers", "num_hits"):
            assert np.array_equal(got[key], before[key]), key
    # a library against itself: every record matches and keeps its taxon; the arrays are the caller's, whatever became of the handle
    assert (matched, unmatched) == (int((taxa != 0).sum()), 0)
    assert np.array_equal(t1, t2) and int(count.sum()) == matched and not steps.any()
    st.close()
    ix.close()


@pytest.mark.parametrize("distinct", [1, 2, 3, 64])
def test_one_wave_of_few_pairs(big, distinct):
    """64 matched records, one wave, with 1, 2, 3 or 64 distinct (t1, t2) pairs: with three, lanes are left over after the two
    leader rounds and go to the block's map one by one"""
    import slacken_amd
    sk = big["rk"][:64].copy()                                    # all of them records of taxon 77
    st1 = (1 + np.arange(64) % distinct).astype(np.int32)
    mig = slacken_amd.capi.MinimizerMigration(big["ix"], None, stream=big["st"])
    mig.add(sk, st1)
    want = check(mig, sk, st1, big["ref"], None, with_depths=False)
    assert [(a, b) for a, b, _, _ in want] == [(t, 77) for t in range(1, distinct + 1)]
    mig.close()
