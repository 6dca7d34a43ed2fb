"""slk_index_taxon_counts (taxstats.hip): the records per taxon of a resident table, counted on the device.  The expected value in
every case is numpy.unique over slk_index_export of the same index -- an independent, older path -- and, where the records are
known, the same computed from the inputs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import synth
import taxgen

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def distinct_keys(n, rng):
    """n distinct non-zero left-aligned 31-mers (the low two bits clear), shuffled"""
    k = np.unique(rng.integers(-2**63, 2**63, size=n + n // 16 + 64, dtype=np.int64) & ~np.int64(3))
    k = k[k != 0]
    rng.shuffle(k)
    assert len(k) >= n
    return k[:n].copy()


def by_export(ix):
    _, taxa = ix.export()
    t, c = np.unique(taxa, return_counts=True)
    return t.astype(np.int32), c.astype(np.uint64)


def by_inputs(taxa):
    t, c = np.unique(np.asarray(taxa, np.int32), return_counts=True)
    return t.astype(np.int32), c.astype(np.uint64)


def check(ix, taxa=None):
    """taxon_counts() == unique(export) (== unique(inputs)); returns the pairs"""
    got_t, got_c = ix.taxon_counts()
    assert got_t.dtype == np.int32 and got_c.dtype == np.uint64
    want_t, want_c = by_export(ix)
    assert np.array_equal(got_t, want_t) and np.array_equal(got_c, want_c)
    if taxa is not None:
        in_t, in_c = by_inputs(taxa)
        assert np.array_equal(got_t, in_t) and np.array_equal(got_c, in_c)
    return got_t, got_c


def raw(ix, capacity, with_arrays=True):
    """the C entry itself: (rc, taxa, counts, n_taxa, n_records)"""
    import slacken_amd
    taxa, counts = np.full(max(capacity, 1), -7, np.int32), np.full(max(capacity, 1), 77, np.uint64)
    n, total = C.c_uint64(123), C.c_uint64(456)
    rc = slacken_amd.lib().slk_index_taxon_counts(ix.h, taxa.ctypes.data if with_arrays else None,
                                                  counts.ctypes.data if with_arrays else None, capacity, C.byref(n), C.byref(total))
    return rc, taxa, counts, n.value, total.value


def make(keys, taxa, max_taxon, finalize=True, **kw):
    import slacken_amd
    ix = slacken_amd.Index(expected_records=kw.pop("expected_records", len(keys)), max_taxon=max_taxon, **kw)
    if len(keys):
        ix.append(keys, np.asarray(taxa, np.int32))
    if finalize:
        ix.finalize()
    return ix


def test_empty_index():
    ix = make(np.zeros(0, np.int64), [], 100)
    rc, _, _, n, total = raw(ix, 0, with_arrays=False)
    assert (rc, n, total) == (0, 0, 0)
    t, c = ix.taxon_counts()
    assert len(t) == 0 and len(c) == 0


def test_one_taxon_on_every_record():
    """every lane of every wave holds the same taxon: the wave's ballot count, and one 32-bit LDS counter per block takes it all"""
    rng = np.random.default_rng(1)
    keys = distinct_keys(200_000, rng)
    ix = make(keys, np.full(len(keys), 37, np.int32), 1000)
    t, c = check(ix, np.full(len(keys), 37))
    assert t.tolist() == [37] and c.tolist() == [200_000]
    assert raw(ix, 1)[4] == 200_000


def test_two_taxa_in_every_wave():
    """two taxa, alternating in the input (the table's order is the hash's): the second round of the ballot loop"""
    rng = np.random.default_rng(2)
    keys = distinct_keys(100_000, rng)
    taxa = np.where(np.arange(len(keys)) % 2 == 0, 5, 900).astype(np.int32)
    t, c = check(make(keys, taxa, 1000), taxa)
    assert t.tolist() == [5, 900] and c.tolist() == [50_000, 50_000]


@pytest.mark.parametrize("skewed", [False, True], ids=["uniform", "skewed"])
def test_more_taxa_than_a_block_map_holds(skewed):
    """5 000 taxa over 300 000 records: more than the 4 096 slots of a block's LDS map, so lanes take the direct route to the device
    counters; skewed: 95 % of the records on 8 taxa, the rest over the 5 000"""
    rng = np.random.default_rng(3 + skewed)
    keys = distinct_keys(300_000, rng)
    ids = rng.choice(np.arange(1, 60_000), size=5000, replace=False).astype(np.int32)
    taxa = rng.choice(ids, size=len(keys))
    if skewed:
        hot = rng.random(len(keys)) < 0.95
        taxa[hot] = rng.choice(ids[:8], size=int(hot.sum()))
    t, c = check(make(keys, taxa, 60_000), taxa)
    assert len(t) > 4096 and int(c.sum()) == 300_000
    if skewed:
        assert np.sort(c)[-8:].sum() > 0.94 * 300_000


def test_smallest_table_and_grid_tails(monkeypatch):
    """32 buckets with a dozen records (one block, most of its lanes past the table's end), and a table whose 16-byte elements
    are no multiple of the grid's stride, with grids of 1, 3 and the default number of blocks"""
    rng = np.random.default_rng(5)
    keys = distinct_keys(12, rng)
    ix = make(keys, np.ones(12, np.int32), 1)
    assert ix.info().buckets == 32
    t, c = check(ix, np.ones(12))
    assert t.tolist() == [1] and c.tolist() == [12]
    keys = distinct_keys(50_001, rng)
    taxa = rng.integers(1, 16, size=len(keys)).astype(np.int32)
    ix = make(keys, taxa, 15)                 # (4 taxon bits: the bucket count is free to be what the records need, 11 365)
    elements = ix.info().buckets * 4          # 16-byte loads; a block takes 512 x 4 of them per step
    for blocks in (None, 1, 3):
        if blocks:
            monkeypatch.setenv("SLK_TAXSTATS_BLOCKS", str(blocks))
            assert elements % (blocks * 2048) != 0
        check(ix, taxa)


def test_grown_table():
    rng = np.random.default_rng(6)
    keys = distinct_keys(120_000, rng)
    taxa = rng.integers(1, 16, size=len(keys)).astype(np.int32)
    # far too small: the table starts with 256 buckets (4 taxon bits, so that the cell layout asks for no more) and doubles on the way
    ix = make(keys, taxa, 15, expected_records=1000)
    assert ix.info().grown >= 1 and ix.info().records == len(keys)
    check(ix, taxa)


def test_dense_ids_leave_as_the_callers_ids():
    """ids beyond 2^22 with the taxonomy set before finalize: the cells hold dense internal ids, the pairs carry the caller's"""
    rng = np.random.default_rng(7)
    extent = (1 << 22) + 5000
    parents, remap = taxgen.sparse_relabel(taxgen.taxonomy(8 * 16, rng), extent, rng)
    ids = np.array(sorted(v for v in remap.values() if v), np.int32)
    assert ids.max() > (1 << 22)
    keys = distinct_keys(20_000, rng)
    taxa = rng.choice(ids, size=len(keys)).astype(np.int32)
    taxa[:50] = ids.max()
    import slacken_amd
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=extent - 1)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    assert ix.info().taxon_bits > 22
    before = check(ix, taxa)                   # not finalized: ids as given, beyond 22 bits
    ix.finalize()
    assert ix.info().dense_taxa > 0
    after = check(ix, taxa)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and after[0][-1] == ids.max()
    rc, t, c, n, total = raw(ix, len(after[0]) - 1)       # the prefix of a short capacity is in the caller's ids too
    assert rc == slacken_amd.capi.E_CAPACITY and np.array_equal(t, after[0][:-1]) and np.array_equal(c, after[1][:-1])


def test_ids_beyond_22_bits_without_a_taxonomy(monkeypatch):
    """No taxonomy to renumber by: the cells keep the caller's ids of more than 22 bits, finalized or not, and the device counters
    are a map instead of an array of 2^taxon_bits entries.  The largest id is max_taxon = 2^23 - 1.  (No table exists for ids near
    2^31 - 1: a cell has to hold remainder, displacement and taxon in 64 bits, which ends at 28 taxon bits with 2^32 buckets, and
    24 bits already cost a 16 GiB table.)  With SLK_TAXSTATS_MAP_LOG2=4 the map starts at 16 slots and doubles until it holds."""
    import slacken_amd
    with pytest.raises(slacken_amd.SlackenError) as e:
        slacken_amd.Index(expected_records=1000, max_taxon=2**31 - 1)
    assert e.value.code == slacken_amd.capi.E_CAPACITY
    rng = np.random.default_rng(8)
    keys = distinct_keys(60_000, rng)
    top = 2**23 - 1
    ids = np.unique(np.concatenate([rng.integers(1, top, size=3000), [1, 2**22, top - 1, top]])).astype(np.int32)
    taxa = rng.choice(ids, size=len(keys)).astype(np.int32)
    taxa[:4] = (1, 2**22, top - 1, top)
    taxa[4:20_000] = top
    for finalize in (False, True):
        ix = make(keys, taxa, top, finalize=finalize)
        assert ix.info().taxon_bits == 23 and ix.info().dense_taxa == 0
        t, c = check(ix, taxa)
        assert t[-1] == top and c[-1] >= 19_996
    monkeypatch.setenv("SLK_TAXSTATS_MAP_LOG2", "4")
    check(ix, taxa)


def test_flagged_buckets():
    """Load factor 0.8: some buckets fill up and records go past them, which sets the top bit of their first cells (TableGeom.flag)
    where the cell layout leaves one.  About 31 250 buckets (q = 15, not a power of two) and 4 taxon bits leave 15 - 4 - 1 = 10 bits:
    8 of displacement and the flag."""
    rng = np.random.default_rng(9)
    keys = distinct_keys(200_000, rng)
    taxa = rng.integers(1, 16, size=len(keys)).astype(np.int32)
    assert "SLK_NO_BUCKET_FLAG" not in os.environ
    ix = make(keys, taxa, 15, load_factor=0.8)
    info = ix.info()
    spare = info.bucket_bits - info.taxon_bits - (0 if info.buckets & (info.buckets - 1) == 0 else 1)
    assert spare - 1 >= 4                      # the geometry has the flag bit (index.hip: shape_of)
    assert info.max_displacement >= 1                             # ... and records went past full buckets: those are flagged
    check(ix, taxa)


def test_before_and_after_finalize():
    rng = np.random.default_rng(10)
    keys = distinct_keys(30_000, rng)
    parents = taxgen.taxonomy(8 * 32, rng)
    taxa = rng.choice(taxgen.defined_taxa(parents), size=len(keys)).astype(np.int32)
    import slacken_amd
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1)
    ix.append(keys[:10_000], taxa[:10_000])
    check(ix, taxa[:10_000])
    ix.append(keys[10_000:], taxa[10_000:])
    ix.set_taxonomy(parents)
    before = check(ix, taxa)
    ix.finalize()
    after = check(ix, taxa)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_dynamic_library(orc):
    """an index built by slk_index_add_sequences (the dynamic library of classify2): LCA records above the genomes' leaves"""
    import slacken_amd
    rng = np.random.default_rng(11)
    parents = taxgen.taxonomy(8 * 32, rng)
    lib = synth.Library(orc, orc.params(), parents, n_genomes=6, genome_len=8000)
    bases, offsets = synth.pack(lib.genomes)
    ix = slacken_amd.Index(expected_records=len(lib.keys) * 2, max_taxon=len(parents) - 1)
    ix.set_taxonomy(parents)
    ix.add_sequences(bases, offsets, lib.genome_taxa)
    t, c = check(ix, lib.taxa)
    assert len(t) > len(lib.genome_taxa)                  # shared stretches gave inner nodes records
    ix.finalize()
    check(ix, lib.taxa)


def test_a_shard_counts_its_own_share():
    import slacken_amd
    rng = np.random.default_rng(12)
    keys = distinct_keys(60_000, rng)
    taxa = rng.integers(1, 500, size=len(keys)).astype(np.int32)
    whole = check(make(keys, taxa, 500), taxa)
    total = {}
    for shard in range(3):
        ix = slacken_amd.Index(expected_records=len(keys) // 3 + 4096, max_taxon=500)
        ix.set_shard(shard, 3)
        ix.append(keys, taxa)
        ix.finalize()
        mine = np.array([slacken_amd.lib().slk_shard_of(int(k), 3) == shard for k in keys[:2000]])
        t, c = check(ix)                                  # == the export of that shard
        assert 0.2 * len(keys) < int(c.sum()) < 0.5 * len(keys) and mine.any() and not mine.all()
        for a, b in zip(t.tolist(), c.tolist()):
            total[a] = total.get(a, 0) + b
    assert sorted(total) == whole[0].tolist() and [total[a] for a in sorted(total)] == whole[1].tolist()


def test_capacity_protocol():
    import slacken_amd
    rng = np.random.default_rng(13)
    keys = distinct_keys(20_000, rng)
    taxa = rng.integers(1, 400, size=len(keys)).astype(np.int32)
    ix = make(keys, taxa, 400)
    want_t, want_c = by_inputs(taxa)
    n_taxa = len(want_t)
    rc, t, c, n, total = raw(ix, 0, with_arrays=False)                  # a query
    assert (rc, n, total) == (0, n_taxa, len(keys))
    rc, t, c, n, total = raw(ix, n_taxa - 1)                            # one short: the first pairs, SLK_E_CAPACITY
    assert rc == slacken_amd.capi.E_CAPACITY and "capacity" in slacken_amd.lib().slk_last_error().decode()
    assert (n, total) == (n_taxa, len(keys))
    assert np.array_equal(t, want_t[:-1]) and np.array_equal(c, want_c[:-1])
    rc, t, c, n, total = raw(ix, n_taxa)                                # exact
    assert (rc, n, total) == (0, n_taxa, len(keys)) and np.array_equal(t, want_t) and np.array_equal(c, want_c)
    rc, t, c, n, total = raw(ix, n_taxa + 5)                            # room to spare: nothing past the pairs is written
    assert rc == 0 and np.array_equal(t[:n_taxa], want_t) and (t[n_taxa:] == -7).all() and (c[n_taxa:] == 77).all()
    assert raw(ix, 4, with_arrays=False)[0] == slacken_amd.capi.E_INVALID


def test_wide_index_is_unsupported():
    import slacken_amd
    ix = slacken_amd.Index(k=50, m=40, expected_records=16, max_taxon=7)
    with pytest.raises(slacken_amd.SlackenError) as e:
        ix.taxon_counts()
    assert e.value.code == slacken_amd.capi.E_UNSUPPORTED and "32 nt" in str(e.value)


def test_index_is_unchanged_and_counts_are_deterministic():
    """the golden reads classify identically before and after a count; two counts give equal arrays"""
    import slacken_amd
    g = json.load(open(os.path.join(GOLD, "golden_classify.json")))
    reads = [line.rstrip("\n").split("\t") for line in open(os.path.join(GOLD, "reads.tsv"))]
    lib = np.load(os.path.join(GOLD, "library.npz"))
    ix = slacken_amd.Index(k=g["k"], m=g["m"], spaces=g["spaces"], expected_records=len(lib["keys"]), max_taxon=len(lib["parents"]) - 1)
    ix.append(lib["keys"], lib["taxa"])
    ix.set_taxonomy(lib["parents"])
    ix.finalize()
    st = ix.stream()
    bases, offsets = synth.pack([np.frombuffer(s.encode(), np.uint8) for _, s in reads])
    classify = lambda: st.classify_batch(bases, offsets, thresholds=g["thresholds"], min_hit_groups=g["min_hit_groups"])   # noqa: E731
    before, exported = classify(), ix.export()
    first = check(ix, lib["taxa"][lib["taxa"] != 0])
    second = ix.taxon_counts()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    after, exported2 = classify(), ix.export()
    for key in ("taxon", "classified", "num_distinct", "total_kmers", "hit_offsets"):
        assert np.array_equal(before[key], after[key]), key
    for field in ("taxon", "count"):
        assert np.array_equal(before["hits"][field], after["hits"][field])
    want = np.array([r[f"c{g['thresholds'][0]}"] for r in g["reads"]])
    assert np.array_equal(after["taxon"][0], want[:, 0])
    assert np.array_equal(exported[0], exported2[0]) and np.array_equal(exported[1], exported2[1])


@pytest.mark.parametrize("distinct", [1, 2, 3, 64])
def test_waves_of_few_taxa(distinct):
    """8 000 records in the smallest table that seven taxon bits allow (2 048 buckets: half full, so a wave's 128 cells hold some 64
    records) with 1, 2, 3 or 64 distinct taxa: with three, lanes are left over after the two leader rounds of nearly every wave.
    The taxa are 63 and up in a domain of 128 ids: with 64 of them the pairs straddle the border between the two waves of the pairs
    kernel, with 2 the second of these waves has a single holder (id 64) and the first one other (id 63)."""
    rng = np.random.default_rng(50 + distinct)
    keys = distinct_keys(8000, rng)
    taxa = (63 + np.arange(len(keys)) % distinct).astype(np.int32)
    ix = make(keys, taxa, 127)
    assert ix.info().buckets == 2048
    t, c = check(ix, taxa)
    assert t.tolist() == list(range(63, 63 + distinct)) and int(c.sum()) == len(keys)
