"""slk_index_export_range (export.hip): a bucket range of a resident table as records, in any order or grouped by Spark's bucket.
The expected records are those of slk_index_export -- the older path over the whole table -- or the inputs themselves; the expected
group of a key is murmur3_long of test_respace_cli.py, a restatement of Spark's hash that shares nothing with the engine."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
import taxgen
from test_gpu_taxstats import distinct_keys
from test_respace_cli import murmur3_long

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_key(keys, taxa):
    o = np.argsort(keys, kind="stable")
    return keys[o], taxa[o]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def union(pieces):
    """the pieces' records sorted by key; no key twice"""
    keys = np.concatenate([p[0] for p in pieces]) if pieces else np.zeros(0, np.int64)
    taxa = np.concatenate([p[1] for p in pieces]) if pieces else np.zeros(0, np.int32)
    assert len(np.unique(keys)) == len(keys)
    return by_key(keys, taxa)


def tiles(ix, cuts, n_groups=0):
    return [ix.export_range(a, b, n_groups) for a, b in zip(cuts[:-1], cuts[1:])]


def check_grouped(got, n_groups, want):
    """offsets non-decreasing from 0 to n; every key in its Spark bucket; the multiset is the ungrouped piece's"""
    keys, taxa, offs = got
    assert offs.dtype == np.uint64 and len(offs) == n_groups + 1
    sizes = np.diff(offs.astype(np.int64))
    assert offs[0] == 0 and offs[-1] == len(keys) == len(taxa) and (sizes >= 0).all()
    groups = np.repeat(np.arange(n_groups), sizes)
    for k, g in zip(keys.tolist(), groups.tolist()):
        assert murmur3_long(k) % n_groups == g            # (Python's % is pmod)
    assert same(by_key(keys, taxa), by_key(*want))


def make(keys, taxa, max_taxon, finalize=True, **kw):
    import slacken_amd
    ix = slacken_amd.Index(expected_records=kw.pop("expected_records", len(keys)), max_taxon=max_taxon, **kw)
    ix.append(keys, np.asarray(taxa, np.int32))
    if finalize:
        ix.finalize()
    return ix


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2301)
    keys = distinct_keys(20_000, rng)
    assert (keys < 0).sum() > 5000                          # negative keys among them
    taxa = rng.integers(1, 500, size=len(keys)).astype(np.int32)
    ix = make(keys, taxa, 500)
    whole = ix.export()
    assert same(whole, by_key(keys, taxa))
    return dict(ix=ix, keys=keys, taxa=taxa, whole=whole, buckets=int(ix.info().buckets))


def test_tiling(table):
    ix, nb, whole = table["ix"], table["buckets"], table["whole"]
    assert ix.info().bucket_cells == 8 and nb > 64
    cuts = [0, 1, 7, 8, 9, nb // 2, nb - 1, nb]              # a range of one bucket ([7, 8), [8, 9), the last) among them
    pieces = tiles(ix, cuts)
    assert all(k.dtype == np.int64 and t.dtype == np.int32 and len(k) == len(t) <= 8 * (b - a)
               for (k, t), a, b in zip(pieces, cuts[:-1], cuts[1:]))
    assert same(union(pieces), whole)
    for step in (8, 9, nb):                                  # ranges of 8 buckets (one wave of cells), of 9, the whole table
        got = list(ix.export_pieces(step))
        assert len(got) == -(-nb // step) and same(union(got), whole)
    for a in (0, 5, nb):                                     # an empty range
        k, t = ix.export_range(a, a)
        assert len(k) == 0 and len(t) == 0
        k, t, offs = ix.export_range(a, a, 7)
        assert len(k) == 0 and offs.tolist() == [0] * 8


def test_ranges_of_empty_buckets():
    """a dozen records in the smallest table their cells allow (256 buckets with 4 taxon bits): most buckets hold nothing"""
    rng = np.random.default_rng(2302)
    keys = distinct_keys(12, rng)
    ix = make(keys, np.arange(1, 13, dtype=np.int32), 15)
    nb = int(ix.info().buckets)
    assert nb <= 256
    singles = [ix.export_range(b, b + 1) for b in range(nb)]
    empty = [b for b, (k, _) in enumerate(singles) if len(k) == 0]
    assert len(empty) >= nb - 12 and same(union(singles), by_key(keys, np.arange(1, 13, dtype=np.int32)))
    run = next(b for b in empty if b + 1 in empty)           # two empty buckets side by side
    assert len(ix.export_range(run, run + 2)[0]) == 0
    k, t, offs = ix.export_range(run, run + 2, 5)
    assert len(k) == 0 and offs.tolist() == [0] * 6


def test_full_buckets():
    """load factor 0.85: buckets fill up and records go past them (flagged first cells, displacements above 0)"""
    rng = np.random.default_rng(2303)
    keys = distinct_keys(50_000, rng)
    taxa = rng.integers(1, 16, size=len(keys)).astype(np.int32)
    ix = make(keys, taxa, 15, load_factor=0.85)
    info = ix.info()
    assert info.max_displacement >= 1 and info.records == len(keys)
    nb = int(info.buckets)
    assert same(union(list(ix.export_pieces(8))), by_key(keys, taxa))
    mid = nb // 2
    piece = ix.export_range(mid - 40, mid + 41)
    assert len(piece[0]) > 0.7 * 81 * 8
    check_grouped(ix.export_range(mid - 40, mid + 41, 7), 7, piece)
    check_grouped(ix.export_range(0, nb, 200), 200, by_key(keys, taxa))


@pytest.mark.parametrize("n_groups", [1, 2, 7, 200, 100_000])
def test_grouping(table, n_groups):
    """the whole table and a piece of it; 100 000 groups are beyond a block's LDS counters and take the device counters"""
    ix, nb = table["ix"], table["buckets"]
    check_grouped(ix.export_range(0, nb, n_groups), n_groups, table["whole"])
    a, b = nb // 3, nb // 3 + 777
    check_grouped(ix.export_range(a, b, n_groups), n_groups, ix.export_range(a, b))


def test_more_groups_than_records(table):
    ix = table["ix"]
    piece = ix.export_range(16, 20)
    assert 0 < len(piece[0]) <= 32
    check_grouped(ix.export_range(16, 20, 1000), 1000, piece)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import slacken_amd
d = np.load(sys.argv[2])
ix = slacken_amd.Index(expected_records=len(d["keys"]), max_taxon=500)
ix.append(d["keys"], d["taxa"])
ix.finalize()
nb = int(ix.info().buckets)
out = {}
for g in (7, 200):
    out[f"k{g}"], out[f"t{g}"], out[f"o{g}"] = ix.export_range(0, nb, g)
    out[f"pk{g}"], out[f"pt{g}"], out[f"po{g}"] = ix.export_range(nb // 3, nb // 3 + 777, g)
np.savez(sys.argv[3], buckets=nb, **out)
"""


def test_grouping_without_lds_counters(table, tmp_path):
    """SLK_EXPORT_LDS_GROUPS=4 in a child process: 7 and 200 groups take the device counters there, the LDS histogram here"""
    (tmp_path / "child.py").write_text(CHILD)
    np.savez(tmp_path / "in.npz", keys=table["keys"], taxa=table["taxa"])
    env = dict(os.environ, SLK_EXPORT_LDS_GROUPS="4")
    r = subprocess.run([sys.executable, str(tmp_path / "child.py"), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    d = np.load(tmp_path / "out.npz")
    ix, nb = table["ix"], table["buckets"]
    assert int(d["buckets"]) == nb
    a, b = nb // 3, nb // 3 + 777
    for g in (7, 200):
        check_grouped((d[f"k{g}"], d[f"t{g}"], d[f"o{g}"]), g, table["whole"])
        check_grouped((d[f"pk{g}"], d[f"pt{g}"], d[f"po{g}"]), g, ix.export_range(a, b))
        assert np.array_equal(d[f"o{g}"], ix.export_range(0, nb, g)[2])      # both routes: the same groups


def test_grown_table():
    rng = np.random.default_rng(2304)
    keys = distinct_keys(40_000, rng)
    taxa = rng.integers(1, 16, size=len(keys)).astype(np.int32)
    ix = make(keys, taxa, 15, expected_records=1000)
    assert ix.info().grown > 0 and ix.info().records == len(keys)
    nb = int(ix.info().buckets)
    assert same(union(list(ix.export_pieces(nb // 5 + 1))), by_key(keys, taxa))
    check_grouped(ix.export_range(0, nb, 7), 7, by_key(keys, taxa))


def test_before_and_after_finalize_with_renumbered_taxa():
    """ids beyond 2^22 with the taxonomy set: finalize renumbers the cells' taxa, the records still carry the caller's ids"""
    import slacken_amd
    rng = np.random.default_rng(2305)
    extent = 1 << 23
    parents, remap = taxgen.sparse_relabel(taxgen.taxonomy(8 * 16, rng), extent, rng)
    ids = np.array(sorted(v for v in remap.values() if v), np.int32)
    assert ids.max() > (1 << 22)
    keys = distinct_keys(8000, rng)
    taxa = rng.choice(ids, size=len(keys)).astype(np.int32)
    taxa[:50] = ids.max()
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=extent - 1)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    assert ix.info().taxon_bits > 22
    nb, want = int(ix.info().buckets), by_key(keys, taxa)
    for finalized in (False, True):
        if finalized:
            ix.finalize()
            assert ix.info().dense_taxa > 0
        assert same(union(list(ix.export_pieces(nb // 3 + 1))), want)
        check_grouped(ix.export_range(0, nb, 200), 200, want)


def test_dynamic_library(orc):
    import slacken_amd
    rng = np.random.default_rng(2306)
    parents = taxgen.taxonomy(8 * 32, rng)
    p = orc.params()
    lib = synth.Library(orc, p, parents, n_genomes=5, genome_len=6000)
    bases, offsets = synth.pack(lib.genomes)
    want = by_key(*orc.build_records(p, parents, bases, offsets, np.asarray(lib.genome_taxa, np.int32)))
    assert 2000 <= len(want[0]) <= 50_000
    ix = slacken_amd.Index(expected_records=len(want[0]) * 2, max_taxon=len(parents) - 1)
    ix.set_taxonomy(parents)
    ix.add_sequences(bases, offsets, lib.genome_taxa)
    nb = int(ix.info().buckets)
    assert same(union(list(ix.export_pieces(nb // 4 + 1))), want)
    check_grouped(ix.export_range(0, nb, 7), 7, want)


def test_a_shard_exports_its_own_share():
    import slacken_amd
    rng = np.random.default_rng(2307)
    keys = distinct_keys(30_000, rng)
    taxa = rng.integers(1, 500, size=len(keys)).astype(np.int32)
    shares = []
    for shard in range(3):
        ix = slacken_amd.Index(expected_records=len(keys) // 3 + 4096, max_taxon=500)
        ix.set_shard(shard, 3)
        ix.append(keys, taxa)
        ix.finalize()
        nb = int(ix.info().buckets)
        mine = union(list(ix.export_pieces(nb // 2 + 1)))
        assert same(mine, ix.export()) and 0.2 * len(keys) < len(mine[0]) < 0.5 * len(keys)
        assert all(slacken_amd.lib().slk_shard_of(int(k), 3) == shard for k in mine[0][:500])
        check_grouped(ix.export_range(0, nb, 7), 7, mine)
        shares.append(mine)
    assert same(union(shares), by_key(keys, taxa))


def raw(ix, b0, b1, n_groups, capacity, with_arrays=True, with_offsets=True):
    """the C entry itself: (rc, keys, taxa, offsets, n_records)"""
    import slacken_amd
    keys, taxa = np.full(max(capacity, 1), -7, np.int64), np.full(max(capacity, 1), -7, np.int32)
    offs = np.full(max(n_groups, 0) + 1, 77, np.uint64)
    n = C.c_uint64(123)
    rc = slacken_amd.lib().slk_index_export_range(ix.h, b0, b1, n_groups, keys.ctypes.data if with_arrays else None,
                                                  taxa.ctypes.data if with_arrays else None, capacity,
                                                  offs.ctypes.data if with_offsets else None, C.byref(n))
    return rc, keys, taxa, offs, n.value


def test_capacity_protocol(table):
    import slacken_amd
    ix, nb, n = table["ix"], table["buckets"], len(table["keys"])
    for g in (0, 7):
        rc, _, _, _, got = raw(ix, 0, nb, g, 0, with_arrays=False, with_offsets=False)     # the count query
        assert (rc, got) == (0, n)
        rc, _, _, _, got = raw(ix, 0, nb, g, n - 1)                                         # one short: the full count
        assert rc == slacken_amd.capi.E_CAPACITY and got == n and "capacity" in slacken_amd.lib().slk_last_error().decode()
        rc, k, t, offs, got = raw(ix, 0, nb, g, n)                                          # exact
        assert (rc, got) == (0, n) and same(by_key(k, t), table["whole"])
        rc, k, t, offs, got = raw(ix, 0, nb, g, n + 5)                                      # nothing past the records is written
        assert rc == 0 and same(by_key(k[:n], t[:n]), table["whole"]) and (k[n:] == -7).all() and (t[n:] == -7).all()
        assert int(offs[-1]) == (n if g else 77)                                            # (ungrouped: group_offsets is ignored)
    a, b = nb // 2, nb // 2 + 100
    rc, _, _, _, part = raw(ix, a, b, 0, 0, with_arrays=False)
    assert rc == 0 and part == len(ix.export_range(a, b)[0]) <= 800
    for g in (0, 7):                                                                        # an empty range: SLK_OK, 0 records
        assert raw(ix, 3, 3, g, 0, with_arrays=False)[::4] == (0, 0) and raw(ix, 3, 3, g, 16)[::4] == (0, 0)


def test_errors(table, monkeypatch):
    import slacken_amd
    capi = slacken_amd.capi
    ix, nb = table["ix"], table["buckets"]
    assert raw(ix, 5, 4, 0, 64)[0] == capi.E_INVALID                    # bucket0 > bucket1
    assert raw(ix, 0, nb + 1, 0, 64)[0] == capi.E_INVALID               # bucket1 > buckets
    assert raw(ix, nb + 1, nb + 1, 0, 64)[0] == capi.E_INVALID
    assert raw(ix, 0, 4, -1, 64)[0] == capi.E_INVALID                   # n_groups < 0
    assert raw(ix, 0, 4, 0, 64, with_arrays=False)[0] == capi.E_INVALID  # a capacity without buffers
    assert raw(ix, 0, 4, 3, 64, with_offsets=False)[0] == capi.E_INVALID
    wide = slacken_amd.Index(k=50, m=40, expected_records=16, max_taxon=7)
    with pytest.raises(slacken_amd.SlackenError) as e:
        wide.export_range(0, 1)
    assert e.value.code == capi.E_UNSUPPORTED and "32 nt" in str(e.value)
    # a spent index: its table was lost while it grew through host memory (the allocation of the new table counted as failed)
    rng = np.random.default_rng(2308)
    keys = distinct_keys(40_000, rng)
    lost = slacken_amd.Index(expected_records=1000, max_taxon=15)
    monkeypatch.setenv("SLK_GROW_VIA_HOST", "1")
    monkeypatch.setenv("SLK_GROW_LOSE_TABLE", "1")
    with pytest.raises(slacken_amd.SlackenError) as e:
        lost.append(keys, np.ones(len(keys), np.int32))
    assert e.value.code == capi.E_HIP
    monkeypatch.delenv("SLK_GROW_VIA_HOST")
    monkeypatch.delenv("SLK_GROW_LOSE_TABLE")
    assert raw(lost, 0, 1, 0, 0, with_arrays=False)[0] == capi.E_STATE
    assert raw(lost, 0, 1, 7, 64)[0] == capi.E_STATE


def test_a_grouped_call_covers_at_most_2_to_the_32_cells():
    """an empty table of more than 2^29 buckets (35 GB): the grouped call over all of it is refused, 2^29 buckets are taken, and the
    ungrouped call streams cells whose indices pass 2^32"""
    import slacken_amd
    ix = slacken_amd.Index(expected_records=2_400_000_000, max_taxon=15, load_factor=0.55)
    nb = int(ix.info().buckets)
    assert nb > 2**29 and ix.info().bucket_cells == 8
    keys = np.array([12, -16, 2**62 + 4, -2**63 + 8], np.int64)
    ix.append(keys, np.array([1, 2, 3, 4], np.int32))
    rc = raw(ix, 0, nb, 1, 16)
    assert rc[0] == slacken_amd.capi.E_INVALID and "pieces" in slacken_amd.lib().slk_last_error().decode()
    assert raw(ix, 0, 2**29 + 1, 3, 0, with_arrays=False)[0] == slacken_amd.capi.E_INVALID
    rc, k, t, offs, n = raw(ix, 0, nb, 0, 16)
    assert (rc, n) == (0, 4) and same(by_key(k[:4], t[:4]), by_key(keys, np.array([1, 2, 3, 4], np.int32)))
    first = raw(ix, 0, 2**29, 2, 16)
    rest = raw(ix, 2**29, nb, 2, 16)
    assert first[0] == 0 and rest[0] == 0 and first[4] + rest[4] == 4
    got = union([(first[1][:first[4]], first[2][:first[4]]), (rest[1][:rest[4]], rest[2][:rest[4]])])
    assert same(got, by_key(keys, np.array([1, 2, 3, 4], np.int32)))
