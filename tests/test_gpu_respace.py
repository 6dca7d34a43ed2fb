"""slk_index_respace (respace.hip) against respace_model.py: a resident library at s spaces becomes the library at more spaces on the
device -- keys masked, records regrouped by LCA -- and the result is an index like any other."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import respace_model as rm
import synth
import taxgen
from test_host_classify_gpu import GOLD

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_STATE = -1, -2, -6


def source(keys, taxa, parents, expected=None, spaces=7, max_taxon=None, finalize=True, taxonomy=True, m=31, k=35):
    import slacken_amd
    ix = slacken_amd.Index(k=k, m=m, spaces=spaces, expected_records=expected or max(len(taxa), 1),
                           max_taxon=max_taxon or len(parents) - 1)
    ix.append(keys, taxa)
    if taxonomy:
        ix.set_taxonomy(parents)
    if finalize:
        ix.finalize()
    return ix


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def gen(orc):
    g = rm.generate(3000, np.random.default_rng(712))
    g["model"] = rm.respace(g["keys"], g["taxa"], g["parents"], 31, 12)
    return g


def test_generated_library_7_to_12(gen):
    # (9 taxon bits: the source's table has the 2^13 buckets its cell layout asks for at least, whatever is expected, and does not grow;
    #  test_a_source_that_has_grown below is the same check on a source that did)
    src = source(gen["keys"], gen["taxa"], gen["parents"], expected=100)
    before = src.export(), src.taxon_counts()
    out = src.respace(12)
    got = out.export()
    assert same(got, gen["model"])
    info = out.info()
    assert info.records == len(gen["model"][0]) and info.duplicate_keys == 0 and info.grown == 0
    assert info.taxon_bits == src.info().taxon_bits and info.taxonomy_size == len(gen["parents"])
    assert out.spaces == 12
    again = src.respace(12)
    assert same(again.export(), got)
    after = src.export(), src.taxon_counts()
    assert same(before[0], after[0]) and same(before[1], after[1])
    t, c = out.taxon_counts()
    wt, wc = np.unique(gen["model"][1], return_counts=True)
    assert np.array_equal(t, wt) and np.array_equal(c, wc.astype(np.uint64))
    # the two are independent: the source may go first
    src.close()
    assert same(out.export(), got)


def test_a_source_that_has_grown(orc):
    """4 taxon bits, so that the source's table starts at 256 buckets and has to double on the way to 40 000 records"""
    rng = np.random.default_rng(99)
    parents = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10], np.int32)
    g = rm.generate(9000, rng, parents=parents)
    src = source(g["keys"], g["taxa"], parents, expected=500, max_taxon=15)
    assert src.info().grown >= 1 and src.info().records == len(g["keys"])
    out = src.respace(12)
    assert same(out.export(), rm.respace(g["keys"], g["taxa"], parents, 31, 12))
    assert out.info().grown == 0


def test_dense_ids(gen):
    rng = np.random.default_rng(5)
    sparse, remap = taxgen.sparse_relabel(gen["parents"], 2**22 + 5000, rng)
    lut = np.zeros(len(gen["parents"]), np.int32)
    for old, new in remap.items():
        lut[old] = new
    taxa = lut[gen["taxa"]]
    assert taxa.max() >= 2**22 and taxa.min() >= 1
    src = source(gen["keys"], taxa, sparse)
    assert src.info().dense_taxa > 0
    out = src.respace(12)
    assert out.info().dense_taxa == src.info().dense_taxa
    assert same(out.export(), (gen["model"][0], lut[gen["model"][1]]))
    assert same(out.export(), rm.respace(gen["keys"], taxa, sparse, 31, 12))


@pytest.mark.parametrize("s_new", [8, 15])
def test_one_step_and_the_widest_mask(orc, s_new):
    g = rm.generate(1500, np.random.default_rng(s_new), s_new=s_new)
    src = source(g["keys"], g["taxa"], g["parents"])
    assert same(src.respace(s_new).export(), rm.respace(g["keys"], g["taxa"], g["parents"], 31, s_new))


def test_chain_equals_one_step(gen):
    src = source(gen["keys"], gen["taxa"], gen["parents"])
    mid = src.respace(10)
    assert same(mid.export(), rm.respace(gen["keys"], gen["taxa"], gen["parents"], 31, 10))
    assert same(mid.respace(12).export(), gen["model"])
    assert same(src.respace(12).export(), gen["model"])


def golden():
    lib = np.load(os.path.join(GOLD, "library.npz"))
    keep = lib["taxa"] != 0
    return lib["keys"][keep], lib["taxa"][keep], lib["parents"]


def test_golden_library_has_nothing_to_merge(orc):
    keys, taxa, parents = golden()
    src = source(keys, taxa, parents)
    out = src.respace(12)
    masked = (keys.view(np.uint64) & np.uint64(rm.mask(31, 12))).view(np.int64)
    assert len(np.unique(masked)) == len(keys)
    o = np.argsort(masked, kind="stable")
    assert same(out.export(), (masked[o], taxa[o]))
    assert out.info().records == src.info().records


def test_one_record_and_none(orc):
    parents = taxgen.taxonomy(40, np.random.default_rng(1))
    key = np.array([rm.mask(31, 7) & 0x123456789ABCDEF0], np.uint64).view(np.int64)
    one = source(key, np.array([7], np.int32), parents).respace(9)
    assert same(one.export(), ((key.view(np.uint64) & np.uint64(rm.mask(31, 9))).view(np.int64), np.array([7], np.int32)))
    empty = source(np.zeros(0, np.int64), np.zeros(0, np.int32), parents).respace(9)
    assert empty.info().records == 0 and len(empty.export()[0]) == 0
    bases, offsets = synth.pack([synth.random_dna(150, np.random.default_rng(2)) for _ in range(10)])
    r = empty.stream().classify_batch(bases, offsets)
    assert not r["classified"].any() and r["taxon"].max() == 0
    assert np.array_equal(empty.lookup(key), [0]) and np.array_equal(one.lookup(one.export()[0]), [7])


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import slacken_amd
d = np.load(sys.argv[2])
ix = slacken_amd.Index(expected_records=len(d["keys"]), max_taxon=len(d["parents"]) - 1)
ix.append(d["keys"], d["taxa"]); ix.set_taxonomy(d["parents"]); ix.finalize()
out = ix.respace(12)
k, t = out.export()
i = out.info()
np.savez(sys.argv[3], keys=k, taxa=t, grown=i.grown, buckets=i.buckets, records=i.records, src_keys=ix.export()[0])
"""


def test_the_pass_repeats_when_the_table_is_too_small(orc, tmp_path):
    """SLK_RESPACE_BUCKETS=32 asks for the smallest first table.  With the 9 taxon bits of the generator's taxonomy a cell leaves room
    for the hash remainder only from 2^13 buckets on (64 = remainder 64 - q + taxon 9 + displacement 4), so the first table has
    65 536 cells whatever the variable says, and 5 000 records can never overflow it: 66 000 classes (265 000 records) do, by count."""
    from test_host_cli import ROOT
    g = rm.generate(66000, np.random.default_rng(4))
    want = rm.respace(g["keys"], g["taxa"], g["parents"], 31, 12)
    assert len(want[0]) == 66000 > 8192 * 8
    np.savez(tmp_path / "in.npz", keys=g["keys"], taxa=g["taxa"], parents=g["parents"])
    env = dict(os.environ, SLK_RESPACE_BUCKETS="32")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.load(tmp_path / "out.npz")
    assert same((got["keys"], got["taxa"]), want)
    assert int(got["grown"]) >= 1 and int(got["buckets"]) > 8192 and int(got["records"]) == 66000
    assert np.array_equal(got["src_keys"], np.sort(g["keys"]))


def test_the_result_classifies(orc):
    """reads against the respaced index = the oracle against the model's records under the new splitter, field for field"""
    rng = np.random.default_rng(31)
    parents = taxgen.taxonomy(8 * 32, rng)
    p7, p12 = orc.params(spaces=7), orc.params(spaces=12)
    lib = synth.Library(orc, p7, parents, n_genomes=8, genome_len=12000, pad_records=0)
    # a library at 7 spaces whose keys merge at 12: the genomes' records, and beside each of a third of them a sibling that differs
    # in the freed bits only, with another taxon
    bits = rm.free_bits(31, 7, 12)
    pick = rng.random(len(lib.keys)) < 0.33
    sib = (lib.keys[pick].view(np.uint64) ^ rm.deposit(rng.integers(1, 1 << len(bits), int(pick.sum())), bits)).view(np.int64)
    keys = np.concatenate([lib.keys, sib])
    taxa = np.concatenate([lib.taxa, rng.choice(taxgen.defined_taxa(parents), len(sib)).astype(np.int32)])
    keys, first = np.unique(keys, return_index=True)
    taxa = taxa[first]
    mk, mt = rm.respace(keys, taxa, parents, 31, 12)
    assert len(mk) < len(keys) - 100
    out = source(keys, taxa, parents).respace(12)
    assert same(out.export(), (mk, mt))
    st = out.stream()
    reads = synth.make_reads(lib, 2000, rng, n_single=0.1, n_run=0.05)
    bases, offsets = synth.pack(reads)
    thr = (0.0, 0.15)
    oix = orc.Index(1, mk, mt)
    want = orc.classify_batch(p12, oix, parents, bases, offsets, thresholds=thr)
    got = st.classify_batch(bases, offsets, thresholds=thr, with_hits=True)
    assert int(want["classified"][0].sum()) > 500
    fields = ("taxon", "classified", "num_distinct", "total_kmers", "num_hits")
    for key in fields:
        assert np.array_equal(got[key], want[key]), key
    fast = st.classify_batch(bases, offsets, thresholds=thr, with_hits=False)
    for key in fields[:4]:
        assert np.array_equal(fast[key], want[key]), key
    ho = got["hit_offsets"].astype(np.int64)
    for i in range(0, len(reads), 10):   # the hit lists themselves, read by read
        _, hits = orc.classify_read(p12, oix, parents, reads[i].tobytes(), None, 2, thr[0])
        g = got["hits"][ho[i]:ho[i + 1]]
        assert [(int(t), int(c)) for t, c in zip(g["taxon"], g["count"])] == hits
    r1, r2 = reads[:200], reads[200:400]
    m1, m2 = synth.pack(r1), synth.pack(r2)
    want = orc.classify_batch(p12, oix, parents, m1[0], m1[1], m2[0], m2[1], thresholds=thr)
    got = st.classify_batch(m1[0], m1[1], m2[0], m2[1], thresholds=thr, with_hits=True)
    for key in fields:
        assert np.array_equal(got[key], want[key]), ("paired", key)
    ho = got["hit_offsets"].astype(np.int64)
    for i in range(0, 200, 10):
        _, hits = orc.classify_read(p12, oix, parents, r1[i].tobytes(), r2[i].tobytes(), 2, thr[0])
        g = got["hits"][ho[i]:ho[i + 1]]
        assert [(int(t), int(c)) for t, c in zip(g["taxon"], g["count"])] == hits


def refused(ix, spaces, code):
    from slacken_amd import SlackenError
    with pytest.raises(SlackenError) as e:
        ix.respace(spaces)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals(gen, orc):
    import slacken_amd
    import torch
    keys, taxa, parents = gen["keys"][:4000], gen["taxa"][:4000], gen["parents"]
    bases, offsets = synth.pack([synth.random_dna(150, np.random.default_rng(2)) for _ in range(50)])

    def cycle():
        src = source(keys, taxa, parents)
        st = src.stream()
        want = st.classify_batch(bases, offsets, with_hits=False)
        before = src.export()

        def intact():
            got = st.classify_batch(bases, offsets, with_hits=False)
            assert all(np.array_equal(got[k], want[k]) for k in want) and same(src.export(), before)
        assert "not meaningful. (was 7, requested 7)" in refused(src, 7, E_INVALID)
        intact()
        assert "not meaningful" in refused(src, 3, E_INVALID)
        intact()
        refused(src, 16, E_INVALID)                                     # m / 2 + 1
        intact()
        open_ix = source(keys, taxa, parents, finalize=False)
        refused(open_ix, 12, E_STATE)
        open_ix.finalize()
        assert same(open_ix.respace(12).export(), rm.respace(keys, taxa, parents, 31, 12))
        no_tax = source(keys, taxa, parents, taxonomy=False)
        refused(no_tax, 12, E_STATE)
        assert same(no_tax.export(), before)
        shard = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1)
        shard.set_shard(1, 2)
        shard.append(keys, taxa)
        shard.set_taxonomy(parents)
        shard.finalize()
        kept = shard.export()
        refused(shard, 12, E_UNSUPPORTED)
        assert same(shard.export(), kept) and 0 < len(kept[0]) < len(keys)
        wide = slacken_amd.Index(k=45, m=40, spaces=7, expected_records=64, max_taxon=len(parents) - 1)
        wide.append(np.arange(1, 21, dtype=np.int64).reshape(10, 2) << 20, taxa[:10])
        wide.set_taxonomy(parents)
        wide.finalize()
        refused(wide, 12, E_UNSUPPORTED)
        assert wide.info().records == 10
        for h in (st, src, open_ix, no_tax, shard, wide):
            h.close()

    free = []
    for _ in range(2):   # (the first cycle is the warm-up, as in tests/test_gpu_resources.py)
        cycle()
        gc.collect()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[0] - free[1] <= 0, f"the second cycle kept {free[0] - free[1]} bytes of device memory"
