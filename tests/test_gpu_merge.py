"""slk_index_merge_records[_device] and slk_index_merge_index (merge.hip) against merge_model.py and the oracle's build_records:
the records of the parts, merged per key by LCA in any order, any chunking, from arrays or from a resident table, are the records of
the library built from the whole.  Everything through slacken_amd.Index, compared as sorted (key, taxon) arrays."""
import itertools

import numpy as np
import pytest

import merge_model as mm
import synth
import taxgen

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_STATE = -1, -2, -6
PARTS = [range(0, 7), range(7, 13), range(13, 20)]


def fresh(parents, expected=1 << 17, taxonomy=True, **kw):
    import slacken_amd
    kw.setdefault("max_taxon", len(parents) - 1)
    ix = slacken_amd.Index(expected_records=expected, **kw)
    if taxonomy:
        ix.set_taxonomy(parents)
    return ix


def built(w, idx, parents=None, taxa=None, **kw):
    """an index holding the sequences idx, added as sequences"""
    ix = fresh(w["parents"] if parents is None else parents, **kw)
    bases, offsets = mm.pack([w["seqs"][i] for i in idx])
    ix.add_sequences(bases, offsets, [(w["taxa"] if taxa is None else taxa)[i] for i in idx])
    return ix


@pytest.fixture(scope="module")
def world(orc):
    rng = np.random.default_rng(1923)
    parents = taxgen.taxonomy(60, rng)
    seqs, taxa = mm.sequences(rng, 20, parents)
    w = dict(p=orc.params(), parents=parents, seqs=seqs, taxa=taxa, rng=rng)
    w["whole"] = mm.build_records(w["p"], parents, seqs, taxa)
    # each part built on the device in an index of its own and exported: what a library on disk holds
    w["parts"] = []
    for idx in PARTS:
        ix = built(w, idx)
        w["parts"].append(ix.export())
        assert mm.same(w["parts"][-1], mm.build_records(w["p"], parents, [seqs[i] for i in idx], [taxa[i] for i in idx]))
        ix.close()
    shared = sum(len(p[0]) for p in w["parts"]) - len(w["whole"][0])
    assert shared >= 0.10 * len(w["whole"][0]) and len(w["whole"][0]) > 20_000
    # a smaller record set for the tests that make many calls: the records of 1500 keys that several parts hold, filled up with
    # others to 4 * 256 * 4 + 1, in random order
    keys = np.concatenate([p[0] for p in w["parts"]])
    tx = np.concatenate([p[1] for p in w["parts"]])
    uniq, counts = np.unique(keys, return_counts=True)
    hot = np.isin(keys, uniq[counts > 1][:1500])
    order = np.concatenate([np.flatnonzero(hot), np.flatnonzero(~hot)])[:4 * 256 * 4 + 1]
    order = order[rng.permutation(len(order))]
    w["small"] = keys[order], tx[order]
    w["small_model"] = mm.as_arrays(mm.merge(parents, [w["small"]]))
    assert len(w["small_model"][0]) < len(order) - 1500 + 1
    return w


# ---- 1. parts against the whole --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(itertools.permutations(range(3))), ids=lambda o: "".join(map(str, o)))
def test_parts_merged_in_every_order_are_the_whole(world, order):
    ix = fresh(world["parents"])
    for i in order:
        ix.merge_records(*world["parts"][i])
    assert mm.same(ix.export(), world["whole"])
    info = ix.info()
    assert info.records == len(world["whole"][0]) and info.duplicate_keys == 0


@pytest.mark.parametrize("sequences_first", [True, False])
def test_one_part_as_sequences_the_others_as_records(world, sequences_first):
    ix = fresh(world["parents"])
    bases, offsets = mm.pack([world["seqs"][i] for i in PARTS[1]])
    seq_taxa = [world["taxa"][i] for i in PARTS[1]]
    if sequences_first:
        ix.add_sequences(bases, offsets, seq_taxa)
    ix.merge_records(*world["parts"][0])
    ix.merge_records(*world["parts"][2])
    if not sequences_first:
        ix.add_sequences(bases, offsets, seq_taxa)
    assert mm.same(ix.export(), world["whole"]) and ix.info().records == len(world["whole"][0])


# ---- 2. chunking and borders -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4 * 256 * 4 + 1])
def test_calls_of_n_records(world, n):
    keys, taxa = world["small"]
    ix = fresh(world["parents"], expected=8192)
    for a in range(0, len(keys), n):
        ix.merge_records(keys[a:a + n], taxa[a:a + n])
    assert mm.same(ix.export(), world["small_model"]) and ix.info().records == len(world["small_model"][0])


def test_records_on_the_device(world):
    import torch
    keys, taxa = world["small"]
    d_k, d_t = torch.from_numpy(keys).cuda(), torch.from_numpy(taxa).cuda()
    torch.cuda.synchronize()
    ix = fresh(world["parents"], expected=8192)
    cut = 1000
    ix.merge_records_device(d_k.data_ptr(), d_t.data_ptr(), cut)
    ix.merge_records_device(d_k.data_ptr() + 8 * cut, d_t.data_ptr() + 4 * cut, len(keys) - cut)
    assert mm.same(ix.export(), world["small_model"])
    ix.merge_records_device(d_k.data_ptr(), d_t.data_ptr(), len(keys))     # idempotent
    assert mm.same(ix.export(), world["small_model"]) and ix.info().records == len(world["small_model"][0])


# ---- 3. one call, one cell -------------------------------------------------------------------------------------------------------
def test_many_lanes_on_eight_keys(world):
    rng = np.random.default_rng(3)
    parents = world["parents"]
    eight = world["whole"][0][:: len(world["whole"][0]) // 8][:8]
    keys = eight[rng.integers(0, 8, 1 << 14)]
    taxa = rng.choice(np.array(taxgen.defined_taxa(parents), np.int32), size=1 << 14)
    ix = fresh(parents, expected=1024)
    ix.merge_records(keys, taxa)
    want = mm.as_arrays(mm.merge(parents, [(keys, taxa)]))
    assert len(want[0]) == 8 and mm.same(ix.export(), want) and ix.info().records == 8


# ---- 4. a table under load ---------------------------------------------------------------------------------------------------------
SMALL_TREE = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10], np.int32)


@pytest.fixture(scope="module")
def many(orc):
    """9 * 10^4 random keys under a tree of 14 nodes, and 3 * 10^4 further records that repeat some of them with other taxa.  (4 taxon
    bits: a table of 2^9 buckets is allowed, so few expected records mean a small table, and at 2^14 buckets the cells have the 8
    displacement bits a load of 0.85 asks for -- with the 7 bits of the other tests' taxa either takes ten times the records.)"""
    rng = np.random.default_rng(45)
    uniq = np.unique(rng.integers(-2**63, 2**63 - 1, 90_000, dtype=np.int64))
    keys = np.concatenate([uniq, rng.choice(uniq, 30_000)])
    taxa = rng.integers(1, len(SMALL_TREE), len(keys)).astype(np.int32)
    order = rng.permutation(len(keys))
    keys, taxa = keys[order], taxa[order]
    model = mm.as_arrays(mm.merge(SMALL_TREE, [(keys, taxa)]))
    assert len(model[0]) == len(uniq) and (model[1] == 1).sum() > 1000      # (merges that walked to the root)
    return dict(keys=keys, taxa=taxa, model=model)


def test_a_table_under_load(many):
    keys, taxa, model = many["keys"], many["taxa"], many["model"]
    ix = fresh(SMALL_TREE, expected=len(model[0]), load_factor=0.85, max_taxon=15)
    for a in range(0, len(keys), 40_000):
        ix.merge_records(keys[a:a + 40_000], taxa[a:a + 40_000])
    info = ix.info()
    assert info.grown == 0 and info.records / (info.buckets * info.bucket_cells) > 0.8
    assert info.max_displacement >= 1            # merges found their records away from the home bucket
    assert mm.same(ix.export(), model)
    ix.finalize()
    assert np.array_equal(ix.lookup(model[0]), model[1])         # the buckets' "a record went past" flag is intact
    for bit in (0, 17, 40):
        near = (model[0].view(np.uint64) ^ np.uint64(1 << bit)).view(np.int64)
        miss = ~np.isin(near, model[0])
        assert miss.sum() > 0.99 * len(near) and not ix.lookup(near[miss]).any()


# ---- 5. growth -------------------------------------------------------------------------------------------------------------------
def test_growth(many):
    keys, taxa, model = many["keys"], many["taxa"], many["model"]
    ix = fresh(SMALL_TREE, expected=1024, max_taxon=15)
    assert ix.info().buckets * ix.info().bucket_cells < len(model[0]) // 4
    for a in range(0, len(keys), 40_000):
        ix.merge_records(keys[a:a + 40_000], taxa[a:a + 40_000])
    info = ix.info()
    assert info.grown >= 1
    assert mm.same(ix.export(), model)
    assert info.records == len(model[0]) and info.duplicate_keys == 0


# ---- 6. remap and refusals of records --------------------------------------------------------------------------------------------
def failing(call, *args):
    import slacken_amd
    with pytest.raises(slacken_amd.SlackenError) as e:
        call(*args)
    return e.value


def test_remap_and_a_taxon_without_a_node(world):
    parents = world["parents"]
    keys, taxa = world["small"]
    used = np.unique(taxa)
    a, b, gone = int(used[0]), int(used[1]), int(used[-1])
    remap = np.arange(len(parents), dtype=np.int32)
    remap[a] = remap[b] = int(used[2])          # two source taxa to one node
    remap[gone] = 0                             # one to nothing
    want = mm.as_arrays(mm.merge(parents, [(keys, taxa)], remaps=[remap]))
    n_bad = int((taxa == gone).sum())
    assert n_bad > 0
    ix = fresh(parents, expected=8192)
    ix.set_merge_remap(remap)
    e = failing(ix.merge_records, keys, taxa)
    assert e.code == E_INVALID and f"{n_bad} records name a taxon the destination's taxonomy does not define (smallest: {gone})" in str(e)
    assert mm.same(ix.export(), want)
    # a remap shorter than the ids it meets: beyond it there is no node
    ix2 = fresh(parents, expected=8192)
    ix2.set_merge_remap(remap[:gone])
    n_beyond = int((taxa >= gone).sum())
    e = failing(ix2.merge_records, keys, taxa)
    assert e.code == E_INVALID and f"{n_beyond} records" in str(e) and f"(smallest: {int(taxa[taxa >= gone].min())})" in str(e)
    # cleared, the same index takes the records as they are: it went on working
    ix.set_merge_remap(None)
    ix.merge_records(keys, taxa)
    assert mm.same(ix.export(), mm.merge(parents, [want, (keys, taxa)]))


def test_bad_taxa_without_a_remap(world):
    parents = world["parents"].copy()
    undefined = int(max(t for t in taxgen.defined_taxa(parents) if t not in world["taxa"] and t not in parents))
    parents[undefined] = 0                       # a leaf no record names: now an id without a node
    keys, taxa = world["small"]
    keys, taxa = keys[:2000].copy(), taxa[:2000].copy()
    assert undefined not in taxa
    taxa[10], taxa[500], taxa[1999] = -7, len(parents), undefined
    taxa[11] = taxa[1500] = 0                    # NONE: skipped silently
    want = mm.as_arrays(mm.merge(parents, [(keys, taxa)]))
    assert sorted(mm.refused(parents, keys, taxa)) == [-7, undefined, len(parents)]
    ix = fresh(parents, expected=8192)
    e = failing(ix.merge_records, keys, taxa)
    assert e.code == E_INVALID and "3 records name a taxon" in str(e) and "(smallest: -7)" in str(e)
    assert mm.same(ix.export(), want)
    for bad in (len(parents), undefined, 2**31 - 1):
        one = np.array([bad], np.int32)
        e = failing(ix.merge_records, keys[:1], one)
        assert e.code == E_INVALID and f"1 records name a taxon the destination's taxonomy does not define (smallest: {bad})" in str(e)
    ix.merge_records(keys[:1], np.zeros(1, np.int32))                    # NONE alone: nothing happens
    assert mm.same(ix.export(), want)
    # the counters were this call's only, and the index goes on working
    ix.merge_records(*world["small"])
    assert mm.same(ix.export(), mm.merge(parents, [want, world["small"]]))
    ix.finalize()
    assert ix.info().records == len(np.unique(np.concatenate([want[0], world["small"][0]])))


# ---- 7. merge_index --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["unfinalized", "finalized", "dense"])
def test_merge_index(world, orc, source):
    parents, taxa, lut = world["parents"], world["taxa"], None
    if source == "dense":                        # ids beyond 22 bits: the finalized source is renumbered, its taxa travel as the caller's
        old = world["parents"]
        lut = np.arange(len(old), dtype=np.int32) + 2**22
        lut[0], lut[1] = 0, 1                    # (ROOT stays 1; every other node moves beyond 2^22)
        parents = np.zeros(2**22 + len(old), np.int32)
        for t in taxgen.defined_taxa(old):
            parents[lut[t]] = lut[old[t]]
        taxa = lut[np.array(world["taxa"])].tolist()
        assert min(taxa) >= 2**22
    relabel = (lambda r: (r[0], lut[r[1]])) if lut is not None else (lambda r: r)
    src = built(world, list(PARTS[1]) + list(PARTS[2]), parents=parents, taxa=taxa)
    if source != "unfinalized":
        src.finalize()
    assert (src.info().dense_taxa > 0) == (source == "dense")
    before = src.export()
    dst = built(world, list(PARTS[0]) + list(PARTS[1]), parents=parents, taxa=taxa)      # overlaps the source in PARTS[1]
    dst.merge_index(src)
    whole = relabel(world["whole"])
    assert mm.same(dst.export(), whole) and dst.info().records == len(whole[0]) and dst.info().duplicate_keys == 0
    assert mm.same(src.export(), before)
    dst.merge_index(src)                         # idempotent
    assert mm.same(dst.export(), whole)
    # the merged index in use: reads classified as by an index built from the whole
    dst.finalize()
    ref = built(world, range(20), parents=parents, taxa=taxa)
    ref.finalize()
    rng = np.random.default_rng(11)
    reads = [world["seqs"][i][a:a + 150] for i in (1, 8, 15, 19) for a in rng.integers(0, max(1, len(world["seqs"][i]) - 150), 8)]
    bases, offsets = synth.pack(reads)
    got = dst.stream().classify_batch(bases, offsets, thresholds=(0.0, 0.2), with_hits=False)
    want = ref.stream().classify_batch(bases, offsets, thresholds=(0.0, 0.2), with_hits=False)
    for key in ("taxon", "classified", "num_distinct", "total_kmers"):
        assert np.array_equal(got[key], want[key]), key
    assert got["classified"].any()


def test_merge_index_translates_and_refuses(world):
    """the remap and the check apply to a resident source as to arrays"""
    parents = world["parents"]
    src = fresh(parents, expected=8192)
    src.merge_records(*world["small"])
    records = src.export()
    gone = int(np.unique(records[1])[-1])
    remap = np.arange(len(parents), dtype=np.int32)
    remap[gone] = 0
    dst = fresh(parents, expected=8192)
    dst.set_merge_remap(remap)
    e = failing(dst.merge_index, src)
    n_bad = int((records[1] == gone).sum())
    assert e.code == E_INVALID and f"{n_bad} records name a taxon" in str(e) and f"(smallest: {gone})" in str(e)
    assert mm.same(dst.export(), mm.merge(parents, [records], remaps=[remap]))


# ---- 8. shards -------------------------------------------------------------------------------------------------------------------
def test_shards_take_their_share(world):
    exports = []
    for g in range(3):
        ix = fresh(world["parents"])
        ix.set_shard(g, 3)
        for part in world["parts"]:
            ix.merge_records(*part)
        exports.append(ix.export())
        assert ix.info().records == len(exports[-1][0]) > 0.25 * len(world["whole"][0])
    keys = np.concatenate([e[0] for e in exports])
    assert len(np.unique(keys)) == len(keys) == len(world["whole"][0])            # disjoint, and nothing lost
    assert mm.same((keys, np.concatenate([e[1] for e in exports])), world["whole"])


# ---- 9. states and arguments -----------------------------------------------------------------------------------------------------
def test_states_and_arguments(world):
    parents = world["parents"]
    keys, taxa = world["small"]
    done = fresh(parents, expected=8192)
    done.merge_records(keys, taxa)
    done.finalize()
    open_ix = fresh(parents, expected=8192)
    assert failing(done.merge_records, keys, taxa).code == E_STATE
    assert failing(done.merge_index, open_ix).code == E_STATE
    bare = fresh(parents, expected=8192, taxonomy=False)
    assert failing(bare.merge_records, keys, taxa).code == E_STATE
    assert failing(bare.merge_index, done).code == E_STATE
    wide = fresh(parents, expected=1024, k=50, m=40)
    import slacken_amd
    lib = slacken_amd.lib()
    one_key, one_taxon = np.zeros(1, np.int64), np.ones(1, np.int32)
    assert lib.slk_index_merge_records(wide.h, one_key.ctypes.data, one_taxon.ctypes.data, 1) == E_UNSUPPORTED
    assert failing(wide.merge_index, done).code == E_UNSUPPORTED          # several id columns in the destination
    assert failing(open_ix.merge_index, wide).code == E_UNSUPPORTED       # ... and in the source
    assert failing(open_ix.merge_index, open_ix).code == E_INVALID
    other_spaces = fresh(parents, expected=8192, spaces=9)
    assert failing(open_ix.merge_index, other_spaces).code == E_INVALID
    assert "splitters differ" in str(failing(other_spaces.merge_index, done))
    # n == 0
    open_ix.merge_records(np.zeros(0, np.int64), np.zeros(0, np.int32))
    open_ix.merge_records_device(None, None, 0)
    empty = fresh(parents, expected=8192)
    open_ix.merge_index(empty)
    assert open_ix.info().records == 0 and len(open_ix.export()[0]) == 0
    # a finalized source into an open destination is the use
    open_ix.merge_index(done)
    assert mm.same(open_ix.export(), world["small_model"])
