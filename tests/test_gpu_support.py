"""Sample support on the GPU (slk_support_*, slacken_amd/csrc/support.hip) through capi.Support against support_model.py, by exact
equality: reads with random sequence, short reads, N's and lower case at three depth filters, one hot taxon (the wave and LDS levels),
more taxa than a block's LDS map (the overflow route), chunk seams, repetition, any batching and order, a handle without the
bitmap, refusals and the cap protocol, a dynamic library, renumbered ids."""
import ctypes as C

import numpy as np
import pytest

import coverage_model as cm
import hostmodel
import support_model as sm
import synth
import taxgen
from test_host_classify2_gpu import write_ranked_taxonomy

pytestmark = pytest.mark.gpu
SEAM = 512                      # BUILD_CHUNK_WINDOWS: a sequence's chunk c starts with window 512 c
LDS_SLOTS = 1024                # SP_SLOTS of support.hip
GENUS, SPECIES = 7, 8


def dna(n, rng):
    return synth.random_dna(n, rng).tobytes()


class Genomes:
    def __init__(self, genomes):
        self.genomes = genomes


def sample_reads(genomes, n, rng, **kw):
    """n reads of 60..300 bases, synth.make_reads' mix: random reads, reads shorter than k, single N's, N runs, lower case"""
    lib = Genomes(genomes)
    return [synth.make_reads(lib, 1, rng, length=int(rng.integers(60, 301)), **kw)[0].tobytes() for _ in range(n)]


def make_index(p_args, keys, taxa, parents, expected=None):
    import slacken_amd
    k, m, s = p_args
    ix = slacken_amd.Index(k=k, m=m, spaces=s, expected_records=expected or len(keys), max_taxon=len(parents) - 1, device=0)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    return ix


def build_world(orc, tmp, k, m, s, seed, dense=False, grown=False):
    """12 genomes of 20 kbp with shared stretches under species of a ranked taxonomy (so that the LCAs lie at several depths), an
    index of them, 2 000 reads and the model's hits for them"""
    rng = np.random.default_rng(seed)
    p = orc.params(k=k, m=m, spaces=s)
    if grown:    # 4 taxon bits, so that the table starts small and has to double on the way; depth = steps to the root
        parents = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 4, 5, 6, 7], np.int32)
        species = list(range(8, 16))
        true_depth = lambda t: len(taxgen.path_to_root(parents, t)) - 1          # noqa: E731
        genus_depth, species_depth = 2, 3
    else:
        parents = taxgen.taxonomy(8 * 6, rng)
        tax = write_ranked_taxonomy(str(tmp / f"tax_{k}_{m}_{s}_{int(dense)}"), parents)
        ls = (len(parents) - 2) // taxgen.N_RANKS
        species = list(range(7 * ls + 2, 8 * ls + 2))
        true_depth = lambda t: hostmodel.depth(tax, t)                            # noqa: E731
        genus_depth, species_depth = GENUS, SPECIES
    genomes = [synth.random_dna(20000, rng) for _ in range(12)]
    for g in range(1, len(genomes)):
        a = int(rng.integers(0, 20000 - 3000))
        genomes[g][a:a + 3000] = genomes[int(rng.integers(0, g))][a:a + 3000]
    node = [species[g % len(species)] for g in range(len(genomes))]
    reads = sample_reads(genomes, 2000, rng)
    depth_of, ids = true_depth, range(len(parents))
    if dense:    # ids that need the dense renumbering
        parents, remap = taxgen.sparse_relabel(parents, (1 << 22) + 5000, rng)
        node = [remap[t] for t in node]
        inverse = {new: old for old, new in remap.items()}
        depth_of, ids = (lambda t: true_depth(inverse[t]) if t in inverse else -1), inverse.keys()      # noqa: E731
    bases, offsets = synth.pack(genomes)
    keys, taxa = orc.build_records(p, parents, bases, offsets, node)
    ix = make_index((k, m, s), keys, taxa, parents, expected=1000 if grown else None)
    depths = np.full(len(parents), -1, np.int32)
    for t in ids:
        depths[t] = depth_of(t)
    oidx = orc.Index(1, keys, taxa)
    model = sm.support(orc, p, oidx, depth_of, reads)
    return dict(orc=orc, p=p, k=k, ix=ix, st=ix.stream(), depths=depths, reads=reads, model=model, oidx=oidx, depth_of=depth_of, parents=parents,
                keys=keys, taxa=taxa, genus_depth=genus_depth, species_depth=species_depth, genomes=genomes, node=node)


@pytest.fixture(scope="module", params=[(35, 31, 7, "plain"), (21, 11, 0, "plain"), (35, 32, 7, "plain"), (35, 31, 7, "dense"), (35, 31, 7, "grown"),
                                        (35, 15, 0, "plain")],
                ids=["k35m31s7", "k21m11s0", "k35m32s7", "dense-ids", "grown-table", "k35m15-two-waves"])
def world(request, orc, tmp_path_factory):
    k, m, s, kind = request.param
    return build_world(orc, tmp_path_factory.mktemp("sup"), k, m, s, seed=200 + m + len(kind), dense=kind == "dense", grown=kind == "grown")


@pytest.fixture(scope="module")
def base(orc, tmp_path_factory):
    return build_world(orc, tmp_path_factory.mktemp("supb"), 35, 31, 7, seed=11)


def rows_of(sup):
    t, k, m, d = sup.result()
    assert t.dtype == np.int32 and k.dtype == np.uint64 and m.dtype == np.uint64 and d.dtype == np.uint64
    return list(zip(t.tolist(), k.tolist(), m.tolist(), d.tolist()))


def run(W, reads, min_depth, want_distinct=True, per_call=None, ix=None, st=None, depths=None):
    """(rows, totals) of the reads added per_call at a time (None: all at once) to a fresh handle"""
    import slacken_amd
    sup = slacken_amd.Support(ix or W["ix"], W["depths"] if depths is None else depths, min_depth=min_depth, want_distinct=want_distinct,
                              stream=st or W["st"])
    per_call = max(1, len(reads)) if per_call is None else per_call
    for a in range(0, len(reads), per_call):
        sup.add(*cm.pack(reads[a:a + per_call]))
    got = rows_of(sup), sup.totals()
    sup.close()
    return got


def test_matches_the_model_and_is_not_vacuous(world, request):
    W, model = world, world["model"]
    if "grown" in request.node.callspec.id:
        assert W["ix"].info().grown >= 1
    if "dense" in request.node.callspec.id:
        assert W["ix"].info().dense_taxa > 0 and len(W["parents"]) > (1 << 22)      # the rows carry the caller's ids all the same
    for min_depth in (0, W["genus_depth"], W["species_depth"]):
        assert run(W, W["reads"], min_depth) == (model.rows(min_depth), model.totals(min_depth))
    sequences, supermers, matched, kept = model.totals(W["species_depth"])
    assert matched > kept > 0 and supermers > matched and sequences == 2000
    assert len(model.rows(0)) > len(model.rows(W["genus_depth"])) >= len(model.rows(W["species_depth"])) > 1   # LCAs at several depths
    assert any(k > m > d for _, k, m, d in model.rows(0))
    assert any(len(r) < W["k"] for r in W["reads"]) and any(b"N" in r for r in W["reads"]) and any(r != r.upper() for r in W["reads"])


def test_one_hot_taxon(orc):
    """every read from one genome that is alone in the index: one row, summed by the wave and in LDS"""
    rng = np.random.default_rng(5)
    p = orc.params()
    parents = np.array([0, 0, 1, 2], np.int32)
    genome = synth.random_dna(20000, rng)
    keys, taxa = orc.build_records(p, parents, *synth.pack([genome]), [3])
    ix = make_index((35, 31, 7), keys, taxa, parents)
    reads = sample_reads([genome], 2000, rng, frac_random=0.0, short=0.0)
    depths = np.array([-1, 0, 1, 2], np.int32)
    model = sm.support(orc, p, orc.Index(1, keys, taxa), lambda t: int(depths[t]), reads)
    W = dict(ix=ix, st=ix.stream(), depths=depths)
    rows, totals = run(W, reads, 2)
    assert (rows, totals) == (model.rows(2), model.totals(2)) and len(rows) == 1 and rows[0][0] == 3
    assert rows[0][1] > rows[0][2] > rows[0][3] > 1000 and totals[3] > 64 * 256      # more hits than a block has lanes
    assert run(W, reads, 3) == ([], model.totals(3)) and model.totals(3)[3] == 0


def test_more_taxa_than_a_blocks_lds_map(orc):
    """every sequence is a taxon of its own and its own read: most hits find no LDS slot and go to the device arrays themselves"""
    n = max(20000, 4 * LDS_SLOTS)
    rng = np.random.default_rng(6)
    p = orc.params()
    parents = np.concatenate([[0, 0], np.ones(n, np.int32)]).astype(np.int32)
    seqs = [dna(100, rng) for _ in range(n)]
    bases, offsets = cm.pack(seqs)
    keys, taxa = orc.build_records(p, parents, bases, offsets, np.arange(2, n + 2, dtype=np.int32))
    depths = np.ones(n + 2, np.int32)
    depths[0], depths[1] = -1, 0
    model = sm.support(orc, p, orc.Index(1, keys, taxa), lambda t: int(depths[t]), seqs)
    want = model.rows(1)
    assert len(want) == n and [t for t, _, _, _ in want] == list(range(2, n + 2))          # the model gives that many rows
    ix = make_index((35, 31, 7), keys, taxa, parents)
    W = dict(ix=ix, st=ix.stream(), depths=depths)
    assert run(W, seqs, 1) == (want, model.totals(1))


def seam_reads(orc, p, k, rng):
    for attempt in range(50):
        plain = [dna(n, rng) for n in [*range(k + 510, k + 515), *range(k + 1022, k + 1027), 5000]]
        wm = cm.window_minimizers(orc, p, plain[-1])
        if wm[SEAM - 1] == wm[SEAM] and wm[2 * SEAM - 1] != wm[2 * SEAM]:      # one seam cuts a super-mer, another does not
            break
    else:
        raise AssertionError("no super-mer straddles a chunk seam")
    repeats = [b"A" * 3000, b"AC" * 1500]
    with_n = []
    for at in (SEAM - 2, SEAM - 1, SEAM, SEAM + 1, SEAM + 2, SEAM + k - 2, SEAM + k - 1):   # around the first seam and its priming window
        q = bytearray(plain[-1])
        q[at] = ord("N")
        with_n.append(bytes(q))
    q = bytearray(plain[-1])                                                   # the valid segment before the seam is shorter than k
    q[SEAM - 10] = ord("N")
    with_n.append(bytes(q))
    q = bytearray(plain[-1])                                                   # ... and so is the one behind it
    q[SEAM + 5] = ord("N")
    with_n.append(bytes(q))
    return plain, repeats, with_n


def test_seams(orc):
    k = 35
    rng = np.random.default_rng(8)
    p = orc.params()
    plain, repeats, with_n = seam_reads(orc, p, k, rng)
    parents = np.array([0, 0, 1, 2, 2, 2], np.int32)
    indexed = plain + repeats
    keys, taxa = orc.build_records(p, parents, *cm.pack(indexed), [3 + i % 3 for i in range(len(indexed))])
    ix = make_index((35, 31, 7), keys, taxa, parents)
    depths = np.array([-1, 0, 1, 2, 2, 2], np.int32)
    oidx = orc.Index(1, keys, taxa)
    W = dict(ix=ix, st=ix.stream(), depths=depths)
    reads = plain + repeats + with_n
    for r in reads:                                                            # each read alone ...
        model = sm.support(orc, p, oidx, lambda t: int(depths[t]), [r])
        assert run(W, [r], 0) == (model.rows(0), model.totals(0)) and model.rows(0)
    model = sm.support(orc, p, oidx, lambda t: int(depths[t]), reads)          # ... and all together
    assert run(W, reads, 0) == (model.rows(0), model.totals(0))
    assert run(W, reads, 2) == (model.rows(2), model.totals(2))
    # the homopolymer is one super-mer over six chunks: one minimizer, all its k-mers
    homo = sm.support(orc, p, oidx, lambda t: int(depths[t]), [repeats[0]])
    assert [(km, mn, d) for _, km, mn, d in homo.rows(0)] == [(3000 - k + 1, 1, 1)]


def test_repetition_batching_and_prefixes(base):
    import slacken_amd
    W, model = base, base["model"]
    reads, sd = W["reads"], W["species_depth"]
    want = model.rows(sd)
    twice, _ = run(W, reads + reads, sd)
    assert twice == [(t, 2 * k, 2 * m, d) for t, k, m, d in want]                # distinct is remembered, the sums double
    rng = np.random.default_rng(3)
    shuffled = [reads[i] for i in rng.permutation(len(reads))]
    for per_call in (None, (len(reads) + 1) // 2, (len(reads) + 6) // 7):        # 1, 2 and 7 calls
        assert run(W, shuffled, sd, per_call=per_call) == (want, model.totals(sd))
    assert run(W, reads[::-1], sd, per_call=1)[0] == want
    # result() between adds is the model's prefix
    sup = slacken_amd.Support(W["ix"], W["depths"], min_depth=sd, stream=W["st"])
    prefix = sm.Support(W["orc"], W["p"], W["oidx"], W["depth_of"])
    assert rows_of(sup) == [] and sup.totals() == (0, 0, 0, 0)
    for a in range(0, len(reads), 700):
        sup.add(*cm.pack(reads[a:a + 700]))
        prefix.add_all(reads[a:a + 700])
        assert rows_of(sup) == prefix.rows(sd) and sup.totals() == prefix.totals(sd)
        assert rows_of(sup) == prefix.rows(sd)                                   # (asking twice changes nothing)
    sup.close()


def test_without_distinct(base):
    import slacken_amd
    import torch
    W, model = base, base["model"]
    sd = W["species_depth"]
    rows, totals = run(W, W["reads"], sd, want_distinct=False)
    assert rows == model.rows(sd, want_distinct=False) and totals == model.totals(sd) and all(d == 0 for _, _, _, d in rows) and rows
    # no bitmap: a table large enough for its bitmap (cells / 8 bytes) to show in the device's free memory
    n = 280_000_000
    big = slacken_amd.Index(expected_records=n, max_taxon=len(W["parents"]) - 1, device=0)
    big.set_taxonomy(W["parents"])
    big.finalize()
    bitmap_bytes = big.info().buckets * big.info().bucket_cells // 8
    assert bitmap_bytes >= 32 << 20

    def drop(want_distinct):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(0)[0]
        sup = slacken_amd.Support(big, W["depths"], min_depth=sd, want_distinct=want_distinct)
        used = before - torch.cuda.mem_get_info(0)[0]
        sup.close()
        return used

    without, with_bitmap = drop(False), drop(True)
    assert without < bitmap_bytes <= with_bitmap and with_bitmap - without >= bitmap_bytes // 2
    big.close()


def test_refusals_and_protocol(base, orc):
    import slacken_amd
    from slacken_amd import capi
    W, model = base, base["model"]
    L = capi.lib()
    parents, sd = W["parents"], W["species_depth"]

    def code_of(fn):
        with pytest.raises(slacken_amd.SlackenError) as e:
            fn()
        return e.value.code

    raw = slacken_amd.Index(expected_records=1000, max_taxon=len(parents) - 1, device=0)
    raw.append(W["keys"][:100], W["taxa"][:100])
    assert code_of(lambda: slacken_amd.Support(raw, W["depths"])) == capi.E_STATE                 # not finalized
    raw.close()
    wide = slacken_amd.Index(k=45, m=40, spaces=0, expected_records=1000, max_taxon=len(parents) - 1, device=0)
    wide.finalize()
    assert code_of(lambda: slacken_amd.Support(wide, W["depths"])) == capi.E_UNSUPPORTED          # two id columns
    wide.close()
    shard = slacken_amd.Index(expected_records=1000, max_taxon=len(parents) - 1, device=0)
    shard.set_shard(1, 2)
    shard.append(W["keys"][:100], W["taxa"][:100])
    shard.finalize()
    assert code_of(lambda: slacken_amd.Support(shard, W["depths"])) == capi.E_UNSUPPORTED         # a shard of a sharded library
    shard.close()
    window = slacken_amd.Index(k=45, m=16, spaces=0, expected_records=1000, max_taxon=len(parents) - 1, device=0)
    window.finalize()
    assert code_of(lambda: slacken_amd.Support(window, W["depths"])) == capi.E_UNSUPPORTED        # a window of 30 m-mers
    window.close()
    assert code_of(lambda: slacken_amd.Support(W["ix"], W["depths"], min_depth=-1)) == capi.E_INVALID
    h = C.c_void_p()
    assert L.slk_support_create(None, None, 0, 0, 1, C.byref(h)) == capi.E_INVALID
    assert L.slk_support_create(W["ix"].h, None, 0, 0, 1, None) == capi.E_INVALID
    assert L.slk_support_create(W["ix"].h, None, 5, 0, 1, C.byref(h)) == capi.E_INVALID
    assert L.slk_support_add(None, W["st"].h, None, None, 0) == capi.E_INVALID
    assert L.slk_support_result(None, None, None, None, None, None, 0) == capi.E_INVALID
    assert L.slk_support_totals(None, None, None, None, None) == capi.E_INVALID
    sup = slacken_amd.Support(W["ix"], W["depths"], min_depth=sd, stream=W["st"])
    reads = W["reads"][:300]
    bases, offsets = cm.pack(reads)
    n = C.c_uint64(0)
    assert L.slk_support_add(sup.h, None, bases.ctypes.data, offsets.ctypes.data, 3) == capi.E_INVALID
    assert L.slk_support_add(sup.h, W["st"].h, bases.ctypes.data, None, 3) == capi.E_INVALID
    assert L.slk_support_add(sup.h, W["st"].h, None, offsets.ctypes.data, 3) == capi.E_INVALID
    assert L.slk_support_result(sup.h, None, None, None, None, None, 0) == capi.E_INVALID
    assert L.slk_support_result(sup.h, C.byref(n), None, None, None, None, 4) == capi.E_INVALID
    bad = offsets.copy()
    bad[1], bad[2] = bad[2], bad[1]
    assert code_of(lambda: sup.add(bases, bad)) == capi.E_INVALID                                   # counted nothing ...
    assert rows_of(sup) == [] and sup.totals() == (0, 0, 0, 0)
    sup.add(bases, offsets)                                                                         # ... and the handle still works
    want = sm.support(orc, W["p"], W["oidx"], W["depth_of"], reads)
    assert rows_of(sup) == want.rows(sd) and len(want.rows(sd)) > 1
    # cap 0 asks for the number; too small a capacity still gives it, with the first rows
    assert L.slk_support_result(sup.h, C.byref(n), None, None, None, None, 0) == 0 and n.value == len(want.rows(sd))
    t1 = np.zeros(1, np.int32)
    k1, m1, d1 = (np.zeros(1, np.uint64) for _ in range(3))
    n.value = 0
    assert L.slk_support_result(sup.h, C.byref(n), t1.ctypes.data, k1.ctypes.data, m1.ctypes.data, d1.ctypes.data, 1) == capi.E_CAPACITY
    assert n.value == len(want.rows(sd)) and (int(t1[0]), int(k1[0]), int(m1[0]), int(d1[0])) == want.rows(sd)[0]
    assert rows_of(sup) == want.rows(sd)                                                            # (not spent by that)
    sup.close()
    # no depths at all: every taxon has depth -1 and nothing passes
    assert run(W, reads, 0, depths=np.zeros(0, np.int32))[0] == []


def test_a_dynamic_library(base, orc):
    """an index built from genomes by slk_index_add_sequences, as classify2's second step builds it"""
    import slacken_amd
    W = base
    sel = [0, 3, 7]
    bases, offsets = synth.pack([W["genomes"][g] for g in sel])
    node = [W["node"][g] for g in sel]
    dyn = slacken_amd.Index(expected_records=100_000, max_taxon=len(W["parents"]) - 1, device=0)
    dyn.set_taxonomy(W["parents"])
    dyn.add_sequences(bases, offsets, node)
    dyn.finalize()
    keys, taxa = orc.build_records(W["p"], W["parents"], bases, offsets, node)
    model = sm.support(orc, W["p"], orc.Index(1, keys, taxa), W["depth_of"], W["reads"])
    sd = W["species_depth"]
    assert run(W, W["reads"], sd, ix=dyn, st=dyn.stream()) == (model.rows(sd), model.totals(sd)) and model.rows(sd)
    assert model.totals(sd)[2] < W["model"].totals(sd)[2]                                           # fewer genomes, fewer hits


@pytest.mark.parametrize("distinct", [1, 2, 3, 64])
def test_one_wave_of_few_taxa(orc, distinct):
    """64 reads of exactly k bases, every one its own indexed sequence: one wave of 64 one-window chunks whose super-mers all close
    at the end of the chunk, so one push brings the queue exactly 64 entries, and the 64 hits of the flush name 1, 2, 3 (lanes are
    left over after the two leader rounds) or 64 taxa.  The taxa are 63 and up: with 64 of them the rows straddle the border between
    two waves of the result kernel, and with 2 or 3 a wave of it has few holders."""
    k = 35
    rng = np.random.default_rng(70 + distinct)
    p = orc.params()
    parents = np.concatenate([[0, 0], np.ones(126, np.int32)]).astype(np.int32)
    reads = [dna(k, rng) for _ in range(64)]
    node = [63 + i % distinct for i in range(64)]
    keys, taxa = orc.build_records(p, parents, *cm.pack(reads), node)
    assert len(keys) == 64
    depths = np.ones(128, np.int32)
    depths[0], depths[1] = -1, 0
    model = sm.support(orc, p, orc.Index(1, keys, taxa), lambda t: int(depths[t]), reads)
    ix = make_index((35, 31, 7), keys, taxa, parents)
    rows, totals = run(dict(ix=ix, st=ix.stream(), depths=depths), reads, 1)
    assert (rows, totals) == (model.rows(1), model.totals(1))
    assert [t for t, _, _, _ in rows] == list(range(63, 63 + distinct)) and totals == (64, 64, 64, 64)


def test_one_lane_fills_the_queue_twice(orc):
    """one read of one chunk (k + 510 bases) with more super-mers than the queue's 128 entries, alone in its wave: the ring's index
    wraps, and the tail flush takes fewer than 64"""
    k = 35
    rng = np.random.default_rng(9)
    p = orc.params()
    parents = np.array([0, 0, 1, 2], np.int32)
    read = dna(k + 510, rng)
    keys, taxa = orc.build_records(p, parents, *cm.pack([read]), [3])
    depths = np.array([-1, 0, 1, 2], np.int32)
    model = sm.support(orc, p, orc.Index(1, keys, taxa), lambda t: int(depths[t]), [read])
    assert model.totals(0)[1] > 128
    ix = make_index((35, 31, 7), keys, taxa, parents)
    assert run(dict(ix=ix, st=ix.stream(), depths=depths), [read], 0) == (model.rows(0), model.totals(0))
