"""slk_pipe: batches in flight on the C ABI, and the compact read forms that are expanded on the device (readform.hip).  Small
batches are compared bit for bit with the CPU oracle; the large-R cases with Stream.classify_batch, which test_gpu_parity.py pins
to the oracle."""
import threading

import numpy as np
import pytest

import synth
import taxgen

pytestmark = pytest.mark.gpu

E_INVALID, E_CAPACITY, E_STATE = -1, -5, -6
THR = (0.0, 0.15)
ROWS = ("taxon", "classified", "num_distinct", "total_kmers")
HIT_MODES = [(0, False), (1, False), (2, False), (2, True)]      # (hits, merged)


def make_world(orc, p, rng, n_genomes, genome_len, pad_records, ntax):
    import slacken_amd
    parents = taxgen.taxonomy(ntax, rng)
    lib = synth.Library(orc, p, parents, n_genomes=n_genomes, genome_len=genome_len, pad_records=pad_records)
    ix = slacken_amd.Index(k=p.k, m=p.m, spaces=p.spaces, expected_records=len(lib.keys), max_taxon=len(parents) - 1)
    ix.append(lib.keys, lib.taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    return dict(p=p, lib=lib, ix=ix, oix=orc.Index(1, lib.keys, lib.taxa), parents=parents, st=ix.stream())


@pytest.fixture(scope="module")
def world(orc):
    """the world of test_gpu_parity.py: 12 genomes of 20 kbp, the default splitter"""
    return make_world(orc, orc.params(), np.random.default_rng(2240), 12, 20000, 50000, 8 * 128)


@pytest.fixture(scope="module")
def small_k(orc):
    """k = 21, m = 12, spaces = 5: reads of 21 .. 60 bases have spans, so the offsets decide the results"""
    w = make_world(orc, orc.params(k=21, m=12, spaces=5), np.random.default_rng(77), 3, 3000, 0, 64)
    w["genome"] = np.concatenate(w["lib"].genomes)
    return w


def side(form, lenform, bases, offsets):
    """one side of a batch as Pipe.submit takes it"""
    from slacken_amd import capi
    d = {}
    if form == "ascii":
        d["bases"] = bases
    elif form == "dense":
        d["codes"], d["valid"] = capi.pack_bases(bases)
    else:
        d["codes"], d["exc_word"], d["exc_bits"] = capi.pack_bases_sparse(bases)
    lens = np.diff(offsets.astype(np.int64))
    if lenform == "offsets":
        d["offsets"] = offsets
    elif lenform == "lengths":
        d["lengths"] = lens.astype(np.uint32)
    else:
        assert len(lens) and (lens == lens[0]).all()
        d["uniform_len"] = int(lens[0])
    return d


def reference(st, bases, offsets, mb=None, mo=None, thresholds=THR, min_hit_groups=2):
    """what the synchronous entry gives: the rows and the un-merged lists, and the lists merged"""
    from test_gpu_parity import merged_lists
    ref = st.classify_batch(bases, offsets, mb, mo, min_hit_groups=min_hit_groups, thresholds=thresholds)
    ref["merged_offsets"], ref["merged_hits"] = merged_lists(ref["hit_offsets"], ref["hits"])
    return ref


def same(got, ref, hits, merged, what=""):
    for key in ROWS:
        assert np.array_equal(got[key], ref[key]), (what, key)
    if hits == 1 or (hits == 2 and not merged):
        assert np.array_equal(got["num_hits"], ref["num_hits"]), (what, "num_hits")
    if hits == 2:
        off, lists = (ref["merged_offsets"], ref["merged_hits"]) if merged else (ref["hit_offsets"], ref["hits"])
        assert np.array_equal(got["hit_offsets"], off), (what, "hit_offsets")
        assert np.array_equal(got["hits"]["taxon"], lists["taxon"]) and np.array_equal(got["hits"]["count"], lists["count"]), (what, "hits")
    else:
        assert "hits" not in got


def run_modes(pipe, reads, mates, R, ref, what, thresholds=THR, modes=HIT_MODES):
    """the batch through the pipe once per hit mode, all in flight together where the depth allows"""
    tickets = []
    for hits, merged in modes:
        pipe.set_merged_hits(merged)
        tickets.append(pipe.submit(reads, mates, R=R, thresholds=thresholds, hits=hits))
    pipe.set_merged_hits(False)
    for (hits, merged), t in zip(modes, tickets):
        same(pipe.collect(t), ref, hits, merged, (what, hits, merged))
    assert pipe.pending() == 0


# ---- parity ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def parity(orc, world):
    """~3 000 reads of every kind, and 3 000 of one length for uniform_len; each with mates; the oracle's rows once"""
    rng = np.random.default_rng(1914)
    kinds = dict(n_single=0.2, n_run=0.1, lowercase=0.1)
    sets = dict(varied=(synth.make_reads(world["lib"], 3000, rng, vary_length=True, short=0.05, **kinds),
                        synth.make_reads(world["lib"], 3000, rng, vary_length=True, short=0.05, **kinds)),
                fixed=(synth.make_reads(world["lib"], 3000, rng, short=0.0, **kinds),
                       synth.make_reads(world["lib"], 3000, rng, length=100, short=0.0, **kinds)))
    out = {}
    for name, (r, m) in sets.items():
        b, o = synth.pack(r)
        mb, mo = synth.pack(m)
        for paired in (False, True):
            args = (b, o, mb, mo) if paired else (b, o)
            ref = reference(world["st"], *args)
            want = orc.classify_batch(world["p"], world["oix"], world["parents"], *args, min_hit_groups=2, thresholds=THR)
            for key in ROWS + ("num_hits",):
                assert np.array_equal(ref[key], want[key]), key
            out[name, paired] = (args, ref)
    return out


@pytest.fixture(scope="module")
def pipe4(world):
    import slacken_amd
    p = slacken_amd.Pipe(world["ix"], 4)
    yield p
    p.close()


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("lenform", ["offsets", "lengths", "uniform_len"])
@pytest.mark.parametrize("form", ["ascii", "dense", "sparse"])
def test_parity(parity, pipe4, form, lenform, paired):
    args, ref = parity["fixed" if lenform == "uniform_len" else "varied", paired]
    reads = side(form, lenform, args[0], args[1])
    mates = side(form, lenform, args[2], args[3]) if paired else None
    assert ref["classified"][0].mean() > 0.3
    run_modes(pipe4, reads, mates, len(args[1]) - 1, ref, (form, lenform, paired))


def test_parity_mixed_sides(parity, pipe4):
    """the two sides of a batch choose their forms independently"""
    args, ref = parity["fixed", True]
    run_modes(pipe4, side("sparse", "uniform_len", args[0], args[1]), side("dense", "lengths", args[2], args[3]), 3000, ref, "mixed")
    args, ref = parity["varied", True]
    run_modes(pipe4, side("dense", "offsets", args[0], args[1]), side("sparse", "lengths", args[2], args[3]), 3000, ref, "mixed")


def test_parity_wide_splitter(orc):
    """minimizers of 63 nt (two id columns, the staged kernels) through the pipe, against the oracle"""
    import slacken_amd
    from test_gpu_wide import build_world
    k, m, spaces = 70, 63, 10
    rng = np.random.default_rng(k * 1000 + m)
    p, W, parents, genomes, keys, tx = build_world(orc, k, m, spaces, True, rng)
    ix = slacken_amd.Index(k=k, m=m, spaces=spaces, canonical=True, expected_records=len(tx), max_taxon=len(parents) - 1)
    ix.append(keys, tx)
    ix.set_taxonomy(parents)
    ix.finalize()
    oix = orc.Index(W, keys, tx)

    class L:
        pass
    L.genomes = genomes
    reads = synth.make_reads(L, 600, rng, length=160, vary_length=True, n_single=0.1, n_run=0.05)
    mates = synth.make_reads(L, 600, rng, length=120, vary_length=True, short=0.1)
    (b, o), (mb, mo) = synth.pack(reads), synth.pack(mates)
    st, pipe = ix.stream(), slacken_amd.Pipe(ix, 4)
    for args in ((b, o), (b, o, mb, mo)):
        want = orc.classify_batch(p, oix, parents, *args, min_hit_groups=2, thresholds=THR)
        ref = reference(st, *args)
        for key in ROWS + ("num_hits",):
            assert np.array_equal(ref[key], want[key]), key
        run_modes(pipe, side("sparse", "lengths", b, o), side("dense", "offsets", mb, mo) if len(args) == 4 else None, 600, ref, "wide")
    assert want["classified"][0].mean() > 0.05
    pipe.close()


# ---- expansion edges: lengths -> offsets ----------------------------------------------------------------------------------------

def draw(w, R, rng, residue=None):
    """R reads of 0 .. 60 bases cut from the world's genomes, a few N among them; zero-length reads at the first position, at the
    last and in a run; residue: the side's total modulo 16 (by one read's length)"""
    g = w["genome"]
    lens = rng.integers(0, 61, R).astype(np.int64)
    if R >= 1:
        lens[0] = 0
        lens[-1] = 0
    if R >= 40:
        lens[10:20] = 0
    if residue is not None and R >= 3:
        lens[R // 2] = 20 + (residue - (lens.sum() - lens[R // 2]) - 20) % 16
    offsets = np.zeros(R + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    total = int(offsets[-1])
    start = rng.integers(0, len(g) - 80, R)
    bases = g[np.repeat(start - offsets[:-1].astype(np.int64), lens) + np.arange(total)].copy()
    bases[rng.random(total) < 0.003] = ord("N")
    assert residue is None or R < 3 or total % 16 == residue
    return bases, offsets


TILE = 1024           # engine.h: READFORM_TILE, the lengths of one block of the count and the scatter pass
SCAN_ROUND = 256      # readform.hip: RF_T, the tiles the one-block scan takes per round -- and the threads of every block
EDGE_R = [0, 1, 2, 63, 64, 65, SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1, TILE - 1, TILE, TILE + 1, 70001]
LARGE_R = [TILE * SCAN_ROUND - 1, TILE * SCAN_ROUND, TILE * SCAN_ROUND + 1]     # the last: the first R with a second round of the scan


@pytest.fixture(scope="module")
def small_pipe(small_k):
    import slacken_amd
    p = slacken_amd.Pipe(small_k["ix"], 4)
    yield p
    p.close()


@pytest.mark.parametrize("R", EDGE_R)
def test_lengths_to_offsets_edges(small_k, small_pipe, R):
    rng = np.random.default_rng(R)
    st = small_k["st"]
    for residue in (0, 5):
        b, o = draw(small_k, R, rng, residue)
        mb, mo = draw(small_k, R, rng, 11 - residue)
        ref = reference(st, b, o, thresholds=(0.0,))
        if 3 <= R <= TILE + 1:
            assert (ref["num_hits"] > 0).any() or R < 60
        run_modes(small_pipe, side("sparse", "lengths", b, o), None, R, ref, ("single", R, residue), thresholds=(0.0,))
        ref = reference(st, b, o, mb, mo, thresholds=(0.0,))
        run_modes(small_pipe, side("ascii", "lengths", b, o), side("dense", "lengths", mb, mo), R, ref, ("paired", R, residue),
                  thresholds=(0.0,), modes=[(0, False), (2, False)])


@pytest.mark.parametrize("R", LARGE_R)
def test_lengths_to_offsets_second_scan_round(small_k, small_pipe, R):
    rng = np.random.default_rng(R)
    b, o = draw(small_k, R, rng, 7)
    ref = small_k["st"].classify_batch(b, o, thresholds=(0.0,), with_hits=False, with_num_hits=True)
    assert (ref["num_hits"][-2000:] > 0).any()        # reads behind the last tile border have spans: their offsets matter
    t = small_pipe.submit(side("sparse", "lengths", b, o), hits=1, thresholds=(0.0,))
    same(small_pipe.collect(t), ref, 1, False, R)


def test_uniform_len_edges(small_k, small_pipe):
    rng = np.random.default_rng(31)
    g = small_k["genome"]
    for R, L in ((1, 33), (64, 32), (65, 47), (257, 60), (70001, 37)):
        start = rng.integers(0, len(g) - 80, R)
        b = g[(start[:, None] + np.arange(L)[None, :]).ravel()].copy()
        b[rng.random(b.size) < 0.003] = ord("N")
        o = (np.arange(R + 1) * L).astype(np.uint64)
        ref = reference(small_k["st"], b, o, thresholds=(0.0,))
        run_modes(small_pipe, side("sparse", "uniform_len", b, o), None, R, ref, ("uniform", R, L), thresholds=(0.0,))


# ---- validity edges -------------------------------------------------------------------------------------------------------------

def test_sparse_validity_edges(world, pipe4):
    from slacken_amd import capi
    rng = np.random.default_rng(8)
    lens = [40, 50, 150, 150, 23, 150, 150, 150, 99]
    reads = [r.copy() for r in synth.make_reads(world["lib"], len(lens), rng, length=150, frac_random=0, n_single=0, n_run=0, lowercase=0,
                                                short=0)]
    reads = [r[:n] for r, n in zip(reads, lens)]
    reads[5][:] = ord("N")                         # a read that is invalid throughout
    b, o = synth.pack(reads)
    total = int(o[-1])
    assert total % 16 != 0
    b[0] = ord("N")                                # word 0
    b[total - 1] = ord("N")                        # the last, partial word
    b[100] = b[117] = ord("n")                     # adjacent words (6 and 7)
    b[39] = b[41] = ord("-")                       # word 2 is shared by reads 0 and 1: one invalid base on either side of the border
    d = side("sparse", "lengths", b, o)
    words = (total + 15) // 16
    assert {0, 2, 6, 7, words - 1} <= set(d["exc_word"].tolist()) and d["exc_word"].size < words
    ref = reference(world["st"], b, o)
    assert (ref["num_hits"][[0, 1, 2]] > 0).all() and ref["num_distinct"][5] == 0 and not ref["classified"][0][5]
    run_modes(pipe4, d, None, len(lens), ref, "edges")
    # the bits of the last word past the side's last base are ignored
    d2 = dict(d)
    d2["exc_bits"] = d["exc_bits"].copy()
    d2["exc_bits"][-1] |= np.uint16((0xFFFF << (total % 16)) & 0xFFFF)
    run_modes(pipe4, d2, None, len(lens), ref, "garbage in the last word")
    # every word an exception
    b2 = b.copy()
    b2[::16] = ord("N")
    d = side("sparse", "offsets", b2, o)
    assert d["exc_word"].size == words
    run_modes(pipe4, d, None, len(lens), reference(world["st"], b2, o), "every word")
    # no exception: null pointers
    clean = [r for i, r in enumerate(synth.make_reads(world["lib"], 200, rng, n_single=0, n_run=0, lowercase=0.1, short=0.05))]
    b3, o3 = synth.pack(clean)
    codes, exc_word, _ = capi.pack_bases_sparse(b3)
    assert exc_word.size == 0
    run_modes(pipe4, dict(codes=codes, offsets=o3), None, len(clean), reference(world["st"], b3, o3), "no exception")


# ---- pipeline semantics ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three(world):
    """three different batches with their synchronous results"""
    rng = np.random.default_rng(333)
    out = []
    for n, paired in ((700, False), (1500, True), (90, False)):
        b, o = synth.pack(synth.make_reads(world["lib"], n, rng, vary_length=True, n_single=0.2, n_run=0.1))
        mb, mo = synth.pack(synth.make_reads(world["lib"], n, rng, length=100)) if paired else (None, None)
        out.append(dict(b=b, o=o, mb=mb, mo=mo, R=n, ref=reference(world["st"], b, o, mb, mo)))
    return out


def submit_batch(pipe, x, form="sparse", lenform="lengths", hits=2, thresholds=THR):
    return pipe.submit(side(form, lenform, x["b"], x["o"]), side(form, lenform, x["mb"], x["mo"]) if x["mb"] is not None else None,
                       R=x["R"], thresholds=thresholds, hits=hits)


def test_collect_in_any_order_and_full_pipe(world, three):
    import slacken_amd
    pipe = slacken_amd.Pipe(world["ix"], 3)
    tickets = [submit_batch(pipe, x) for x in three]
    assert len(set(tickets)) == 3 and pipe.pending() == 3
    with pytest.raises(slacken_amd.SlackenError) as e:                 # a fourth submit: refused at once, nothing changes
        submit_batch(pipe, three[0])
    assert e.value.code == E_STATE and pipe.pending() == 3
    for i in (2, 0, 1):
        same(pipe.collect(tickets[i]), three[i]["ref"], 2, False, i)
        with pytest.raises(slacken_amd.SlackenError) as e:             # collected: gone
            pipe.collect(tickets[i])
        assert e.value.code == E_STATE
    assert pipe.pending() == 0
    for unknown in (0, max(tickets) + 1, 1 << 40):
        with pytest.raises(slacken_amd.SlackenError) as e:
            pipe.collect(unknown)
        assert e.value.code == E_STATE
    pipe.close()


def test_small_hits_capacity_leaves_the_ticket(world, three):
    import slacken_amd
    pipe = slacken_amd.Pipe(world["ix"], 3)
    for merged in (False, True):
        pipe.set_merged_hits(merged)
        tickets = [submit_batch(pipe, x) for x in three]
        with pytest.raises(slacken_amd.SlackenError) as e:
            pipe.collect(tickets[1], hits_capacity=3)
        ref = three[1]["ref"]
        assert e.value.code == E_CAPACITY and pipe.pending() == 3
        assert np.array_equal(e.value.hit_offsets, ref["merged_offsets"] if merged else ref["hit_offsets"])      # filled all the same
        need = int(e.value.hit_offsets[-1])
        with pytest.raises(slacken_amd.SlackenError) as e:             # ... and again
            pipe.collect(tickets[1], hits_capacity=need - 1)
        assert e.value.code == E_CAPACITY and pipe.pending() == 3
        same(pipe.collect(tickets[1], hits_capacity=need), ref, 2, merged)               # exactly enough
        same(pipe.collect(tickets[0]), three[0]["ref"], 2, merged)
        same(pipe.collect(tickets[2]), three[2]["ref"], 2, merged)
    pipe.close()


def test_pageable_input_is_free_when_submit_returns(world, three):
    import slacken_amd
    pipe = slacken_amd.Pipe(world["ix"], 3)
    for form, lenform in (("ascii", "offsets"), ("dense", "lengths"), ("sparse", "lengths")):
        tickets = []
        for x in three:
            reads = side(form, lenform, x["b"].copy(), x["o"].copy())
            mates = side(form, lenform, x["mb"].copy(), x["mo"].copy()) if x["mb"] is not None else None
            tickets.append(pipe.submit(reads, mates, R=x["R"], thresholds=THR, hits=2))
            for d in (reads, mates or {}):
                for a in d.values():
                    if isinstance(a, np.ndarray):
                        a.view(np.uint8)[:] = 0xA5
        for t, x in zip(tickets, three):
            same(pipe.collect(t), x["ref"], 2, False, (form, lenform))
    pipe.close()


def test_pinned_input(world, three):
    """memory of slk_host_alloc is read by DMA: left alone until the collect, the results are the same"""
    import slacken_amd
    from slacken_amd import capi
    pipe = slacken_amd.Pipe(world["ix"], 2)
    x = three[1]

    def pin(a):
        out = capi.pinned_array(a.shape, a.dtype)
        out[...] = a
        return out
    reads = {k: pin(v) if isinstance(v, np.ndarray) else v for k, v in side("sparse", "lengths", x["b"], x["o"]).items()}
    mates = {k: pin(v) if isinstance(v, np.ndarray) else v for k, v in side("dense", "offsets", x["mb"], x["mo"]).items()}
    t1 = pipe.submit(reads, mates, thresholds=THR, hits=2)
    t2 = pipe.submit(reads, mates, thresholds=THR, hits=0)
    same(pipe.collect(t2), x["ref"], 0, False)
    same(pipe.collect(t1), x["ref"], 2, False)
    pipe.close()


def test_buffers_regrow_while_neighbours_are_in_flight(world):
    import slacken_amd
    rng = np.random.default_rng(12)
    pipe = slacken_amd.Pipe(world["ix"], 3)
    st = world["st"]
    sizes = [300, 3000, 50, 1500, 4000, 10, 2500, 700, 5000, 1, 3500, 6000]
    flight = []
    for i, n in enumerate(sizes):
        paired, thr, hits = i % 2 == 1, THR[:1 + i % 2] if i % 3 else (0.0, 0.05, 0.5), (2, 0, 1)[i % 3]
        b, o = synth.pack(synth.make_reads(world["lib"], n, rng, vary_length=True, n_single=0.2))
        mb, mo = synth.pack(synth.make_reads(world["lib"], n, rng, length=80)) if paired else (None, None)
        ref = reference(st, b, o, mb, mo, thresholds=thr)
        form, lenform = ("ascii", "dense", "sparse")[i % 3], ("lengths", "offsets")[i % 2]
        t = pipe.submit(side(form, lenform, b, o), side(form, lenform, mb, mo) if paired else None, thresholds=thr, hits=hits)
        flight.append((t, ref, hits, i))
        if len(flight) == 3:
            t, ref, hits, j = flight.pop(0)
            same(pipe.collect(t), ref, hits, False, j)
    for t, ref, hits, j in flight:
        same(pipe.collect(t), ref, hits, False, j)
    pipe.close()


def test_deferred_and_unbounded_batch_between_plain_ones(orc):
    """a batch whose fragments overflow the lane kernel's map (deferred) and the wave kernel's (the unbounded re-run at collect),
    built as test_gpu_parity.py's test_many_taxa_per_read_take_the_deferred_path builds it, between two plain batches"""
    import slacken_amd
    p = orc.params()
    rng = np.random.default_rng(99)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    plain = [synth.random_dna(150, rng) for _ in range(120)]
    big = [synth.random_dna(3000, rng), synth.random_dna(150, rng), synth.random_dna(6000, rng)] + plain[:50]
    kk = np.unique(np.concatenate([orc.minimizer_keys(p, b.tobytes()) for b in big + plain]))
    many = rng.choice(taxa, size=len(kk), replace=len(kk) > len(taxa)).astype(np.int32)
    ix = slacken_amd.Index(expected_records=len(kk), max_taxon=len(parents) - 1)
    ix.append(kk, many)
    ix.set_taxonomy(parents)
    ix.finalize()
    oix, st = orc.Index(1, kk, many), ix.stream()
    batches = []
    for reads in (plain[50:], big, plain[60:110]):
        b, o = synth.pack(reads)
        ref = reference(st, b, o, thresholds=(0.0, 0.1, 0.5))
        want = orc.classify_batch(p, oix, parents, b, o, min_hit_groups=2, thresholds=(0.0, 0.1, 0.5))
        for key in ROWS + ("num_hits",):
            assert np.array_equal(ref[key], want[key]), key
        batches.append((b, o, ref))
    assert batches[1][2]["num_distinct"][0] > 128 and batches[1][2]["num_distinct"][2] > 128
    assert (batches[0][2]["num_distinct"] > 12).all()
    pipe = slacken_amd.Pipe(ix, 3)
    for hits, merged in HIT_MODES:
        pipe.set_merged_hits(merged)
        tickets = [pipe.submit(side("sparse", "lengths", b, o), thresholds=(0.0, 0.1, 0.5), hits=hits) for b, o, _ in batches]
        for i in (1, 2, 0):
            same(pipe.collect(tickets[i]), batches[i][2], hits, merged, (i, hits, merged))
    pipe.close()


def test_two_pipes_from_two_threads(world, three):
    import slacken_amd
    errors = []

    def work(seed):
        try:
            pipe = slacken_amd.Pipe(world["ix"], 2)
            order = np.random.default_rng(seed).integers(0, 3, 8)
            flight = []
            for i in order:
                flight.append((submit_batch(pipe, three[i], hits=2 if seed else 0), i))
                if len(flight) == 2:
                    t, j = flight.pop(0)
                    same(pipe.collect(t), three[j]["ref"], 2 if seed else 0, False, (seed, j))
            for t, j in flight:
                same(pipe.collect(t), three[j]["ref"], 2 if seed else 0, False, (seed, j))
            pipe.close()
        except BaseException as e:      # noqa: B036 (handed to the main thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(s,)) for s in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]


def test_close_with_tickets_pending(world, three):
    import slacken_amd
    pipe = slacken_amd.Pipe(world["ix"], 3)
    for x in three:
        submit_batch(pipe, x)
    assert pipe.pending() == 3
    pipe.close()
    pipe = slacken_amd.Pipe(world["ix"], 1)
    same(pipe.collect(submit_batch(pipe, three[0])), three[0]["ref"], 2, False)
    pipe.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_submit_refusals(world, three):
    import slacken_amd
    from slacken_amd import capi
    pipe = slacken_amd.Pipe(world["ix"], 2)
    x = three[0]
    held = submit_batch(pipe, x)                   # one ticket in flight throughout: a refusal leaves it alone
    b, o, R = x["b"], x["o"], x["R"]
    lens = np.diff(o.astype(np.int64)).astype(np.uint32)
    codes, valid = capi.pack_bases(b)
    _, exc_word, exc_bits = capi.pack_bases_sparse(b)
    assert exc_word.size >= 3
    words = (b.size + 15) // 16
    swapped = exc_word.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    twice = exc_word.copy()
    twice[1] = twice[0]
    beyond = exc_word.copy()
    beyond[-1] = words
    bad = dict(
        lengths_and_uniform_len=dict(bases=b, lengths=lens, uniform_len=150),
        offsets_and_lengths=dict(bases=b, offsets=o, lengths=lens),
        no_length_form=dict(bases=b),
        bases_and_codes=dict(bases=b, codes=codes, valid=valid, offsets=o),
        neither_bases_nor_codes=dict(offsets=o),
        valid_with_exceptions=dict(codes=codes, valid=valid, exc_word=exc_word, exc_bits=exc_bits, offsets=o),
        ascii_with_validity=dict(bases=b, valid=valid, offsets=o),
        exceptions_without_bits=dict(codes=codes, exc_word=exc_word, offsets=o),
        exc_word_not_ascending=dict(codes=codes, exc_word=swapped, exc_bits=exc_bits, offsets=o),
        exc_word_repeated=dict(codes=codes, exc_word=twice, exc_bits=exc_bits, offsets=o),
        exc_word_out_of_range=dict(codes=codes, exc_word=beyond, exc_bits=exc_bits, offsets=o),
        offsets_decreasing=dict(bases=b, offsets=np.concatenate([o[:5], o[3:4], o[6:]])),
    )
    for name, d in bad.items():
        with pytest.raises(slacken_amd.SlackenError) as e:
            pipe.submit(d, R=R, thresholds=THR)
        assert e.value.code == E_INVALID, name
        assert pipe.pending() == 1, name
    # lengths that sum to 2^32 or more: refused from the numbers alone (nothing of that size is allocated or read)
    for d in (dict(bases=np.zeros(16, np.uint8), lengths=np.full(3, 0x60000000, np.uint32)),
              dict(codes=np.zeros(16, np.uint32), lengths=np.full(3, 0x60000000, np.uint32)),
              dict(bases=np.zeros(16, np.uint8), lengths=np.array([1, 0x80000000, 1], np.uint32)),
              dict(bases=np.zeros(16, np.uint8), uniform_len=0x60000000)):
        with pytest.raises(slacken_amd.SlackenError) as e:
            pipe.submit(d, R=3, thresholds=THR)
        assert e.value.code == E_INVALID and pipe.pending() == 1
    # mates with another R (slk_pipe_submit has one R for both sides: the binding compares the arrays)
    for mates in (dict(bases=b, offsets=o[:-1]), dict(bases=b, lengths=lens[:-1]), dict(codes=codes, valid=valid, lengths=np.append(lens, 5))):
        with pytest.raises(slacken_amd.SlackenError) as e:
            pipe.submit(dict(bases=b, offsets=o), mates, thresholds=THR)
        assert e.value.code == E_INVALID and pipe.pending() == 1
    with pytest.raises(slacken_amd.SlackenError) as e:                 # ... and a refusal of the mates' side by the library
        pipe.submit(dict(bases=b, offsets=o), dict(codes=codes, valid=valid, offsets=o, uniform_len=150), thresholds=THR)
    assert e.value.code == E_INVALID and pipe.pending() == 1
    # thresholds, hits
    for kw in (dict(thresholds=()), dict(thresholds=THR, hits=3)):
        with pytest.raises(slacken_amd.SlackenError) as e:
            pipe.submit(dict(bases=b, offsets=o), **kw)
        assert e.value.code == E_INVALID and pipe.pending() == 1
    same(pipe.collect(held), x["ref"], 2, False)
    pipe.close()
    for depth in (0, 9):
        with pytest.raises(slacken_amd.SlackenError) as e:
            slacken_amd.Pipe(world["ix"], depth)
        assert e.value.code == E_INVALID


def test_pipe_on_an_index_that_is_not_finalized(world, three):
    import slacken_amd
    ix = slacken_amd.Index(expected_records=16, max_taxon=7)
    pipe = slacken_amd.Pipe(ix, 2)
    with pytest.raises(slacken_amd.SlackenError) as e:
        submit_batch(pipe, three[0])
    assert e.value.code == E_STATE and pipe.pending() == 0
    pipe.close()
