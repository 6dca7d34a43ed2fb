"""Contig-length fragments are split over many waves (fused.hip segment_body<false, true>, pieces.h): an unpaired
fragment of at least the threshold is cut into pieces of k-mer windows, every piece is a wave's unit, the pieces' counts meet in an
HBM taxon map that cannot overflow, and a merge kernel settles the borders between pieces and resolves the fragment.  Here the pieces
are as small as the engine allows (4 096 windows) and the threshold is two of them, so that fragments of 10-40 kbp have 3-10 pieces
and every border rule is met: against the oracle, and against the same batch on the routes that do not split."""
import os

import numpy as np
import pytest

import pieces_model as pm
import synth
import taxgen

pytestmark = pytest.mark.gpu

PW, MIN_LEN = 4096, 8193
KEYS = ("total_kmers", "num_hits", "num_distinct", "taxon", "classified")
THR = (0.0, 0.1, 0.5)


@pytest.fixture(autouse=True)
def small_pieces(monkeypatch):
    monkeypatch.setenv("SLK_PIECE_WINDOWS", str(PW))
    monkeypatch.setenv("SLK_PIECE_MIN_LEN", str(MIN_LEN))


def make_world(orc, keys, taxa, parents, **extra):
    import slacken_amd
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    return dict(p=orc.params(), parents=parents, st=ix.stream(), oix=orc.Index(1, keys, taxa), ix=ix, **extra)


@pytest.fixture(scope="module")
def world(orc):
    p = orc.params()
    rng = np.random.default_rng(77)
    parents = taxgen.taxonomy(8 * 32, rng)
    lib, keys, taxa = pm.library_with_repeats(orc, p, parents, rng)
    return make_world(orc, keys, taxa, parents, lib=lib)


def n_pieces(n_bases, k=35):
    return -(-(n_bases - k + 1) // PW)


def unsplit(world, bases, offsets, **kw):
    """the same batch on today's routes"""
    saved = os.environ.get("SLK_PIECE_MIN_LEN")
    os.environ["SLK_PIECE_MIN_LEN"] = "0"
    try:
        got = world["st"].classify_batch(bases, offsets, with_hits=False, with_num_hits=True, **kw)
        assert world["st"].last_split() == (0, 0, 0)
        return got
    finally:
        os.environ.pop("SLK_PIECE_MIN_LEN")
        if saved is not None:
            os.environ["SLK_PIECE_MIN_LEN"] = saved


def check(orc, world, reads, thresholds=THR, min_hit_groups=2):
    bases, offsets = synth.pack(reads)
    got = world["st"].classify_batch(bases, offsets, thresholds=thresholds, min_hit_groups=min_hit_groups, with_hits=False, with_num_hits=True)
    split = world["st"].last_split()
    want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=min_hit_groups,
                              thresholds=thresholds)
    for key in KEYS:
        bad = np.nonzero(np.atleast_2d(got[key] != want[key]).any(axis=0))[0]
        assert bad.size == 0, (key, bad[:5].tolist(), [len(reads[i]) for i in bad[:5]],
                               np.atleast_2d(got[key])[:, bad[:5]].tolist(), np.atleast_2d(want[key])[:, bad[:5]].tolist())
    other = unsplit(world, bases, offsets, thresholds=thresholds, min_hit_groups=min_hit_groups)
    for key in KEYS:
        assert np.array_equal(other[key], got[key]), "today's routes vs the piece route: " + key
    long_ones = [r for r in reads if len(r) >= MIN_LEN]
    assert split[:2] == (len(long_ones), sum(n_pieces(len(r)) for r in long_ones)), split
    return got, split


@pytest.mark.parametrize("seed", range(4))
def test_a_mixed_batch(orc, world, seed):
    rng = np.random.default_rng(300 + seed)
    lib = world["lib"]
    reads = [pm.long_read(lib, rng, int(rng.integers(MIN_LEN, 40001))) for _ in range(40)]
    reads += synth.make_reads(lib, 200, rng, vary_length=True)
    reads += [pm.long_read(lib, rng, int(rng.integers(1001, 8001))) for _ in range(20)]
    order = rng.permutation(len(reads))
    got, split = check(orc, world, [reads[i] for i in order], min_hit_groups=int(rng.integers(1, 4)))
    assert split[0] == 40 and got["classified"][0].mean() > 0.3


def test_borders_one_by_one(orc, world):
    """One read; the same read with a run of Ns (shorter than, equal to, longer than k) or a repeat slid across the border between
    its first two pieces (window 4 096 = base 4 096); fragments that are one span cut by every border; a last piece of one window."""
    g = np.concatenate(world["lib"].genomes[:2])
    base = g[20000:33000].copy()
    reads = [base]
    for ins_len in (1, 34, 35, 36, 70):
        for at in range(PW - 72, PW + 38, 3):
            r = base.copy()
            r[at:at + ins_len] = ord("N")
            reads.append(r)
    unit = np.frombuffer(b"AC", np.uint8)
    for at in range(PW - 310, PW + 40, 7):
        r = base.copy()
        r[at:at + 300] = np.tile(unit, 150)
        reads.append(r)
    reads.append(np.full(20000, ord("N"), np.uint8))                   # one ambiguous span, cut four times
    reads.append(np.tile(np.frombuffer(b"ACGGT", np.uint8), 4000))     # one minimizer value throughout
    reads.append(np.full(12000, ord("A"), np.uint8))
    for n in (2 * PW + 34 - 1, 2 * PW + 34, 2 * PW + 34 + 1):          # two whole pieces; ... and a last piece of one window
        reads.append(g[1000:1000 + n].copy())
    check(orc, world, reads)


def test_the_nearest_earlier_piece_that_has_a_super_mer(orc, world):
    """sequence at both ends and 9 000 Ns between: a whole piece holds no super-mer, and the keys either side of it are equal"""
    flank = world["lib"].genomes[3][:200]
    rep = np.tile(np.frombuffer(b"AC", np.uint8), 100)
    reads = [np.concatenate([f, np.full(9000, ord("N"), np.uint8), f]) for f in (flank, rep)]
    reads.append(np.concatenate([rep, np.full(13000, ord("N"), np.uint8), rep, np.full(5000, ord("N"), np.uint8), rep]))
    check(orc, world, reads, min_hit_groups=1)


@pytest.fixture(scope="module")
def many_taxa_world(orc):
    """every minimizer of the fragments is a record with a random taxon (tests/test_gpu_parity.py: the deferred path's recipe)"""
    p = orc.params()
    rng = np.random.default_rng(99)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    big = [synth.random_dna(12000, rng), synth.random_dna(30000, rng), synth.random_dna(30000, rng), synth.random_dna(12000, rng)]
    kk = np.unique(np.concatenate([orc.minimizer_keys(p, b.tobytes()) for b in big]))
    many = rng.choice(taxa, size=len(kk), replace=True).astype(np.int32)
    return make_world(orc, kk, many, parents, big=big)


def run_device(st, bases, offsets, thresholds=THR, min_hit_groups=2):
    """slk_classify_batch_device, queued: -> the tensors that hold the batch and will hold its results"""
    import torch
    n = len(offsets) - 1
    d_b, d_o = torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()
    outs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    d_t = torch.zeros(len(thresholds) * n, dtype=torch.int32, device="cuda")
    d_c = torch.zeros(len(thresholds) * n, dtype=torch.uint8, device="cuda")
    st.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, int(offsets[-1]), d_t.data_ptr(), d_c.data_ptr(), outs[0].data_ptr(),
                             outs[1].data_ptr(), outs[2].data_ptr(), min_hit_groups=min_hit_groups, thresholds=thresholds)
    return dict(n=n, C=len(thresholds), keep=(d_b, d_o), t=d_t, c=d_c, outs=outs)


def fetch(q):
    n, C = q["n"], q["C"]
    return dict(taxon=q["t"].cpu().numpy().reshape(C, n), classified=q["c"].cpu().numpy().reshape(C, n), num_distinct=q["outs"][0].cpu().numpy(),
                total_kmers=q["outs"][1].cpu().numpy(), num_hits=q["outs"][2].cpu().numpy())


def test_more_than_128_taxa_stay_on_the_route(orc, many_taxa_world):
    w = many_taxa_world
    got, split = check(orc, w, w["big"])
    assert (got["num_distinct"] > 128).all()
    assert split[2] > 0                      # a piece of 4 096 windows names several hundred taxa: its wave emptied a full map
    # two batches queued before one synchronisation: neither waits for, or is classified again with, the other
    st = w["st"]
    batches = [synth.pack(w["big"][:2]), synth.pack(w["big"][2:] + [w["big"][0][:9000].copy()])]
    queued = [run_device(st, b, o) for b, o in batches]
    st.synchronize()
    assert st.last_split()[:2] == (3, n_pieces(30000) + n_pieces(12000) + n_pieces(9000))
    for (b, o), q in zip(batches, queued):
        want = orc.classify_batch(w["p"], w["oix"], w["parents"], b, o, None, None, min_hit_groups=2, thresholds=THR)
        res = fetch(q)
        for key in KEYS:
            assert np.array_equal(res[key], want[key]), key


def test_a_map_bounded_by_the_taxonomy(orc):
    """33 taxa and a fragment of 40 000 bases: the fragment's map is sized by the taxa, not by its windows -- and every taxon is hit"""
    p = orc.params()
    rng = np.random.default_rng(5)
    parents = taxgen.taxonomy(24, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    assert len(parents) - 1 == 33 and len(taxa) == 33
    reads = [synth.random_dna(40000, rng), synth.random_dna(9000, rng)]
    kk = np.unique(np.concatenate([orc.minimizer_keys(p, r.tobytes()) for r in reads]))
    tx = rng.choice(taxa, size=len(kk), replace=True).astype(np.int32)
    w = make_world(orc, kk, tx, parents)
    _, hits = orc.classify_read(p, w["oix"], parents, reads[0].tobytes(), None, 2, 0.0)
    assert len({t for t, _ in hits if t > 0}) == 33                   # the fragment's distinct taxa equal the taxonomy's size
    check(orc, w, reads)


def test_more_units_than_the_grid(orc, world):
    """The piece kernel's grid is fixed and the number of pieces is only known on the device: a wave takes the unit of its own number
    first and draws further ones from a counter.  Two or three pieces per fragment, more pieces than waves; the batch stays on the device."""
    grid_waves = world["st"].split_info()[0]
    n = grid_waves // 2 + 150
    rng = np.random.default_rng(78)
    lib = world["lib"]
    cat = np.concatenate(lib.genomes)
    lens = rng.integers(8200, 8401, n)
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    starts = rng.integers(0, len(cat) - 8400, n)
    rid = np.repeat(np.arange(n), lens)
    bases = cat[starts[rid] + (np.arange(int(offsets[-1])) - offsets[:-1].astype(np.int64)[rid])].copy()
    subs = rng.random(len(bases)) < 0.01
    bases[subs] = synth.random_dna(int(subs.sum()), rng)
    bases[rng.random(len(bases)) < 0.0005] = ord("N")
    st = world["st"]
    q = run_device(st, bases, offsets, thresholds=(0.0, 0.2))
    st.synchronize()
    units = sum(n_pieces(int(x)) for x in lens)         # two or three pieces each
    assert st.last_split()[:2] == (n, units) and units > grid_waves
    want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=2, thresholds=(0.0, 0.2))
    res = fetch(q)
    for key in KEYS:
        assert np.array_equal(res[key], want[key]), key


def test_a_batch_without_a_long_fragment_runs_nothing_of_the_route(orc, world):
    """The entries that take host arrays plan from the fragments' lengths: a batch whose longest fragment is under the threshold
    allocates and launches nothing (a fresh stream keeps no scratch), however many bases it holds; a batch with long fragments gets
    the scratch their pieces and maps need, not the worst case of its size."""
    rng = np.random.default_rng(21)
    lib = world["lib"]
    st = world["ix"].stream()
    try:
        reads = [pm.long_read(lib, rng, int(rng.integers(5000, MIN_LEN))) for _ in range(30)]
        bases, offsets = synth.pack(reads)
        assert len(bases) > 10 * MIN_LEN
        st.classify_batch(bases, offsets, thresholds=THR, with_hits=False, with_num_hits=True)
        assert st.last_split() == (0, 0, 0) and st.split_info()[1] == 0
        reads += [pm.long_read(lib, rng, 20000), pm.long_read(lib, rng, MIN_LEN)]
        bases, offsets = synth.pack(reads)
        got = st.classify_batch(bases, offsets, thresholds=THR, with_hits=False, with_num_hits=True)
        want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=2, thresholds=THR)
        for key in KEYS:
            assert np.array_equal(got[key], want[key]), key
        assert st.last_split()[:2] == (2, n_pieces(20000) + n_pieces(MIN_LEN))
        # two maps of 2 (512 + 1) -> 2048 entries of 8 bytes (9 taxon bits), 8 units of 56 bytes, two slots, the header; DevBuf adds an eighth
        assert 0 < st.split_info()[1] < 2 * (2 * 2048 * 8 + 8 * 56 + 2 * 32 + 64)
    finally:
        st.close()


def test_off_and_refused(orc, world, monkeypatch):
    import slacken_amd
    rng = np.random.default_rng(8)
    lib = world["lib"]
    reads = [pm.long_read(lib, rng, int(n)) for n in (9000, 20000, 31000, 3000, 150)]
    bases, offsets = synth.pack(reads)
    st = world["st"]
    kw = dict(thresholds=THR, min_hit_groups=2)
    want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=2, thresholds=THR)
    # the setter: the environment overrides it, so it is taken away here
    monkeypatch.delenv("SLK_PIECE_MIN_LEN")
    try:
        st.set_split_long(MIN_LEN)
        on = st.classify_batch(bases, offsets, with_hits=False, with_num_hits=True, **kw)
        assert st.last_split()[:2] == (3, n_pieces(9000) + n_pieces(20000) + n_pieces(31000))
        st.set_split_long(0)
        off = st.classify_batch(bases, offsets, with_hits=False, with_num_hits=True, **kw)
        assert st.last_split() == (0, 0, 0)
        for key in KEYS:
            assert np.array_equal(on[key], want[key]) and np.array_equal(off[key], want[key]), key
        # hit lists, and mates: those calls keep today's routes
        st.set_split_long(MIN_LEN)
        hits = st.classify_batch(bases, offsets, with_hits=True, **kw)
        assert st.last_split()[0] == 0
        mates = [pm.long_read(lib, rng, int(n)) for n in (9000, 300, 12000, 100, 150)]
        mb, mo = synth.pack(mates)
        paired = st.classify_batch(bases, offsets, mb, mo, with_hits=False, with_num_hits=True, **kw)
        assert st.last_split()[0] == 0
        want_p = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, mb, mo, min_hit_groups=2, thresholds=THR)
        for key in KEYS:
            assert np.array_equal(hits[key], want[key]) and np.array_equal(paired[key], want_p[key]), key
        with pytest.raises(slacken_amd.capi.SlackenError) as e:
            st.set_split_long(-2)
        assert e.value.code == -1                     # SLK_E_INVALID
    finally:
        st.set_split_long(-1)


def test_through_the_pipe_and_the_text_entry(orc, world, monkeypatch, capfd):
    import slacken_amd
    rng = np.random.default_rng(301)
    lib = world["lib"]
    reads = [pm.long_read(lib, rng, int(rng.integers(MIN_LEN, 40001))) for _ in range(12)]
    reads += synth.make_reads(lib, 60, rng, vary_length=True) + [pm.long_read(lib, rng, int(rng.integers(1001, 8001))) for _ in range(8)]
    reads = [r for r in reads if len(r) > 0]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    bases, offsets = synth.pack(reads)
    want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=2, thresholds=THR)
    n_long = sum(len(r) >= MIN_LEN for r in reads)
    said = "slk split: %d fragments, %d pieces" % (n_long, sum(n_pieces(len(r)) for r in reads if len(r) >= MIN_LEN))
    monkeypatch.setenv("SLK_DEBUG_SPLIT", "1")        # (a pipe's streams are its own: the engine says on stderr what the route did)
    pipe = slacken_amd.capi.Pipe(world["ix"], depth=2)
    try:
        capfd.readouterr()
        tickets = [pipe.submit(dict(bases=bases, offsets=offsets), thresholds=THR, hits=1) for _ in range(2)]
        for t in tickets:
            got = pipe.collect(t)
            for key in KEYS:
                assert np.array_equal(got[key], want[key]), "pipe: " + key
        assert capfd.readouterr().err.count(said) == 2
    finally:
        pipe.close()
    monkeypatch.delenv("SLK_DEBUG_SPLIT")
    text = b"".join(b">r%d\n%s\n" % (i, r.tobytes()) for i, r in enumerate(reads))
    got = world["st"].classify_text(text, "fasta", thresholds=THR, with_hits=False)
    assert world["st"].last_split()[0] == n_long
    for key in ("total_kmers", "num_distinct", "taxon", "classified"):
        assert np.array_equal(got[key], want[key]), "text: " + key


def test_default_switches(orc, world, monkeypatch):
    """No SLK_PIECE_* variable and the setter untouched: the engine's default -- fragments of at least 300 000 bases, in pieces of 65 536
    windows, in a batch whose fragments average over 1000 bases -- and the same call with the setter alone."""
    monkeypatch.delenv("SLK_PIECE_MIN_LEN")
    monkeypatch.delenv("SLK_PIECE_WINDOWS")
    rng = np.random.default_rng(3)
    reads = [pm.long_read(world["lib"], rng, 400_000), pm.long_read(world["lib"], rng, 70_000)]
    bases, offsets = synth.pack(reads)
    st = world["st"]
    want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=2, thresholds=THR)
    got = st.classify_batch(bases, offsets, thresholds=THR, with_hits=False, with_num_hits=True)
    assert st.last_split()[:2] == (1, -(-(400_000 - 34) // 65536))
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    # reads in the same batch, so that its fragments average under 1000 bases: the engine's own choice leaves such a batch alone
    short = synth.make_reads(world["lib"], 600, rng)
    b2, o2 = synth.pack(reads + short)
    want2 = orc.classify_batch(world["p"], world["oix"], world["parents"], b2, o2, None, None, min_hit_groups=2, thresholds=THR)
    got2 = st.classify_batch(b2, o2, thresholds=THR, with_hits=False, with_num_hits=True)
    assert st.last_split() == (0, 0, 0)
    try:
        st.set_split_long(65537)
        got3 = st.classify_batch(b2, o2, thresholds=THR, with_hits=False, with_num_hits=True)
        assert st.last_split()[:2] == (2, -(-(400_000 - 34) // 65536) + -(-(70_000 - 34) // 65536))
        for key in KEYS:
            assert np.array_equal(got2[key], want2[key]) and np.array_equal(got3[key], want2[key]), key
    finally:
        st.set_split_long(-1)
