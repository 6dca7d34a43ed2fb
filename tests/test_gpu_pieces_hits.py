"""Hit lists on the piece route (slk_stream_set_split_hits; fused.hip segment_body<true, true>, pieces.h
piece_move_kernel): a call that wants hit lists takes the route once the caller asked for it, and its lists -- hit_offsets, taxon and
k-mers of every entry, merged or not -- are those of the routes that do not split, and the oracle's.  Sizes as in test_gpu_pieces.py:
pieces of 4 096 windows, a threshold of two pieces, fragments of 3-10 pieces, so that every border rule is met; and one fragment of
more than 64 pieces, which the merge plans in two rounds."""
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
    monkeypatch.delenv("SLK_PIECE_HITS", raising=False)


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


def merged_lists(hit_offsets, hits):
    """TaxonCounts.fromHits over every fragment's list: adjacent entries of one taxon become one, counts summed (test_gpu_parity.py)"""
    ho = hit_offsets.astype(np.int64)
    n = len(hits)
    if n == 0:
        return np.zeros(len(ho), np.uint64), hits[:0]
    first_of_read = np.zeros(n, bool)
    first_of_read[ho[:-1][ho[:-1] < n]] = True
    start = first_of_read.copy()
    start[1:] |= hits["taxon"][1:] != hits["taxon"][:-1]
    run = np.cumsum(start) - 1
    out = np.zeros(int(run[-1]) + 1, hits.dtype)
    out["taxon"] = hits["taxon"][start]
    out["count"] = np.bincount(run, weights=hits["count"].astype(np.float64)).astype(np.int64)
    runs_before = np.concatenate([[0], np.cumsum(start)])
    return runs_before[ho].astype(np.uint64), out


def same_lists(a, b, what):
    assert np.array_equal(a["hit_offsets"], b["hit_offsets"]), what + ": hit_offsets"
    bad = np.nonzero((a["hits"]["taxon"] != b["hits"]["taxon"]) | (a["hits"]["count"] != b["hits"]["count"]))[0]
    assert bad.size == 0, (what, bad[:5].tolist(), a["hits"][bad[:5]].tolist(), b["hits"][bad[:5]].tolist())


def expected_split(reads):
    long_ones = [r for r in reads if len(r) >= MIN_LEN]
    return (len(long_ones), sum(n_pieces(len(r)) for r in long_ones))


def check(orc, world, reads, thresholds=THR, min_hit_groups=2, oracle_scalars=True):
    """the batch with the switch on (the route ran: last_split says so) against the same call with the switch off, the oracle's scalars,
    the oracle's list of every long fragment, and the merged lists"""
    st = world["st"]
    bases, offsets = synth.pack(reads)
    kw = dict(thresholds=thresholds, min_hit_groups=min_hit_groups)
    plain = st.classify_batch(bases, offsets, **kw)
    assert st.last_split() == (0, 0, 0)
    st.set_split_hits(True)
    try:
        got = st.classify_batch(bases, offsets, **kw)
        split = st.last_split()
        assert split[:2] == expected_split(reads), split
        st.set_merged_hits(True)
        try:
            mg = st.classify_batch(bases, offsets, **kw)
            assert st.last_split()[:2] == expected_split(reads)
        finally:
            st.set_merged_hits(False)
    finally:
        st.set_split_hits(False)
    for key in KEYS:
        assert np.array_equal(got[key], plain[key]), "switch on vs off: " + key
    same_lists(got, plain, "switch on vs off")
    if oracle_scalars:
        want = orc.classify_batch(world["p"], world["oix"], world["parents"], bases, offsets, None, None, min_hit_groups=min_hit_groups,
                                  thresholds=thresholds)
        for key in KEYS:
            assert np.array_equal(got[key], want[key]), "oracle: " + key
    ho = got["hit_offsets"].astype(np.int64)
    for i, r in enumerate(reads):
        if len(r) < MIN_LEN:
            continue
        _, hits = orc.classify_read(world["p"], world["oix"], world["parents"], r.tobytes(), None, min_hit_groups, thresholds[0])
        g = got["hits"][ho[i]:ho[i + 1]]
        assert [(int(t), int(c)) for t, c in zip(g["taxon"], g["count"])] == hits, (i, len(r))
    want_off, want_hits = merged_lists(got["hit_offsets"], got["hits"])
    assert np.array_equal(mg["hit_offsets"], want_off), "merged lists: offsets"
    assert np.array_equal(mg["hits"]["taxon"], want_hits["taxon"]) and np.array_equal(mg["hits"]["count"], want_hits["count"]), "merged lists"
    for key in ("taxon", "classified", "num_distinct", "total_kmers"):
        assert np.array_equal(mg[key], plain[key]), "merged lists: " + key
    return got, split


def mixed_batch(world, seed):
    rng = np.random.default_rng(300 + seed)
    lib = world["lib"]
    reads = [pm.long_read(lib, rng, int(rng.integers(MIN_LEN, 40001))) for _ in range(40)]
    reads += synth.make_reads(lib, 200, rng, vary_length=True)
    reads += [pm.long_read(lib, rng, int(rng.integers(1001, 8001))) for _ in range(20)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], int(rng.integers(1, 4))


@pytest.mark.parametrize("seed", range(4))
def test_a_mixed_batch(orc, world, seed):
    reads, mhg = mixed_batch(world, seed)
    got, split = check(orc, world, reads, min_hit_groups=mhg)
    assert split[0] == 40 and got["classified"][0].mean() > 0.3


def test_borders_one_by_one(orc, world):
    """test_gpu_pieces.py's read set: a run of Ns (shorter than, equal to, longer than k) or a repeat slid across the border between the
    first two pieces; fragments that are ONE entry cut by every border; a last piece of one window"""
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
    got, _ = check(orc, world, reads)
    ho = got["hit_offsets"].astype(np.int64)
    i = len(reads) - 6
    for j in (i, i + 1):                              # 20 000 Ns, ACGGT x 4 000: ONE entry that holds every window of the fragment
        assert ho[j + 1] - ho[j] == 1 and int(got["hits"]["count"][ho[j]]) == 20000 - 34
    assert int(got["hits"]["taxon"][ho[i]]) == -1    # AMBIGUOUS_SPAN


def test_the_nearest_earlier_piece_that_has_a_super_mer(orc, world):
    """sequence at both ends and 9 000 Ns between: a whole piece is nothing but the continuation of an earlier entry"""
    flank = world["lib"].genomes[3][:200]
    rep = np.tile(np.frombuffer(b"AC", np.uint8), 100)
    reads = [np.concatenate([f, np.full(9000, ord("N"), np.uint8), f]) for f in (flank, rep)]
    reads.append(np.concatenate([rep, np.full(13000, ord("N"), np.uint8), rep, np.full(5000, ord("N"), np.uint8), rep]))
    check(orc, world, reads, min_hit_groups=1)


def test_more_than_64_pieces(orc, world):
    """the merge reads 64 pieces' records at a time: a fragment of 68 pieces, with an ambiguous span and one super-mer that each run
    from the first 64 pieces into the rest, beside a fragment of three"""
    rng = np.random.default_rng(11)
    lib = world["lib"]
    big = pm.long_read(lib, rng, 68 * PW - 500)
    big[62 * PW + 100:65 * PW + 7] = ord("N")
    chain = np.concatenate([pm.long_read(lib, rng, 63 * PW + 1000), np.tile(np.frombuffer(b"ACGGT", np.uint8), 2000), pm.long_read(lib, rng, 3000)])
    assert n_pieces(len(big)) == 68 and n_pieces(len(chain)) > 64
    check(orc, world, [big, pm.long_read(lib, rng, 9000), chain])


@pytest.fixture(scope="module")
def many_taxa_world(orc):
    """every minimizer of the fragments is a record with a random taxon (test_gpu_pieces.py's recipe)"""
    p = orc.params()
    rng = np.random.default_rng(99)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    big = [synth.random_dna(12000, rng), synth.random_dna(30000, rng), synth.random_dna(30000, rng), synth.random_dna(12000, rng)]
    kk = np.unique(np.concatenate([orc.minimizer_keys(p, b.tobytes()) for b in big]))
    many = rng.choice(taxa, size=len(kk), replace=True).astype(np.int32)
    return make_world(orc, kk, many, parents, big=big)


def test_many_taxa_per_piece(orc, many_taxa_world):
    """the wave's LDS map spills into the fragment's map while the lists are being written"""
    w = many_taxa_world
    got, split = check(orc, w, w["big"])
    assert (got["num_distinct"] > 128).all()
    assert split[2] > 0


def test_packed_and_text_entries(orc, world):
    reads, mhg = mixed_batch(world, 0)
    reads = [r for r in reads if len(r) > 0]
    bases, offsets = synth.pack(reads)
    st = world["st"]
    kw = dict(thresholds=THR, min_hit_groups=mhg)
    plain = st.classify_batch(bases, offsets, **kw)
    text = b"".join(b">r%d\n%s\n" % (i, r.tobytes()) for i, r in enumerate(reads))
    st.set_split_hits(True)
    try:
        pk = st.classify_batch(bases, offsets, packed=True, **kw)
        assert st.last_split()[:2] == expected_split(reads)
        tx = st.classify_text(text, "fasta", **kw)
        assert st.last_split()[:2] == expected_split(reads)
    finally:
        st.set_split_hits(False)
    for key in KEYS:
        assert np.array_equal(pk[key], plain[key]), "packed: " + key
    same_lists(pk, plain, "packed")
    assert tx["R"] == len(reads)
    for key in ("total_kmers", "num_distinct", "taxon", "classified"):
        assert np.array_equal(tx[key], plain[key]), "text: " + key
    same_lists(tx, plain, "text")


def test_off_means_off(orc, world, monkeypatch):
    rng = np.random.default_rng(8)
    reads = [pm.long_read(world["lib"], rng, int(n)) for n in (9000, 20000, 31000, 3000, 150)]
    bases, offsets = synth.pack(reads)
    st = world["st"]
    kw = dict(thresholds=THR, min_hit_groups=2)
    monkeypatch.delenv("SLK_PIECE_MIN_LEN")          # (the environment overrides the setter)
    try:
        st.set_split_long(MIN_LEN)
        off = st.classify_batch(bases, offsets, **kw)
        assert st.last_split() == (0, 0, 0)          # the switch is off by default
        st.set_split_hits(True)
        on = st.classify_batch(bases, offsets, **kw)
        assert st.last_split()[:2] == expected_split(reads)
        monkeypatch.setenv("SLK_PIECE_HITS", "0")    # ... and the environment overrides this setter too
        env_off = st.classify_batch(bases, offsets, **kw)
        assert st.last_split() == (0, 0, 0)
        monkeypatch.delenv("SLK_PIECE_HITS")
        st.set_split_long(-1)                        # unasked: hit-list calls stay off the route whatever the switch says
        unasked = st.classify_batch(bases, offsets, **kw)
        assert st.last_split() == (0, 0, 0)
        st.set_split_long(0)
        never = st.classify_batch(bases, offsets, **kw)
        assert st.last_split() == (0, 0, 0)
        st.set_split_hits(False)
        monkeypatch.setenv("SLK_PIECE_HITS", "1")
        st.set_split_long(MIN_LEN)
        env_on = st.classify_batch(bases, offsets, **kw)
        assert st.last_split()[:2] == expected_split(reads)
        # mates keep their routes with the switch on as well
        st.set_split_hits(True)
        mates = [pm.long_read(world["lib"], rng, int(n)) for n in (9000, 300, 12000, 100, 150)]
        mb, mo = synth.pack(mates)
        st.classify_batch(bases, offsets, mb, mo, **kw)
        assert st.last_split() == (0, 0, 0)
    finally:
        st.set_split_long(-1)
        st.set_split_hits(False)
    for other, what in ((on, "on"), (env_off, "SLK_PIECE_HITS=0"), (unasked, "unasked"), (never, "split_long 0"), (env_on, "SLK_PIECE_HITS=1")):
        for key in KEYS:
            assert np.array_equal(other[key], off[key]), what + ": " + key
        same_lists(other, off, what)


def test_through_the_pipe(orc, world, monkeypatch, capfd):
    import slacken_amd
    rng = np.random.default_rng(301)
    lib = world["lib"]
    reads = [pm.long_read(lib, rng, int(rng.integers(MIN_LEN, 40001))) for _ in range(12)]
    reads += synth.make_reads(lib, 60, rng, vary_length=True) + [pm.long_read(lib, rng, int(rng.integers(1001, 8001))) for _ in range(8)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    bases, offsets = synth.pack(reads)
    want = world["st"].classify_batch(bases, offsets, thresholds=THR)
    assert world["st"].last_split() == (0, 0, 0)
    said = "slk split: %d fragments, %d pieces" % expected_split(reads)
    monkeypatch.setenv("SLK_PIECE_HITS", "1")         # (a pipe's streams are its own: the environment reaches them)
    monkeypatch.setenv("SLK_DEBUG_SPLIT", "1")
    pipe = slacken_amd.capi.Pipe(world["ix"], depth=2)
    try:
        capfd.readouterr()
        tickets = [pipe.submit(dict(bases=bases, offsets=offsets), thresholds=THR, hits=2) for _ in range(2)]
        for t in tickets:
            got = pipe.collect(t)
            for key in KEYS:
                assert np.array_equal(got[key], want[key]), "pipe: " + key
            same_lists(got, want, "pipe")
        assert capfd.readouterr().err.count(said) == 2
    finally:
        pipe.close()
