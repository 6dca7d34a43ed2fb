"""Cases of the route matrix (test_gpu_routes.py): a library, an index on either side, one batch of reads with every length and
character at which the three classify implementations (lane.hip, fused.hip, kernels.hip) take another path, and the oracle's answers
to it -- computed once per case and shared by every route's leg.  The library and the library-derived reads come from synth.py, the
generator test_gpu_fuzz.py draws from.  Test infrastructure; needs no GPU until Case.engine() is asked for."""
import numpy as np

import synth
import taxgen

THRESHOLDS = (0.0, 0.15, 1.0)
MIN_HIT_GROUPS = (1, 3)
SCALARS = ("taxon", "classified", "num_distinct", "total_kmers", "num_hits")
DEFAULT_XOR = 0xe37e28c4271b5a2d

# the edge strings of test_gpu_parity.py::test_spans_parity
EDGE_STRINGS = (b"", b"N", b"ACGT" * 50, b"A" * 200, b"ACGTU" * 30, b"ACGT" * 9 + b"-" + b"TTGCA" * 20, b"N" * 100, b"AATTTACTTTAGTTAC")


def splitter(k, m, spaces, xor_mask=DEFAULT_XOR, canonical=True):
    return dict(k=k, m=m, spaces=spaces, xor_mask=xor_mask, canonical=canonical)


def route_batch(lib, k, rng, n_varied=400, n_random=110):
    """-> (reads, from_lib): about 600 reads in a fixed shuffled order.  Library-derived and random reads of 0, 1, k-1, k, k+1, 150,
    1000, 1001 and 2500 bases (1000 | 1001: the lane kernel's limit; 2500: its long variant), library-derived reads of 20 .. 300 bases
    with single Ns, N runs and lower case, the same with U for T, random reads, the edge strings."""
    reads, from_lib = [], []

    def add(rs, derived):
        reads.extend(rs)
        from_lib.extend([derived] * len(rs))
    plain = dict(sub_rate=0.01, n_single=0.0, n_run=0.0, lowercase=0.0, short=0.0)
    for L in (0, 1, k - 1, k, k + 1, 150, 1000, 1001, 2500):
        add(synth.make_reads(lib, 3, rng, length=L, frac_random=0.0, **plain), True)
        add(synth.make_reads(lib, 1, rng, length=L, frac_random=1.0, **plain), False)
    add(synth.make_reads(lib, n_varied, rng, length=150, vary_length=True, frac_random=0.0, n_single=0.15, n_run=0.1, lowercase=0.1, short=0.05), True)
    with_u = synth.make_reads(lib, 30, rng, length=150, vary_length=True, frac_random=0.0, n_single=0.1, lowercase=0.3, short=0.0)
    add([np.frombuffer(r.tobytes().replace(b"T", b"U").replace(b"t", b"u"), np.uint8) for r in with_u], True)
    add(synth.make_reads(lib, n_random, rng, length=150, vary_length=True, frac_random=1.0), False)
    add([np.frombuffer(s, np.uint8) for s in EDGE_STRINGS], False)
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], np.array(from_lib, bool)[order]


def ragged_mates(reads):
    """every read gets another read of the batch as its mate: lengths unrelated to its own, empty ones among them"""
    n = len(reads)
    step = next(s for s in (7, 11, 13) if n % s)      # (a permutation of the batch: every read is somebody's mate)
    mates = [reads[(i * step + 3) % n] for i in range(n)]
    assert any(len(m) == 0 for m in mates) and any(len(m) == 0 and len(r) > 0 for r, m in zip(reads, mates))
    return mates


class Case:
    """one library and one batch; the oracle's answers per (paired, min_hit_groups), its hit lists per paired"""

    def __init__(self, orc, ps, parents, keys, taxa, reads, from_lib=None):
        self.orc, self.ps, self.p = orc, ps, orc.params(**ps)
        self.parents, self.keys, self.taxa = parents, keys, taxa
        self.oix = orc.Index(1, keys, taxa)
        self.reads, self.from_lib = reads, from_lib
        self.mates = ragged_mates(reads)
        self.packed = {False: synth.pack(reads) + (None, None), True: synth.pack(reads) + synth.pack(self.mates)}
        self._want, self._lists, self._engine = {}, {}, None

    def want(self, paired, mhg):
        if (paired, mhg) not in self._want:
            b, o, mb, mo = self.packed[paired]
            self._want[paired, mhg] = self.orc.classify_batch(self.p, self.oix, self.parents, b, o, mb, mo, min_hit_groups=mhg, thresholds=THRESHOLDS)
        return self._want[paired, mhg]

    def lists(self, paired):
        """(hit_offsets u64[R + 1], taxon, count) of every read's un-merged hit list, from orc.classify_read read by read"""
        if paired not in self._lists:
            off, tx, cn = [0], [], []
            for i, r in enumerate(self.reads):
                _, hits = self.orc.classify_read(self.p, self.oix, self.parents, r.tobytes(), self.mates[i].tobytes() if paired else None, 1, 0.0)
                tx += [t for t, _ in hits]
                cn += [c for _, c in hits]
                off.append(len(tx))
            self._lists[paired] = (np.array(off, np.uint64), np.array(tx, np.int32), np.array(cn, np.int32))
        return self._lists[paired]

    def prefix(self, paired, R):
        """the first R reads (and mates) alone, packed"""
        b, o = synth.pack(self.reads[:R])
        return (b, o) + (synth.pack(self.mates[:R]) if paired else (None, None))

    def engine(self, **index_kw):
        """(index, stream) on the GPU, made once"""
        if self._engine is None:
            import slacken_amd
            kw = dict(expected_records=len(self.keys), max_taxon=len(self.parents) - 1)
            kw.update(index_kw)
            ix = slacken_amd.Index(**self.ps, **kw)
            ix.append(self.keys, self.taxa)
            ix.set_taxonomy(self.parents)
            ix.finalize()
            self._engine = (ix, ix.stream())
        return self._engine

    def check_not_vacuous(self):
        """what keeps a comparison with this case from passing on empty answers -- all of it the oracle's output"""
        for paired in (False, True):
            w = self.want(paired, 1)
            assert w["classified"][0][self.from_lib].mean() >= 0.5 and self.from_lib.sum() >= 200, (self.ps, paired)
            if not paired:     # (a pair always has its mate border)
                assert (w["num_hits"] == 0).any(), self.ps
            assert (w["num_distinct"] >= 2).sum() >= 10, (self.ps, paired)
            off, tx, _ = self.lists(paired)
            assert np.array_equal(np.diff(off.astype(np.int64)), w["num_hits"]) and len(tx) > len(self.reads)
            assert not np.array_equal(self.want(paired, 3)["classified"], w["classified"])       # min_hit_groups decides something
            assert not np.array_equal(w["classified"][0], w["classified"][-1])                   # ... and so does the threshold


def splitter_case(orc, ps, seed):
    rng = np.random.default_rng(seed)
    p = orc.params(**ps)
    parents = taxgen.taxonomy(8 * 16, rng)
    lib = synth.Library(orc, p, parents, n_genomes=6, genome_len=6000, pad_records=3000, seed=seed)
    keys, taxa = lib.keys, lib.taxa
    if not ps["canonical"]:
        # (make_reads takes half of its reads from the other strand: a library of one strand would leave those without a hit, so this
        #  one holds both -- the records met first stay)
        more = [(orc.minimizer_keys(p, synth.revcomp(g).tobytes()), t) for g, t in zip(lib.genomes, lib.genome_taxa)]
        keys = np.concatenate([keys] + [kk for kk, _ in more])
        taxa = np.concatenate([taxa] + [np.full(len(kk), t, np.int32) for kk, t in more])
        keys, first = np.unique(keys, return_index=True)
        taxa = taxa[first]
    if len(keys) < 1000:
        # (two-letter minimizers: every genome holds all sixteen, and their common ancestor would be the library's only taxon)
        taxa = rng.choice(lib.genome_taxa, size=len(keys)).astype(np.int32)
    reads, from_lib = route_batch(lib, ps["k"], rng)
    return Case(orc, ps, parents, keys, taxa, reads, from_lib)


def many_taxa_case(orc, seed=99):
    """the library of test_gpu_parity.py::test_many_taxa_per_read_take_the_deferred_path: every minimizer of every read is a record with
    a random taxon of its own, so a read of 150 bases names more than 12 taxa (the lane kernel's map) and one of 3000 more than 128
    (the wave kernel's)"""
    ps = splitter(35, 31, 7)
    p = orc.params(**ps)
    rng = np.random.default_rng(seed)
    parents = taxgen.taxonomy(8 * 64, rng)
    defined = np.array(taxgen.defined_taxa(parents))
    reads = [synth.random_dna(3000, rng), synth.random_dna(150, rng), synth.random_dna(6000, rng)]
    reads += [synth.random_dna(150, rng) for _ in range(120)] + [synth.random_dna(400, rng) for _ in range(10)] + [np.zeros(0, np.uint8)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    keys = np.unique(np.concatenate([orc.minimizer_keys(p, r.tobytes()) for r in reads if len(r)]))
    taxa = rng.choice(defined, size=len(keys)).astype(np.int32)
    case = Case(orc, ps, parents, keys, taxa, reads)
    nd = case.want(False, 1)["num_distinct"]
    assert (nd > 12).sum() >= 100 and 2 <= (nd > 128).sum() <= 5
    assert (case.want(True, 1)["num_distinct"] > 128).sum() >= 2
    return case


def wide_case(orc, w, canonical, seed):
    """a window of w m-mers at the host entry: m = 9, k = m + w - 1; 300 reads of k-1 .. 3k bases, most of them library-derived"""
    m = 9
    k = m + w - 1
    ps = splitter(k, m, 0, canonical=canonical)
    rng = np.random.default_rng(seed)
    p = orc.params(**ps)
    parents = taxgen.taxonomy(8 * 16, rng)
    lib = synth.Library(orc, p, parents, n_genomes=6, genome_len=max(6000, 4 * k), pad_records=1000, seed=seed)
    reads, from_lib = [], []
    for i in range(300):
        L = (k - 1, k, k + 1, 3 * k)[i] if i < 4 else int(rng.integers(k - 1, 3 * k + 1))
        derived = i % 5 != 4
        r = synth.make_reads(lib, 1, rng, length=L, frac_random=0.0 if derived else 1.0, sub_rate=0.01, n_single=0.1, n_run=0.05, lowercase=0.05, short=0.0)[0]
        reads.append(r)
        from_lib.append(derived)
    reads.append(np.zeros(0, np.uint8))
    from_lib.append(False)
    order = rng.permutation(len(reads))
    return Case(orc, ps, parents, lib.keys, lib.taxa, [reads[i] for i in order], np.array(from_lib, bool)[order])
