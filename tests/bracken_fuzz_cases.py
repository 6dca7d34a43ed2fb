"""The parameter space of the Bracken weights fuzz (tests/test_bracken_fuzz_model.py on the model, tests/test_gpu_bracken_fuzz.py on
the device): config(seed) derives a splitter, a read length, a max_fragment and a bracken_cases.Case from the seed alone, so that
both tests see the same inputs.  Pinned seeds (PINNED) hold the configurations that must not be left to chance.  Test
infrastructure."""
import os
from dataclasses import dataclass

import numpy as np

import taxgen
from bracken_cases import Case

FRAGMENT_MAX = 1024 * 1024            # BrackenWeights.scala:303; max_fragment = 0 in the C ABI
SPARSE_EXTENT = 1_000_000             # ids of a relabelled taxonomy (NCBI-like: few taxa in a wide id space)
DEFAULT_MASK = 0xe37e28c4271b5a2d


@dataclass
class Config:
    seed: int
    k: int
    m: int
    spaces: int
    canonical: bool
    xor_mask: int
    read_len: int
    max_fragment: int                 # 0: the default (FRAGMENT_MAX)
    n_genomes: int
    genome_len: int
    sparse: bool

    @property
    def w(self):
        return self.k - self.m + 1

    @property
    def fragment(self):
        return self.max_fragment or FRAGMENT_MAX

    def splitter(self):
        return dict(k=self.k, m=self.m, spaces=self.spaces, xor_mask=self.xor_mask, canonical=self.canonical)

    def case(self, orc):
        """The Case of this configuration, relabelled into a sparse id space when the configuration says so."""
        p = orc.params(**self.splitter())
        case = Case(orc, p, seed=7000 + self.seed, n_genomes=self.n_genomes, genome_len=self.genome_len, read_len=self.read_len,
                    extra_short=True)
        if self.sparse:
            parents, remap = taxgen.sparse_relabel(case.parents, SPARSE_EXTENT, np.random.default_rng(7000 + self.seed))
            lut = np.zeros(len(case.parents), np.int32)
            for old, new in remap.items():
                lut[old] = new
            case.parents = parents
            case.rec_taxa = lut[np.asarray(case.rec_taxa)]
            case.index = orc.Index(1, case.keys, case.rec_taxa)
            case.taxa = [int(lut[t]) for t in case.taxa]
            case.sources = [int(lut[t]) for t in case.sources]
        return p, case


# (k, m, spaces, canonical, read_len, max_fragment): constructed, not hoped for
PINNED = {
    1000: (13, 13, 0, True, 50, 0),       # k == m (w = 1): every k-mer its own super-mer
    1001: (24, 24, 5, False, 150, 1500),  # k == m at a second read length, pieces
    1002: (52, 20, 3, True, 100, 0),      # w = 33 with m <= 32: the staged scanner
    1003: (79, 32, 0, True, 250, 5000),   # w = 48
    1004: (35, 31, 7, True, 35, 35),      # read_len == k, max_fragment == read_len: one read per piece, one piece per base
}

READ_LENS = ("k", "k+1", 50, 100, 150, 250, 600, 1000)
FRAGMENTS = ("default", "L", "L+1", "2L", 1500, 5000)


def config(seed):
    if seed in PINNED:
        k, m, spaces, canonical, read_len, max_fragment = PINNED[seed]
        return Config(seed, k, m, spaces, canonical, DEFAULT_MASK, read_len, max_fragment, n_genomes=4,
                      genome_len=2000 if max_fragment and max_fragment <= read_len + 1 else 4000, sparse=bool(seed % 2))
    rng = np.random.default_rng(7000 + seed)
    m = int(rng.integers(8, 33))
    k = int(rng.integers(m, m + (48 if seed % 4 == 3 else 32)))
    spaces = int(rng.integers(0, m // 2 + 1))
    canonical = bool(rng.integers(0, 2))
    xor_mask = int(rng.integers(0, 2**63)) * 2 + 1 if seed % 2 else DEFAULT_MASK
    rl = READ_LENS[seed % len(READ_LENS)]
    read_len = max(k, {"k": k, "k+1": k + 1}.get(rl, rl))
    mf = FRAGMENTS[(seed + seed // len(READ_LENS)) % len(FRAGMENTS)]   # seed // 8: the two cycles drift against each other
    max_fragment = {"default": 0, "L": read_len, "L+1": read_len + 1, "2L": 2 * read_len}.get(mf, mf)
    if max_fragment:
        max_fragment = max(max_fragment, read_len)
    n_genomes = int(rng.integers(2, 8))
    genome_len = int(rng.integers(2000, 6001))
    if max_fragment and max_fragment <= read_len + 1:   # one piece per base: the Python model walks each of them
        genome_len = 2000
    return Config(seed, k, m, spaces, canonical, xor_mask, read_len, max_fragment, n_genomes, genome_len, sparse=bool(seed % 2))


N_DEFAULT = 24
DEFAULT_SEEDS = sorted(set(range(N_DEFAULT)) | set(PINNED))
N_SEEDS = int(os.environ.get("SLK_BRACKEN_FUZZ_SEEDS", N_DEFAULT))   # (a longer soak: SLK_BRACKEN_FUZZ_SEEDS=300)
SEEDS = sorted(set(range(N_SEEDS)) | set(PINNED))
