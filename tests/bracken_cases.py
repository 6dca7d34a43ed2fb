"""Inputs for the Bracken tests: genomes under a random taxonomy with shared stretches (so that minimizers have LCA records
above the leaves) and the adversarial features of BrackenWeights' piece handling -- N runs and IUPAC codes within the first
readLen bases of a record or piece, runs of valid bases shorter than k between ambiguous ones, lowercase and U, records
shorter than readLen or k.  Test infrastructure."""
import numpy as np

import synth
import taxgen


def mutate(g, rng, k, read_len, n_features=6):
    g = g.copy()
    n = len(g)
    for _ in range(n_features):
        kind = rng.integers(0, 5)
        a = int(rng.integers(0, max(1, min(n - 1, 2 * read_len)))) if rng.random() < 0.6 else int(rng.integers(0, n))
        if kind == 0:     # N run
            g[a:a + int(rng.integers(1, 12))] = ord("N")
        elif kind == 1:   # IUPAC code
            g[a] = ord("RYKMSWBDHV"[rng.integers(0, 10)])
        elif kind == 2:   # a valid run shorter than k between ambiguous bases
            short = int(rng.integers(1, k))
            g[a] = ord("N")
            if a + short + 1 < n:
                g[a + short + 1] = ord("N")
        elif kind == 3:   # lowercase
            g[a:a + 40] = np.char.lower(g[a:a + 40].view("S1")).view(np.uint8)
        else:             # U for T
            seg = g[a:a + 40]
            seg[seg == ord("T")] = ord("U")
    return g


class Case:
    """An index (oracle records) over a few genomes, and the records to simulate reads from."""

    def __init__(self, orc, p, seed, n_genomes=6, genome_len=3000, read_len=100, extra_short=True):
        rng = np.random.default_rng(seed)
        self.p = p
        self.parents = taxgen.taxonomy(8 * 6, rng)
        taxa = np.array(taxgen.defined_taxa(self.parents))
        leaves = np.setdiff1d(taxa, self.parents[taxa])
        self.taxa = [int(t) for t in rng.choice(leaves, size=min(n_genomes, len(leaves)), replace=False)]
        genomes = [synth.random_dna(genome_len, rng) for _ in self.taxa]
        for g in range(1, len(genomes)):   # shared stretches => LCA records, ancestor destinations
            src = genomes[int(rng.integers(0, g))]
            for _ in range(3):
                a = int(rng.integers(0, genome_len - 400))
                genomes[g][a:a + 400] = src[a:a + 400]
        lib_bases = np.concatenate(genomes)
        lib_off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.uint64)
        self.keys, self.rec_taxa = orc.build_records(p, self.parents, lib_bases, lib_off, np.array(self.taxa, np.int32))
        self.index = orc.Index(1, self.keys, self.rec_taxa)
        self.records, self.sources = [], []
        for g, t in zip(genomes, self.taxa):
            self.records.append(mutate(g, rng, p.k, read_len).tobytes())
            self.sources.append(t)
        if extra_short:
            for ln in (p.k - 1, p.k, read_len - 1, read_len, read_len + 1, read_len + 7):
                g = synth.random_dna(ln, rng)
                self.records.append(g.tobytes())
                self.sources.append(self.taxa[int(rng.integers(0, len(self.taxa)))])
            # a record that starts with a valid run shorter than k and an N run (ambiguous segments at a piece start; the quirk
            # itself needs a later SEQUENCE segment that ends just past the first window: bracken_hard.quirk_record)
            g = genomes[0][:read_len * 3].copy()
            g[20:25] = ord("N")
            self.records.append(g.tobytes())
            self.sources.append(self.taxa[0])

    def packed(self, order=None):
        recs = self.records if order is None else [self.records[i] for i in order]
        src = self.sources if order is None else [self.sources[i] for i in order]
        bases = np.frombuffer(b"".join(recs), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
        return bases, off, np.array(src, np.int32)
