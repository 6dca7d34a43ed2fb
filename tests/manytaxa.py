"""A batch that takes the unbounded re-run (status bit 1: a fragment with more than 128 distinct taxa overflows the wave kernel's map
and the whole batch is classified again by the staged kernels), for the tests of the host entries that end in it: 300 reads of
150 bases around one of 3000 whose every minimizer is a record with a random taxon of some 500."""
import numpy as np

import synth
import taxgen

THR = (0.0, 0.3)
BIG = 100     # the long read's place: with SLK_HOST_SUBBATCH=64 in the second of five sub-batches
KEYS = ("taxon", "classified", "num_distinct", "total_kmers")


def world(orc, seed):
    import slacken_amd
    p = orc.params()
    rng = np.random.default_rng(seed)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    reads = [synth.random_dna(150, rng) for _ in range(300)]
    reads.insert(BIG, synth.random_dna(3000, rng))
    keys = np.unique(np.concatenate([orc.minimizer_keys(p, r.tobytes()) for r in reads]))
    tx = rng.choice(taxa, size=len(keys)).astype(np.int32)
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1)
    ix.append(keys, tx)
    ix.set_taxonomy(parents)
    ix.finalize()
    return dict(p=p, ix=ix, st=ix.stream(), oix=orc.Index(1, keys, tx), parents=parents, reads=reads)


def check(orc, w, got, want, with_hits, reads, mates=None):
    """got against the oracle's batch results `want`, read by read; with hit lists: every list's length, and the long read's list"""
    assert want["num_distinct"][BIG] > 128
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    if with_hits:
        assert np.array_equal(np.diff(got["hit_offsets"].astype(np.int64)), want["num_hits"])
        for i in (BIG - 1, BIG, BIG + 1, len(reads) - 1):
            _, hits = orc.classify_read(w["p"], w["oix"], w["parents"], reads[i].tobytes(), None if mates is None else mates[i].tobytes(), 2, THR[0])
            g = got["hits"][int(got["hit_offsets"][i]):int(got["hit_offsets"][i + 1])]
            assert [(int(t), int(c)) for t, c in zip(g["taxon"], g["count"])] == hits
