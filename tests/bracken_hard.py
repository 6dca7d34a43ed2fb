"""Inputs that drive the Bracken window kernel down its rare routes, with the evidence that they do (test infrastructure):

quirk_record()   a record whose first piece starts with a short SEQUENCE segment and an N, then a segment whose last super-mer
                 covers k-mer W of the first window: the trailing-hit ordinal of BrackenWeights.scala:230 takes that super-mer's
                 k-mers [W, t0) from its taxon.  Checked on the model: piece_arrays finds the quirk and the literal
                 window counts differ from the true ones.
ManyTaxa        an index whose records over one stretch of genome carry 40 different taxa round-robin, so that windows hold
                 more taxa than a window lane keeps in LDS (16, bracken.hip: BR_MAPCAP) and the lane hands over to the HBM map."""
import numpy as np

import bracken_model as bm
import synth
import taxgen

MAPCAP = 16   # bracken.hip: BR_MAPCAP
CHUNK = 512   # bracken.hip: BR_CHUNK
GRID_LANES = 256 * 40 * 64   # bracken.hip: br_run_batch caps the window kernel's grid at 256 * 40 blocks of BR_BLOCK = 64 lanes
MIN_MAP_LOG2 = 10            # bracken.hip: the smallest (source, dest) map SLK_BRACKEN_MAP_LOG2 gives


def deficits(orc, p, index, piece, read_len, qt):
    """per read: true minus literal count of the quirk taxon"""
    lit = bm.literal_window_counts(orc, p, index, piece, read_len)
    pure = bm.window_counts_pure(orc, p, index, piece, read_len)
    return np.array([pure[q].get(qt, 0) - lit[q].get(qt, 0) for q in range(len(lit))])


def quirk_record(orc, p, index, g, read_len, length):
    """g[:length] with two Ns placed so that the reproduced quirk fires in the first piece; (record, qt, deficit per read)"""
    k = p.k
    W = read_len - (k - 1)
    best = None
    for a in range(k // 2, k - 1):              # a valid run shorter than k, then an N: the next segment starts at a + 1 > 0
        for end in range(W + k, W + k + 40):    # the segment ends just past the first window
            h = np.array(g[:length], np.uint8)
            h[a] = ord("N")
            h[end] = ord("N")
            rec = h.tobytes()
            _, _, _, _, qt, qe = bm.piece_arrays(orc, p, index, rec, read_len)
            if qt == 0:
                continue
            d = deficits(orc, p, index, rec, read_len, qt)
            if d.max() <= 0:
                continue
            if best is None or (d[CHUNK:CHUNK + 1].sum() > 0 and best[2][CHUNK:CHUNK + 1].sum() == 0):
                best = (rec, qt, d)
            if len(d) > CHUNK and d[CHUNK] > 0:
                return best
    return best


class ManyTaxa:
    """Two genomes: B (one taxon for all its records) and A (its records spread round-robin over 40 leaves).  A record
    B[:nb] + A[:na] starts with windows of few taxa and slides into windows of more than MAPCAP (the mid-slide hand-over);
    A on its own starts there (the hand-over while the first window is built).  quirk=True adds a record that starts with a quirk
    in its B part; with b_every > 0 B's taxon stays in the windows over A, so that the deficit can still be open at a hand-over."""

    def __init__(self, orc, p, seed, read_len, b_every=0):
        rng = np.random.default_rng(seed)
        self.p = p
        self.parents = taxgen.taxonomy(8 * 80, rng)
        taxa = np.array(taxgen.defined_taxa(self.parents))
        leaves = [int(t) for t in np.setdiff1d(taxa, self.parents[taxa])]
        assert len(leaves) >= 41
        self.tb, spread = leaves[0], leaves[1:41]
        A, B = synth.random_dna(6000, rng), synth.random_dna(6000, rng)
        bases = np.concatenate([A, B])
        off = np.array([0, len(A), len(A) + len(B)], np.uint64)
        keys, tx = orc.build_records(p, self.parents, bases, off, np.array([spread[0], self.tb], np.int32))
        a_keys = set(int(x) for x in orc.minimizer_keys(p, A.tobytes()))
        i = 0
        for r in range(len(keys)):   # b_every > 0: every b_every-th record of A keeps B's taxon (it stays in A's windows)
            if int(keys[r]) in a_keys:
                tx[r] = self.tb if b_every and i % b_every == 0 else spread[i % len(spread)]
                i += 1
        self.keys, self.rec_taxa = keys, tx
        self.index = orc.Index(1, keys, tx)
        self.A, self.B = A, B
        self.read_len = read_len

    def records(self, orc, quirk=False):
        L = self.read_len
        recs = [np.concatenate([self.B[:900], self.A[:1500]]).tobytes(),   # few taxa first, then many
                self.A[:1800].tobytes(),                                     # many taxa from the first window on
                np.concatenate([self.A[:700], self.B[:800], self.A[2000:3000]]).tobytes()]
        if quirk:   # the quirk in the B part, then A arrives while the deficit may still be open
            found = quirk_record(orc, self.p, self.index, np.concatenate([self.B[:700], self.A[3000:4500]]), L, 2200)
            assert found is not None
            recs.append(found[0])
        return recs

    def max_taxa(self, orc, rec):
        return max(len(c) for c in bm.window_counts_pure(orc, self.p, self.index, rec, self.read_len))
