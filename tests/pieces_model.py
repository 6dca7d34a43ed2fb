"""The rule between the pieces of a split fragment, stated in Python on top of the oracle.

A fragment's k-mer windows are cut into pieces of `piece_windows` windows (the last piece takes the rest); a piece's bases are its
windows plus k - 1.  Each piece is taken through the oracle as if it were a read of its own -- its spans, their taxa, the taxon map
-- and what looks across a border between two pieces is settled afterwards from what each piece saw at its two ends:

  * the first super-mer of a piece was counted as a distinct hit group although the last super-mer BEFORE it -- in the nearest
    earlier piece that has one, not necessarily the neighbour -- may carry the same key: then it is taken back (if it had a taxon:
    only those were counted);
  * a super-mer or an ambiguous span cut by a border was counted as two spans: it is one.

Everything else is additive over windows: the total of k-mers, the taxon map, the probes."""
import numpy as np

VALID = np.zeros(256, bool)
VALID[list(b"ACGTUacgtu")] = True


def cut(n_bases, k, piece_windows):
    """[(first base, bases)] of the pieces of a read of n_bases >= k bases"""
    nwin = n_bases - k + 1
    return [(w0, min(piece_windows, nwin - w0) + k - 1) for w0 in range(0, nwin, piece_windows)]


def piece_record(orc, p, oix, bases):
    """what one piece leaves behind: its two ends, its provisional counts, its taxon map"""
    k = p.k
    spans = orc.spans(p, bases.tobytes())
    ok = VALID[bases]
    rec = dict(has=False, first_key=None, last_key=None, first_nz=False,
               starts_seq=bool(ok[:k].all()), ends_open=bool(ok[-k:].all()),          # its first / last window is a k-mer of a sequence run
               first_amb=bool(not ok[:k].any()), end_amb=bool(not ok[-k:].any()),     # ... lies in an ambiguous span
               nd=0, n_out=len(spans), total=0, map={})
    for s in spans:
        rec["total"] += s["kmers"]
        if s["flag"] != 1:
            continue
        taxon = oix.lookup(s["key"])
        if not rec["has"]:
            rec.update(has=True, first_key=s["key"], first_nz=taxon != 0)
        rec["last_key"] = s["key"]
        rec["nd"] += 1 if (s["distinct"] and taxon != 0) else 0
        rec["map"][taxon] = rec["map"].get(taxon, 0) + s["kmers"]
    return rec


def merge(records):
    """the borders between pieces, then the sums: dict(num_distinct, num_hits, total_kmers, map)"""
    nd = n_out = total = 0
    tmap = {}
    last = None          # last key of the nearest earlier piece that has a super-mer
    prev = None
    for rec in records:
        nd += rec["nd"]
        n_out += rec["n_out"]
        total += rec["total"]
        for t, c in rec["map"].items():
            tmap[t] = tmap.get(t, 0) + c
        if rec["has"] and rec["first_nz"] and last is not None and last == rec["first_key"]:
            nd -= 1
        if prev is not None:
            cut_supermer = prev["ends_open"] and rec["starts_seq"] and prev["last_key"] == rec["first_key"]
            cut_ambiguous = prev["end_amb"] and rec["first_amb"]
            n_out -= 1 if (cut_supermer or cut_ambiguous) else 0
        if rec["has"]:
            last = rec["last_key"]
        prev = rec
    return dict(num_distinct=nd, num_hits=n_out, total_kmers=total, map=tmap)


def by_pieces(orc, p, oix, read, piece_windows):
    return merge([piece_record(orc, p, oix, read[a:a + n]) for a, n in cut(len(read), p.k, piece_windows)])


def whole(orc, p, oix, parents, read):
    """the same numbers from the oracle's run over the whole read"""
    res, hits = orc.classify_read(p, oix, parents, read.tobytes(), None, 2, 0.0)
    tmap = {}
    for t, c in hits:
        if t >= 0:
            tmap[t] = tmap.get(t, 0) + c
    return dict(num_distinct=res["num_distinct"], num_hits=res["num_hits"], total_kmers=res["total_kmers"], map=tmap)


# ---- inputs the CPU and the GPU tests of the piece route share -----------------------------------------------------------------
def library_with_repeats(orc, p, parents, rng, n_genomes=12, genome_len=30000, pad_records=20000):
    """A synthetic library whose records also cover low-complexity sequence, so that long super-mers with equal keys carry real taxa
    -> (synth.Library with .units, keys, taxa)"""
    import synth
    lib = synth.Library(orc, p, parents, n_genomes=n_genomes, genome_len=genome_len, pad_records=pad_records)
    units = [synth.random_dna(int(rng.integers(1, 7)), rng) for _ in range(24)] + [np.frombuffer(b"AC", np.uint8), np.frombuffer(b"ACGGT", np.uint8)]
    keys, taxa = [lib.keys], [lib.taxa]
    for u in units:
        kk = np.setdiff1d(np.unique(orc.minimizer_keys(p, np.tile(u, 40).tobytes())), np.concatenate(keys))
        keys.append(kk)
        taxa.append(np.full(len(kk), int(rng.choice(lib.genome_taxa)), np.int32))
    lib.units = units
    return lib, np.concatenate(keys), np.concatenate(taxa).astype(np.int32)


def long_read(lib, rng, length):
    """stretches of several genomes (several taxa per read) with substitutions, N runs shorter and longer than k, repeats whose
    windows share one minimizer for hundreds of bases, random sequence"""
    import synth
    parts, have = [], 0
    while have < length:
        kind = rng.random()
        if kind < 0.70:
            g = lib.genomes[rng.integers(0, len(lib.genomes))]
            n = int(rng.integers(100, 4000))
            a = int(rng.integers(0, len(g) - n))
            part = g[a:a + n].copy()
            if rng.random() < 0.5:
                part = synth.revcomp(part).copy()
            subs = rng.random(n) < 0.01
            part[subs] = synth.random_dna(int(subs.sum()), rng)
        elif kind < 0.80:
            part = np.full(int(rng.choice([1, 2, 5, 30, 34, 35, 36, 40, 64, 70, 100, 200])), ord("N"), np.uint8)
        elif kind < 0.90:
            part = np.tile(lib.units[rng.integers(0, len(lib.units))], int(rng.integers(20, 400)))
        else:
            part = synth.random_dna(int(rng.integers(10, 500)), rng)
        parts.append(part)
        have += len(part)
    return np.concatenate(parts)[:length].copy()
