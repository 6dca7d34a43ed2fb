"""Bracken weights restated on the CPU oracle (BrackenWeights.scala, S/ = the reference's src/main/scala/com/jnpersson/).

literal()  taxonHits + FragmentWindow + readClassifications + splitToMaxLength restated line by line
           (S/slacken/BrackenWeights.scala:46-137,152-164,198-233,251-285), on the oracle's split_by_ambiguity, split_encode,
           Index.lookup and resolve_tree.  Slow: one Python step per read.
fast()     the same counts from per-k-mer arrays (numpy): true window counts, except that the one taxon whose k-mers
           [W, t0) a wrong trailing-hit ordinal (:230) credits to NONE follows c <- max(c - dec, 0) + inc.

Both return {(dest, source): reads}.  Records are bytes without whitespace; sources their taxa.  Test infrastructure."""
import numpy as np

NONE = 0
SEQUENCE_FLAG = 1


def split_to_max_length(seq, max_len, read_len):
    """TaxonFragment.splitToMaxLength(max, k = readLen) (:152-164)."""
    if len(seq) <= max_len:
        return [seq]
    return [seq[s:min(s + max_len, len(seq))] for s in range(0, len(seq) - read_len + 1, max_len - (read_len - 1))]


def taxon_hits(orc, p, index, seq, k):
    """TaxonFragment.taxonHits (:198-233): [(distinct, ordinal, taxon, count)], the trailing hit's ordinal as the reference has it."""
    hits = []
    first, last = True, None
    for pos, ln, flag in orc.split_by_ambiguity(seq, k):
        sub = seq[pos:pos + ln]
        if flag == SEQUENCE_FLAG:
            for key, start, length in orc.split_encode(p, sub):
                distinct = first or key != last                         # :218
                first, last = False, key
                hits.append((distinct, start + pos, index.lookup(key), length - (k - 1)))
            hits.append((False, ln - (k - 1), NONE, k - 1))            # :230 (no `pos`)
        else:
            hits.append((False, pos, NONE, ln))                          # :232-235
    return hits


def fragment_window_dests(hits, W, n_reads, resolve, min_hit_groups=2):
    """FragmentWindow (:46-137) driven by readClassifications (:251-268) and classify (:276-285)."""
    window_start, window_end = 0, W
    i = 0
    cur = []
    while i < len(hits) and hits[i][1] < window_end:                    # hits.span(inWindow) (:76-80)
        cur.append(hits[i])
        i += 1
    num_hit_groups = sum(1 for h in cur if h[0] and h[2] != NONE)       # :84-90
    last = cur[-1]                                                       # :92
    counts = {}                                                          # Int2IntArrayMap (:59)
    for h in cur:                                                        # :94-100
        for ks in range(h[1], h[1] + h[3]):
            if window_start <= ks < window_end:
                counts[h[2]] = counts.get(h[2], 0) + 1
    out = []
    for start in range(n_reads):
        if start > 0:                                                    # advance() (:104-136)
            remove = cur[0]
            updated = counts.get(remove[2], 0) - 1
            if updated > 0:
                counts[remove[2]] = updated
            else:
                counts.pop(remove[2], None)
            window_start += 1
            window_end += 1
            if cur[0][1] + (cur[0][3] - 1) < window_start:               # passedWindow (:72-73)
                cur.pop(0)
                if remove[0] and remove[2] != NONE:
                    num_hit_groups -= 1
            if last[1] + last[3] < window_end and i < len(hits):
                add = hits[i]
                i += 1
                cur.append(add)
                last = add
                if add[0] and add[2] != NONE:
                    num_hit_groups += 1
            counts[last[2]] = counts.get(last[2], 0) + 1
        out.append(resolve(counts) if num_hit_groups >= min_hit_groups else NONE)
    return out


def _resolver(orc, parents):
    cache = {}

    def resolve(counts):   # resolveTree(summary, 0.0), the NONE key included (it scores 0)
        key = tuple(sorted(counts.items()))
        if key not in cache:
            cache[key] = orc.resolve_tree(parents, list(counts.keys()), list(counts.values()), 0.0)
        return cache[key]
    return resolve


def literal(orc, p, index, parents, records, sources, read_len, max_fragment=1024 * 1024):
    k = p.k
    W = read_len - (k - 1)
    resolve = _resolver(orc, parents)
    out = {}
    for seq, src in zip(records, sources):
        for piece in split_to_max_length(bytes(seq), max_fragment, read_len):
            n_reads = len(piece) - read_len + 1
            if n_reads <= 0:
                continue
            for d in fragment_window_dests(taxon_hits(orc, p, index, piece, k), W, n_reads, resolve):
                out[(d, src)] = out.get((d, src), 0) + 1
    return out


def piece_arrays(orc, p, index, piece, read_len):
    """Per k-mer position: taxon, hit-group start / member / end flags; and the quirk (taxon, t0) or (0, 0)."""
    k = p.k
    W = read_len - (k - 1)
    n = len(piece)
    tax = np.zeros(n, np.int64)
    start = np.zeros(n, bool)
    member = np.zeros(n, bool)
    end = np.zeros(n, bool)
    qt, qe = 0, 0
    first, last = True, None
    for pos, ln, flag in orc.split_by_ambiguity(piece, k):
        if flag != SEQUENCE_FLAG:
            continue
        last_tax, last_start = 0, pos
        for key, s, length in orc.split_encode(p, piece[pos:pos + ln]):
            c = length - (k - 1)
            a = pos + s
            t = index.lookup(key)
            distinct = first or key != last
            first, last = False, key
            tax[a:a + c] = t
            if distinct and t != NONE:
                member[a:a + c] = True
                start[a] = True
                end[a + c - 1] = True
            last_tax, last_start = t, a
        t0 = pos + ln - (k - 1)
        if pos > 0 and last_start < W and t0 > W and t0 - pos < W:
            qt, qe = last_tax, t0
    return tax, start, member, end, qt, qe


def fast(orc, p, index, parents, records, sources, read_len, max_fragment=1024 * 1024):
    k = p.k
    W = read_len - (k - 1)
    resolve = _resolver(orc, parents)
    out = {}
    for seq, src in zip(records, sources):
        for piece in split_to_max_length(bytes(seq), max_fragment, read_len):
            nr = len(piece) - read_len + 1
            if nr <= 0:
                continue
            tax, start, member, end, qt, qe = piece_arrays(orc, p, index, piece, read_len)
            taxa = [t for t in np.unique(tax) if t != NONE]
            cnt = np.zeros((nr, len(taxa)), np.int64)
            for j, t in enumerate(taxa):
                cs = np.concatenate([[0], np.cumsum(tax == t)])
                cnt[:, j] = cs[W:W + nr] - cs[:nr]
            if qt != NONE:   # the literal count of qt: c <- max(c - dec, 0) + inc, the stolen k-mers entering as NONE
                j = taxa.index(qt)
                c = int(cnt[0, j])
                for q in range(1, nr):
                    dec = tax[q - 1] == qt
                    inc = tax[q - 1 + W] == qt and not (q - 1 + W < qe)
                    c = max(c - int(dec), 0) + int(inc)
                    cnt[q, j] = c
            cs = np.concatenate([[0], np.cumsum(start)])
            hg = cs[W:W + nr] - cs[:nr] + (member[:nr] & ~start[:nr])
            dest = np.zeros(nr, np.int64)
            if taxa:
                rows, inv = np.unique(cnt, axis=0, return_inverse=True)
                inv = np.asarray(inv).reshape(-1)
                dest_of_row = np.array([resolve({t: int(c) for t, c in zip(taxa, row) if c > 0}) for row in rows], np.int64)
                dest = dest_of_row[inv]
            dest = np.where(hg >= 2, dest, NONE)
            ds, cs_ = np.unique(dest, return_counts=True)
            for d, c in zip(ds, cs_):
                out[(int(d), src)] = out.get((int(d), src), 0) + int(c)
    return out


def window_counts_pure(orc, p, index, piece, read_len):
    """The per-read true window counts ({taxon: k-mers}, NONE left out): what the reads would see without the quirk."""
    tax, _, _, _, _, _ = piece_arrays(orc, p, index, piece, read_len)
    W = read_len - (p.k - 1)
    res = []
    for q in range(len(piece) - read_len + 1):
        ts, cs = np.unique(tax[q:q + W], return_counts=True)
        res.append({int(t): int(c) for t, c in zip(ts, cs) if t != NONE})
    return res


def literal_window_counts(orc, p, index, piece, read_len):
    """The literal FragmentWindow's countSummary per read, NONE left out."""
    k = p.k
    W = read_len - (k - 1)
    res = []

    def grab(counts):
        res.append({t: c for t, c in counts.items() if t != NONE})
        return NONE
    fragment_window_dests(taxon_hits(orc, p, index, piece, k), W, len(piece) - read_len + 1, grab, min_hit_groups=0)
    return res


def to_arrays(d):
    """{(dest, source): n} -> (dest, source, count) sorted by dest then source (slk_bracken_result's order)."""
    items = sorted(d.items())
    return (np.array([a for (a, _), _ in items], np.int32), np.array([b for (_, b), _ in items], np.int32),
            np.array([c for _, c in items], np.uint64))
