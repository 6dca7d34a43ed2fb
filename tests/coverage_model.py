"""Plain-Python model of the genome coverage (S/slacken/IndexStatistics.scala:38-52, 86-222): the (source, depth) rows of
showTaxonFullCoverageStats from the oracle's super-mers and lookups, the k-mers per source taxon, TotalKmerSizeAggregator with the
three TKC columns, and the text of the three files `coverage` writes.  Every expected value of the coverage tests comes from here."""
import math

import numpy as np

import hostmodel

VALID = frozenset(b"ACGTUacgtu")


def segments(seq):
    """the maximal runs of nucleotides (InputReader.removeInvalid): [(start, length)]"""
    out, start = [], None
    for i, ch in enumerate(seq):
        if ch in VALID:
            if start is None:
                start = i
        elif start is not None:
            out.append((start, i - start))
            start = None
    if start is not None:
        out.append((start, len(seq) - start))
    return out


def kmers(seq, k):
    """sum over the super-mers of length - (k - 1) (:45-46) = the windows of the valid segments"""
    return sum(max(0, n - k + 1) for _, n in segments(seq))


def window_minimizers(orc, p, seq):
    """the minimizer of every window of a sequence WITHOUT invalid characters, by window start (from the super-mers)"""
    out = []
    for key, _, length in orc.split_encode(p, seq):
        out += [key[0]] * (length - p.k + 1)
    return out


def as_bytes(seq):
    return seq if isinstance(seq, bytes) else bytes(seq) if not isinstance(seq, str) else seq.encode()


def coverage(orc, p, index, depth_of, seqs, sources, groups=None):
    """seqs[i] (bytes) came from taxon sources[i]; index: oracle.Index of the records; depth_of(taxon) -> depth.
    groups: None, or a list of sets of sources folded one after the other.  Returns
      rows    [(source, depth, all, distinct)] sorted by source then depth
      totals  [(source, k-mers, super-mers)] sorted by source
      misses  super-mers whose minimizer the index lacks"""
    pairs, totals, misses = {}, {}, 0        # (group, minimizer, source) -> countAll
    group_of = {}
    for g, members in enumerate(groups or []):
        for s in members:
            group_of[s] = g
    for seq, src in zip(seqs, sources):
        src = int(src)
        if src == 0:
            continue
        seq = as_bytes(seq)
        mins = orc.library_minimizers(p, seq).tolist()
        t = totals.setdefault(src, [0, 0])
        t[0] += kmers(seq, p.k)
        t[1] += len(mins)
        for key in mins:
            pairs[(group_of.get(src, 0), key, src)] = pairs.get((group_of.get(src, 0), key, src), 0) + 1
    rows = {}
    for (_, key, src), count_all in pairs.items():
        taxon = index.lookup([key])
        if taxon == 0:                       # the inner join (:99-100)
            misses += count_all
            continue
        r = rows.setdefault((src, depth_of(taxon)), [0, 0])
        r[0] += count_all
        r[1] += 1
    return ([(s, d, a, n) for (s, d), (a, n) in sorted(rows.items())], [(s, k, n) for s, (k, n) in sorted(totals.items())], misses)


def coverage_lines(rows):
    """(minimizerCoverage text, minimizerDistinctCoverage text): "<taxon>  <d>:<c>|<d>:<c>", sources and depths ascending"""
    by = {}
    for s, d, a, n in rows:
        by.setdefault(s, []).append((d, a, n))
    all_text = "".join(f"{s}  " + "|".join(f"{d}:{a}" for d, a, _ in by[s]) + "\n" for s in sorted(by))
    distinct_text = "".join(f"{s}  " + "|".join(f"{d}:{n}" for d, _, n in by[s]) + "\n" for s in sorted(by))
    return all_text, distinct_text


def java_round(x):
    """java.lang.Math.round(double): floor(x + 1/2), NaN -> 0"""
    if math.isnan(x):
        return 0
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def _div(a, b):
    """Scala's Double division: 0.0 / 0.0 is NaN, not an error"""
    a, b = float(a), float(b)
    if b == 0.0:
        return math.nan if a == 0.0 else math.copysign(math.inf, a)
    return a / b


class TotalKmerSizeAggregator:
    """:130-222, line by line.  tax: hostmodel.Taxonomy (children in descending id order, as the reference builds them)"""

    def __init__(self, tax, genome_sizes):
        self.tax, self.sizes, self.tree = tax, dict(genome_sizes), {}
        self._compute(1)

    def _compute(self, taxon):           # computeLeafAggAndCounts :193-219
        size = count = 0
        if taxon in self.sizes:
            size, count = self.sizes[taxon], 1
        for c in self.tax.children[taxon]:
            s, n = self._compute(c)
            size, count = size + s, count + n
        self.tree[taxon] = (size, count)
        return size, count

    def s1(self, taxon):                 # :140-148
        kids = [self.tree[c] for c in self.tax.children[taxon]]
        agg = (sum(a for a, _ in kids), sum(b for _, b in kids)) if kids else self.tree[taxon]
        if taxon in self.sizes:
            agg = (agg[0] + self.sizes[taxon], agg[1] + 1)
        return _div(agg[0], agg[1])

    def s2(self, taxon):                 # :156-167
        if self.tax.children[taxon]:
            avgs = [float(a) / float(b) for a, b in (self.tree[c] for c in self.tax.children[taxon]) if b > 0]
            if taxon in self.sizes:
                avgs = [float(self.sizes[taxon])] + avgs
            total = 0.0
            for v in avgs:               # List.sum: from the left
                total += v
            return _div(total, len(avgs))
        a, b = self.tree[taxon]
        return 0.0 if b == 0 else float(a) / float(b)

    def s3(self, taxon):                 # :175-185
        nonzero = [self.tree[c] for c in self.tax.children[taxon] if self.tree[c][1] > 0]
        agg = (sum(a for a, _ in nonzero), sum(b for _, b in nonzero)) if nonzero else self.tree[taxon]
        nz = float(len(nonzero))
        if agg[1] + nz == 0:
            return 0.0
        return ((self.s1(taxon) * float(agg[1])) + (self.s2(taxon) * nz)) / (float(agg[1]) + nz)

    def columns(self, taxon):
        return [self.s1(taxon), self.s2(taxon), self.s3(taxon)]


def min_report(tax, records, genome_sizes):
    """TotalKmerCountReport.print (:114-128): KrakenReport of the records per taxon with the three TKC columns behind "In taxon" """
    lines, _, _ = hostmodel.kraken_report(tax, records)
    agg = TotalKmerSizeAggregator(tax, genome_sizes)
    out = []
    for i, line in enumerate(lines):
        cols = line.split("\t")
        if i == 0:
            extra = ["TKC1-LeafOnly", "TKC2-FirstChildren", "TKC3-AllChildren"]
        else:
            extra = [str(java_round(v)) for v in agg.columns(int(cols[4]))]
        out.append("\t".join(cols[:3] + extra + cols[3:]))
    return "\n".join(out) + "\n"


def tie_distance(tax, records, genome_sizes):
    """how close any average a report of these inputs prints comes to a .5 tie (the tests keep their inputs away from it)"""
    lines, _, _ = hostmodel.kraken_report(tax, records)
    agg = TotalKmerSizeAggregator(tax, genome_sizes)
    best = 1.0
    for line in lines[1:]:
        for v in agg.columns(int(line.split("\t")[4])):
            if not math.isnan(v):
                best = min(best, abs((v - math.floor(v)) - 0.5))
    return best


def pack(seqs):
    """(bases uint8, offsets uint64) of a list of byte strings"""
    seqs = [as_bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return np.frombuffer(b"".join(seqs), np.uint8), offsets
