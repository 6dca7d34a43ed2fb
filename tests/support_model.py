"""Plain-Python model of the sample support (S/slacken/Dynamic.scala:95-117, 152-180, 210-228): every SEQUENCE span of every read
(oracle.spans) is looked up in the records (oracle.Index.lookup), the hits whose taxon has depth >= min_depth are grouped by taxon
into the sum of their k-mers, their number and the number of different minimizers among them.  Also the text of the four files
`support` writes, through hostmodel.kraken_report.  Every expected value of the support tests comes from here."""
import hostmodel

SUFFIXES = ("totalKmerCount", "distinctMinimizerCount", "totalMinimizerCount", "classifiedReadCount")


def as_text(seq):
    return seq if isinstance(seq, str) else bytes(seq).decode("latin-1")


class Support:
    """add() reads (seq1, seq2 or None) in any number of calls; rows() and totals() at any time, for any min_depth"""

    def __init__(self, orc, p, index, depth_of):
        self.orc, self.p, self.index, self.depth_of = orc, p, index, depth_of
        self.hits = []                                   # (taxon, k-mers, key) of every SEQUENCE span the records hold
        self.sequences = self.supermers = 0

    def add(self, seq1, seq2=None):
        self.sequences += 1 if seq2 is None else 2
        for sp in self.orc.spans(self.p, as_text(seq1), None if seq2 is None else as_text(seq2)):
            if sp["flag"] != self.orc.SEQUENCE_FLAG:     # the mate-pair border and ambiguous spans carry no true taxon
                continue
            self.supermers += 1
            taxon = self.index.lookup(sp["key"])
            if taxon != 0:                               # a miss is NONE: never counted
                self.hits.append((taxon, sp["kmers"], sp["key"]))
        return self

    def add_all(self, reads):
        """reads: sequences, or (seq1, seq2) pairs"""
        for r in reads:
            if isinstance(r, tuple):
                self.add(*r)
            else:
                self.add(r)
        return self

    def rows(self, min_depth, want_distinct=True):
        """[(taxon, kmers, minimizers, distinct)] ascending by taxon"""
        kmers, minimizers, keys, depth = {}, {}, {}, {}
        for taxon, n, key in self.hits:
            if taxon not in depth:
                depth[taxon] = self.depth_of(taxon)
            if depth[taxon] < min_depth:
                continue
            kmers[taxon] = kmers.get(taxon, 0) + n
            minimizers[taxon] = minimizers.get(taxon, 0) + 1
            keys.setdefault(taxon, set()).add(key)
        return [(t, kmers[t], minimizers[t], len(keys[t]) if want_distinct else 0) for t in sorted(kmers)]

    def totals(self, min_depth):
        """(sequences, SEQUENCE super-mers, those the records hold, those that passed min_depth)"""
        return (self.sequences, self.supermers, len(self.hits), sum(r[2] for r in self.rows(min_depth)))


def support(orc, p, index, depth_of, reads):
    return Support(orc, p, index, depth_of).add_all(reads)


def report_text(tax, counts):
    """KrakenReport.print of (taxon, value) pairs, as the files hold it"""
    return "\n".join(hostmodel.kraken_report(tax, counts)[0]) + "\n"


def report_texts(tax, rows, classified):
    """the four texts of Dynamic.reportDynamicIndexSupport (:210-228) by file suffix; classified: [(taxon, classified reads)]"""
    columns = {"totalKmerCount": 1, "totalMinimizerCount": 2, "distinctMinimizerCount": 3}
    out = {name: report_text(tax, [(r[0], r[col]) for r in rows]) for name, col in columns.items()}
    out["classifiedReadCount"] = report_text(tax, sorted(classified))
    return out
