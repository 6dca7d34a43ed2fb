"""Plain-Python model of what `stats` and `inspect` print without a genome library, restated line by line from the Scala:
KeyValueIndex.showIndexStats(None) (S/slacken/KeyValueIndex.scala:240-251), kmerDepthHistogram / taxonDepthHistogram (:326-336) as
Dataset.show() prints them, and report(labels, output, None) (:274-306).  Every function takes the taxonomy (hostmodel.Taxonomy)
and `counts`, a list of (taxon, records) with distinct taxa -- records.groupBy("taxon").agg(count("*")).  Every expected value of
the statistics tests comes from here."""
from decimal import Decimal, ROUND_HALF_UP

import hostmodel

RANK_VALUES = hostmodel.RANKS[1:]   # Taxonomy.rankValues (Taxonomy.scala:51): root .. species, depth 0 .. 8; no "unclassified"


def in_tax(tax, t):
    return 0 <= t < len(tax.parents)


def depth(tax, t):
    """Taxonomy.depth (:217-224); an id outside the arrays has depth -1 (the engine's rule; the reference throws)"""
    return hostmodel.depth(tax, t) if in_tax(tax, t) else -1


def is_leaf(tax, t):
    """Taxonomy.isLeafNode (:171-172): children(taxon).isEmpty"""
    return not in_tax(tax, t) or not tax.children[t]


def taxa_with_ancestors(tax, taxa):
    """Taxonomy.taxaWithAncestors (:307-311): set ++= pathToRoot(a).takeWhile(e => !set.contains(e))"""
    seen = set()
    for a in taxa:
        t = a
        while t != 0 and t not in seen:     # pathToRoot (:204-215) ends at NONE
            seen.add(t)
            t = tax.parents[t] if in_tax(tax, t) else 0
    return seen


def format_perc(d):
    """formatPerc (S/kmers/package.scala:60): "%.2f%%".format(d * 100); java.util.Formatter rounds the shortest digits HALF_UP"""
    if d != d:
        return "NaN%"
    return str(Decimal(repr(float(d * 100))).quantize(Decimal("0.01"), rounding=ROUND_HALF_UP)) + "%"


def div(a, b):
    """Scala's Double division: 0.0 / 0 is NaN"""
    return a / b if b else float("nan")


def index_stats(tax, counts, m):
    """showIndexStats(None) (:240-251)"""
    all_taxa = list(counts)
    leaf_taxa = [x for x in all_taxa if is_leaf(tax, x[0])]
    tree_size = len(taxa_with_ancestors(tax, [x[0] for x in all_taxa]))
    rec_total = sum(x[1] for x in all_taxa)
    leaf_total = sum(x[1] for x in leaf_taxa)
    return (f"Tree size: {tree_size} taxa, stored taxa: {len(all_taxa)}, of which {len(leaf_taxa)} "
            f"leaf taxa ({format_perc(div(float(len(leaf_taxa)), len(all_taxa)))})\n"
            f"Total {m}-minimizers: {rec_total}, of which leaf records: {leaf_total} ({format_perc(div(float(leaf_total), rec_total))})\n")


def show(head, rows):
    """Dataset.show(): numRows = 20, truncate = 20 (neither applies to these tables): cells right-aligned, columns as wide as their
    widest cell and at least 3"""
    assert len(rows) <= 20 and all(len(c) <= 20 for r in rows for c in r)
    width = [max([3, len(head[c])] + [len(r[c]) for r in rows]) for c in range(len(head))]
    rule = "+" + "+".join("-" * w for w in width) + "+\n"
    line = lambda r: "|" + "|".join(r[c].rjust(width[c]) for c in range(len(head))) + "|\n"   # noqa: E731
    return rule + line(head) + rule + "".join(line(r) for r in rows) + rule + "\n"


def rank_of_depth(d):
    """numericalRankToStrUdf (GenomeLibrary.scala:63-65)"""
    return next((RANK_VALUES[i] for i in range(len(RANK_VALUES)) if i == d), "???")


def depth_histogram(tax, counts, by_records):
    """kmerDepthHistogram (one row per record, :326-330) / taxonDepthHistogram (one row per distinct taxon, :332-336):
    groupBy("depth").count().sort("depth"), then rank, select("depth", "rank", "count")"""
    hist = {}
    for t, c in counts:
        d = depth(tax, t)
        hist[d] = hist.get(d, 0) + (c if by_records else 1)
    return show(("depth", "rank", "count"), [(str(d), rank_of_depth(d), str(hist[d])) for d in sorted(hist)])


def stats(tax, counts, m, histogram):
    """what Slacken.scala:304-312 prints after the splitter lines"""
    if not histogram:
        return index_stats(tax, counts, m)
    return ("Minimizer depth histogram\n" + depth_histogram(tax, counts, True) +
            "Taxon depth histogram\n" + depth_histogram(tax, counts, False))


def report_text(tax, counts):
    """new KrakenReport(taxonomy, counts).print; without counts 100.0 * 0 / 0 is NaN, which "%6.2f" prints as "   NaN" """
    if not counts:
        return "#Perc\tAggregate\tIn taxon\tRank\tTaxon\tName\n   NaN\t0\t0\tR\t1\t" + (tax.names[1] or "") + "\n"
    lines, _, _ = hostmodel.kraken_report(tax, counts)
    return "\n".join(lines) + "\n"


def label_taxa(text):
    """GenomeLibrary.getTaxonLabels(labels).select("_2").distinct() (:74-78)"""
    out = set()
    for line in text.split("\n"):
        cols = line.split("\t")
        if len(cols) >= 2 and cols[1].strip().isdigit():
            out.add(int(cols[1]))
    return out


def reports(tax, counts, labels_text=None):
    """report(labels, output, None) (:274-306): {file suffix: text}"""
    all_taxa = list(counts)
    out = {"_min_report.txt": report_text(tax, all_taxa),
           "_genome_report.txt": report_text(tax, [(t, 1) for t, _ in all_taxa])}
    if labels_text is not None:
        present = {t for t, _ in all_taxa}
        missing = sorted(label_taxa(labels_text) - present)        # BitSet: ascending
        out["_missing_report.txt"] = report_text(tax, [(t, 1) for t in missing])
    return out
