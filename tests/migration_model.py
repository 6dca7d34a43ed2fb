"""Plain-Python model of `compareIndex` (S/slacken/analysis/MinimizerMigration.scala:33-85): the inner join of two libraries'
records on the minimizer, steps per pair, the text Dataset.show() prints for the histogram of steps, and the selection of taxa
whose minimizers went to ROOT / cellular organisms, as a Kraken report.  Every expected value of the migration tests comes from
here."""
import hostmodel

ROOT = 1
CELLULAR_ORGANISMS = 131567   # MinimizerMigration.scala:74


def join(subject, reference):
    """subject: iterable of (key, t1) records; reference: dict key -> t2.  Returns ({(t1, t2): records}, matched, unmatched).
    Records with t1 == 0 (NONE) are no records (slk_index_append skips them); a key the reference lacks leaves the join (:47)."""
    pairs, matched, unmatched = {}, 0, 0
    for key, t1 in subject:
        t1 = int(t1)
        if t1 == 0:
            continue
        t2 = reference.get(int(key), 0)
        if t2 == 0:
            unmatched += 1
            continue
        matched += 1
        pairs[(t1, int(t2))] = pairs.get((t1, int(t2)), 0) + 1
    return pairs, matched, unmatched


def depth(tax, t):
    """Taxonomy.depth of the reference's taxonomy; an id it does not have has depth -1 (the engine's rule; the reference throws)"""
    if tax is None or t < 0 or t >= len(tax.parents):
        return -1
    return hostmodel.depth(tax, t)


def steps(tax, t1, t2):
    """:51-64"""
    l1, l2 = depth(tax, t1), depth(tax, t2)
    return -100 if l1 == -1 else -200 if l2 == -1 else l1 - l2


def triples(pairs, tax, with_depths=True):
    """[(t1, t2, steps, count)] sorted by t1 then t2, as slk_migration_result gives them; steps 0 without depths"""
    return [(t1, t2, steps(tax, t1, t2) if with_depths else 0, c) for (t1, t2), c in sorted(pairs.items())]


def show(trip):
    """groupBy("steps").agg(count("steps")).sort("steps").show() (:70-72)"""
    hist = {}
    for _, _, s, c in trip:
        hist[s] = hist.get(s, 0) + c
    head = ("steps", "count(steps)")
    rows = [(str(s), str(hist[s])) for s in sorted(hist)]
    width = [max([3, len(head[c])] + [len(r[c]) for r in rows]) for c in range(2)]
    rule = "+" + "+".join("-" * w for w in width) + "+\n"
    line = lambda r: "|" + "|".join(r[c].rjust(width[c]) for c in range(2)) + "|\n"   # noqa: E731
    return rule + line(head) + rule + "".join(line(r) for r in rows) + rule + "\n"


def to_root(trip):
    """[(t1, records)] of the pairs that moved into {ROOT, cellular organisms} from outside it (:77-79)"""
    top = (ROOT, CELLULAR_ORGANISMS)
    out = {}
    for t1, t2, _, c in trip:
        if t2 in top and t1 not in top:
            out[t1] = out.get(t1, 0) + c
    return sorted(out.items())


def report(subject_tax, trip):
    """OUTPUT_taxaToRoot_report.txt: KrakenReport(index.bcTaxonomy, toRoot) (:81-83)"""
    lines, _, _ = hostmodel.kraken_report(subject_tax, to_root(trip))
    return "\n".join(lines) + "\n"
