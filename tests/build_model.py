"""Plain-Python model of what `build` prints after the index statistics: GenomeLibrary.inputStats (S/slacken/GenomeLibrary.scala:81-107)
restated line by line, on stats_model.py (leaves, implied tree, Dataset.show()) and hostmodel.py (the taxonomy, depths)."""
import stats_model as sm


def is_defined(tax, t):
    """Taxonomy.isDefined (:175-176); an id outside the arrays is undefined (the engine's rule; the reference throws)"""
    return sm.in_tax(tax, t) and (tax.parents[t] != 0 or t == 1)


def missing_steps_to_root(tax, t):
    """Taxonomy.missingStepsToRoot (:300-304): the levels superkingdom (1) .. species (8) that no depth on the path to the root has"""
    found = set()
    while t != 0 and sm.in_tax(tax, t):
        found.add(sm.depth(tax, t))
        t = tax.parents[t]
    return [level for level in range(1, 9) if level not in found]


def read_labels(path):
    """GenomeLibrary.getTaxonLabels (:74-78): (sequence id, taxon) per line"""
    out = []
    for line in open(path).read().split("\n"):
        cols = line.split("\t")
        if len(cols) >= 2:
            out.append((cols[0], int(cols[1])))
    return out


def splitter_line(k=35, m=31, spaces=7, mask=None):
    """the first line `build` prints: the parameters in the engine's words (a recorded deviation from the Scala object's toString)"""
    from slacken_amd import capi
    mask = capi.DEFAULT_TOGGLE_MASK if mask is None else mask
    mask = mask - (1 << 64) if mask >> 63 else mask
    return f"Splitter randomXOR k={k} m={m} XORmask={mask} canonical=true minimizerSpaces={spaces}\n"


def input_stats(label_file, labels, tax):
    labelled = sorted({t for _, t in labels})                               # select("_c1").distinct()
    invalid = [x for x in labelled if not is_defined(tax, x)]
    out = ""
    if invalid:
        out += f"{len(invalid)} unknown genomes in {label_file} were not indexed (missing from the taxonomy):\n"
        out += "List(" + ", ".join(map(str, invalid)) + ")\n"
    non_leaf = [x for x in labelled if not sm.is_leaf(tax, x)]
    if non_leaf:
        out += f"{len(non_leaf)} non-leaf genomes in {label_file}\n"
    valid = [x for x in labelled if is_defined(tax, x)]
    biggest = len(sm.taxa_with_ancestors(tax, valid))
    out += f"{len(valid)} valid taxa in input sequences described by {label_file} (maximal implied tree size {biggest})\n"
    out += f"Max leaf nodes in resulting database: {len(valid) - len(non_leaf)}\n"
    hist = {}
    for x in valid:
        for level in missing_steps_to_root(tax, x):
            hist[level] = hist.get(level, 0) + 1
    rows = [(str(level), str(hist[level]), sm.rank_of_depth(level)) for level in sorted(hist)]
    return out + sm.show(("missingLevel", "count(missingLevel)", "label"), rows)
