"""`compare`, restated with dicts and sets: the contract of MappingComparison (S/slacken/analysis/MappingComparison.scala) and the
command around it (S/slacken/Slacken.scala:343-366), with the Taxonomy methods it uses (S/slacken/Taxonomy.scala).  The yardstick of
slacken_amd/host/compare.hpp, `slacken-amd compare` and the slk_compare_* join on the device.  Nothing here is fast.

Deviations from the reference: a line with too few columns, an empty id or taxon field or a taxon that is no
non-negative Java int is an error naming the line (the reference throws); a taxon outside [0, T) among the reference rows or the
joined rows is an error; an id twice among the kept reference rows (after the "/2" rows are dropped, BEFORE the taxonomy's filter) or
twice among the test rows that match such a row is an error (Spark's join would multiply the rows)."""
import bz2
import gzip
import math
import os
import re
from decimal import ROUND_HALF_UP, Decimal

NONE, ROOT = 0, 1
RANK_DEPTH = {"unclassified": -1, "root": 0, "superkingdom": 1, "kingdom": 2, "phylum": 3, "class": 4, "order": 5, "family": 6, "genus": 7,
              "species": 8}                                        # Taxonomy.scala:39-48
GENUS, SPECIES = ("Genus", 7), ("Species", 8)
MIN_COUNT_TAXON = 10                                               # Slacken.scala:358
BAD_LINE, DUPLICATE_REFERENCE, DUPLICATE_TEST, TAXON_RANGE = 1, 2, 3, 4


class CompareError(Exception):
    def __init__(self, kind, offset, what):
        super().__init__(f"kind {kind} at byte {offset}: {what}")
        self.kind, self.offset, self.what = kind, offset, what


class Taxonomy:
    """Taxonomy.fromNodesAndNames :81-109: nodes = (taxon, parent, rank title), merged = (secondary, primary)"""

    def __init__(self, nodes, merged=()):
        n = max([t + 1 for t, _, _ in nodes] + [s + 1 for s, _ in merged] + [2])
        self.parents = [NONE] * n
        self.ranks = [None] * n                                    # a depth, or None where the title is no standard rank
        for t, p, title in nodes:
            self.parents[t] = p
            self.ranks[t] = RANK_DEPTH.get(title)
        self.primary = list(range(n))
        for s, p in merged:
            self.primary[s] = p
        self.parents[ROOT] = NONE
        self.ranks[NONE] = -1
        self.ranks[ROOT] = 0

    @classmethod
    def load(cls, d):                                              # Taxonomy.load :116-137
        nodes = [tuple(x.strip() for x in line.split("|")[:3]) for line in open(os.path.join(d, "nodes.dmp")) if line.strip()]
        merged = []
        if os.path.exists(os.path.join(d, "merged.dmp")):
            merged = [tuple(int(x.strip()) for x in line.split("|")[:2]) for line in open(os.path.join(d, "merged.dmp")) if line.strip()]
        return cls([(int(a), int(b), c) for a, b, c in nodes], merged)

    @property
    def size(self):
        return len(self.parents)

    def is_defined(self, t):                                       # :175-176
        return self.parents[t] != NONE or t == ROOT

    def path_to_root(self, t):                                     # :204-215 (an id that is not defined: just itself)
        out = []
        while t != NONE:
            out.append(t)
            t = self.parents[t]
        return out

    def depth(self, t):                                            # :222-228
        while True:
            if t == NONE:
                return -1
            if self.ranks[t] is not None:
                return self.ranks[t]
            t = self.parents[t]

    def steps_to_ancestor(self, t, a):                             # :241-244
        path = self.path_to_root(t)
        return path.index(a) if a in path else -1

    def has_ancestor(self, t, a):                                  # :236-237
        return self.steps_to_ancestor(t, a) != -1

    def standard_steps_to_ancestor(self, t, a):                    # :248-254
        return self.depth(t) - self.depth(a) if self.has_ancestor(t, a) else -1

    def standard_ancestor_at_level(self, t, rank_depth):           # :276-279; None where there is none
        below = []
        for x in self.path_to_root(t):
            if self.depth(x) < rank_depth:
                break
            below.append(x)
        return below[-1] if below else None

    def taxa_with_ancestors(self, taxa):                           # :307-310
        out = set()
        for a in taxa:
            for e in self.path_to_root(a):
                if e in out:
                    break
                out.add(e)
        return out


# ---- hitCategory :313-331 -------------------------------------------------------------------------------------------------------
def hit_category(tax, ref, test, rank_depth):
    """-> (class, index): ("TruePos", 0), ("VaguePos", steps), ("FalseNeg", 9), ("FalsePos", 9)"""
    if test == NONE:
        return ("FalseNeg", 9)
    anc = tax.standard_ancestor_at_level(ref, rank_depth) if rank_depth is not None else None
    ref_ancestor = anc if anc is not None else ref
    if ref == test:
        return ("TruePos", 0)
    if ref_ancestor != ROOT and tax.has_ancestor(test, ref_ancestor):
        return ("TruePos", 0)
    if ref_ancestor == ROOT or tax.has_ancestor(ref, test):
        return ("VaguePos", tax.standard_steps_to_ancestor(ref, test))
    if test == ROOT:
        return ("VaguePos", tax.standard_steps_to_ancestor(ref, test))
    return ("FalsePos", 9)


# ---- text -----------------------------------------------------------------------------------------------------------------------
def lines_of(data):
    """(byte offset, line) of every non-empty line; lines end with \\n, \\r\\n or a lone \\r"""
    out, i, n = [], 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] not in (10, 13):
            j += 1
        if j > i:
            out.append((i, data[i:j]))
        i = j + 2 if data[j:j + 2] == b"\r\n" else j + 1
    return out


def java_int(field):
    """Integer.parseInt: an optional sign and ASCII digits, inside the range of an int; None otherwise"""
    if not re.fullmatch(rb"[+-]?[0-9]+", field):
        return None
    v = int(field)
    return v if -2**31 <= v < 2**31 else None


def fields_of(offset, line, id_col, taxon_col):
    """(id, raw taxon) of a line, columns counted from 1, split at TAB only"""
    f = line.split(b"\t")
    if len(f) < max(id_col, taxon_col) or not f[id_col - 1] or not f[taxon_col - 1]:
        raise CompareError(BAD_LINE, offset, "too few columns or an empty field")
    t = java_int(f[taxon_col - 1])
    if t is None or t < 0:
        raise CompareError(BAD_LINE, offset, "the taxon is no non-negative int")
    return f[id_col - 1], t


def reference_rows(data, id_col=2, taxon_col=3, header=False):
    """readCustomFormat :265-274 without the taxonomy: {normalised id: raw taxon} of the kept rows, and (rows read, rows dropped as "/2").
    --header drops the first non-empty line."""
    rows, read, dropped = {}, 0, 0
    lines = lines_of(data)
    for offset, line in lines[1:] if header else lines:
        rid, taxon = fields_of(offset, line, id_col, taxon_col)
        read += 1
        if b"/2" in rid:
            dropped += 1
            continue
        rid = rid.replace(b"/1", b"")                              # replaceAll: every occurrence, one pass from the left
        if rid in rows:
            raise CompareError(DUPLICATE_REFERENCE, offset, rid.decode(errors="replace"))
        rows[rid] = taxon
    return rows, (read, dropped)


def kraken_rows(data):
    """readKrakenFormat :259-263 without the taxonomy: [(offset, id as it is, raw taxon)]"""
    return [(offset,) + fields_of(offset, line, 2, 3) for offset, line in lines_of(data)]


def join(rows, tests):
    """the device's part of the work: ({(raw ref taxon, raw test taxon): joined rows}, {raw ref taxon: kept rows}, test rows, joined rows)"""
    pairs, seen = {}, set()
    for offset, tid, taxon in tests:
        if tid in rows:
            if tid in seen:
                raise CompareError(DUPLICATE_TEST, offset, tid.decode(errors="replace"))
            seen.add(tid)
            key = (rows[tid], taxon)
            pairs[key] = pairs.get(key, 0) + 1
    ref_taxa = {}
    for t in rows.values():
        ref_taxa[t] = ref_taxa.get(t, 0) + 1
    return pairs, ref_taxa, len(tests), sum(pairs.values())


# ---- numbers as Java prints them ------------------------------------------------------------------------------------------------
def java_double(x):
    """Double.toString: the shortest digits that identify the double; plain from 1e-3 up to 1e7, E notation outside"""
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    if x == 0:
        return sign + "0.0"
    _, digits, exp = Decimal(repr(abs(x))).as_tuple()
    d = "".join(map(str, digits)).rstrip("0") or "0"
    e10 = len(digits) + exp - 1                                    # the exponent of d[0].d[1:]
    if 1e-3 <= abs(x) < 1e7:
        if e10 >= 0:
            whole, frac = d[:e10 + 1].ljust(e10 + 1, "0"), d[e10 + 1:]
        else:
            whole, frac = "0", "0" * (-e10 - 1) + d
        return f"{sign}{whole}.{frac or '0'}"
    return f"{sign}{d[0]}.{d[1:] or '0'}E{e10}"


def format_perc(x):
    """Helpers.formatPerc: "%.2f%%".format(x * 100) -- java.util.Formatter rounds the shortest digits HALF_UP"""
    v = x * 100
    if v != v:
        return "NaN%"
    if math.isinf(v):
        return ("Infinity" if v > 0 else "-Infinity") + "%"
    return str(Decimal(repr(v)).quantize(Decimal("0.01"), rounding=ROUND_HALF_UP)) + "%"


# ---- the metrics ----------------------------------------------------------------------------------------------------------------
def check_range(tax, taxon):
    if not 0 <= taxon < tax.size:
        raise CompareError(TAXON_RANGE, 0, f"taxon {taxon} outside the taxonomy")


def filtered_reference(tax, ref_taxa):
    """readReferenceData :119-132 over the kept rows per raw taxon: ({primary taxon: rows} of the defined ones, the unknown taxa)"""
    by_taxon, unknown = {}, set()
    for raw, n in ref_taxa.items():
        check_range(tax, raw)
        t = tax.primary[raw]
        if tax.is_defined(t):
            by_taxon[t] = by_taxon.get(t, 0) + n
        else:
            unknown.add(t)
    return by_taxon, sorted(unknown)


def joined_pairs(tax, pairs):
    """the joined rows per (refTaxon, testTaxon) after primary(), the rows of undefined reference taxa gone"""
    out = {}
    for (r, t), n in pairs.items():
        check_range(tax, r)
        check_range(tax, t)
        r, t = tax.primary[r], tax.primary[t]
        if tax.is_defined(r):
            out[(r, t)] = out.get((r, t), 0) + n
    return out


def per_taxon(tax, ref_by_taxon, joined, rank):
    """perTaxonComparison :170-209 -> (cmp, ref, precision, recall), its stdout lines"""
    name, depth = rank
    anc = lambda x: tax.standard_ancestor_at_level(x, depth)
    ref_taxa = {anc(t) for t in ref_by_taxon} - {None}
    counts = {}
    for (_, t), n in joined.items():
        a = anc(t)
        if a is not None and a != NONE:
            counts[a] = counts.get(a, 0) + n
    cmp_taxa = {t for t, n in counts.items() if n >= MIN_COUNT_TAXON}
    vague = tax.taxa_with_ancestors(ref_taxa) - ref_taxa
    tp, fp = len(ref_taxa & cmp_taxa), len((cmp_taxa - ref_taxa) - vague)
    vp, fn = len(cmp_taxa & vague), len(ref_taxa - cmp_taxa)
    div = lambda a, b: a / b if b else (math.nan if a == 0 else math.inf)
    precision, recall = div(tp, len(cmp_taxa - vague)), div(tp, len(ref_taxa))
    out = [f"*** Per taxon comparison (minimum {MIN_COUNT_TAXON}) at level Some({name})",
           f"Total ref taxa {len(ref_taxa)}, total classified taxa {len(cmp_taxa)}",
           f"TP {tp}, VP {vp} FP {fp}, FN {fn}}}",
           f"Precision {format_perc(precision)} recall {format_perc(recall)}", ""]
    return (len(cmp_taxa), len(ref_taxa), precision, recall), out


def per_read(tax, joined, rank):
    """perReadComparison :211-257 -> (classified, total, tp, fp, vp, fn, ppv, sensitivity, index), its stdout lines"""
    name, depth = rank
    total = sum(joined.values())
    classified = sum(n for (_, t), n in joined.items() if t != NONE)
    cats, index_sum = {}, 0
    for (r, t), n in joined.items():
        c, i = hit_category(tax, r, t, depth)
        cats[c] = cats.get(c, 0) + n
        index_sum += i * n
    tp, fp, vp, fn = (cats.get(c, 0) for c in ("TruePos", "FalsePos", "VaguePos", "FalseNeg"))
    div = lambda a, b: a / b if b else (math.nan if a == 0 else math.inf)
    sensitivity = div(tp, total)
    ppv = tp / (tp + fp) if tp + fp > 0 else 0.0
    index = index_sum / total if total else math.nan
    out = [f"Total reads {total}", f"Classified {classified} {format_perc(div(classified, total))}",
           f"*** Per-read comparison at level Some({name})", f"PPV {format_perc(ppv)} Sensitivity {format_perc(sensitivity)}", ""]
    return (classified, total, tp, fp, vp, fn, ppv, sensitivity, index), out


HEADER = ("title\tfamily\tgroup\tsample\tlibrary\tk\tm\tfrequency\tfl\ts\tc\trank\t"
          "taxon_classified\ttaxon_total\ttaxon_precision\ttaxon_recall\t"
          "read_classified\tread_total\tread_tp\tread_fp\tread_vp\tread_fn\tread_ppv\tread_sensitivity\tread_index")   # Metrics.header :68
TITLE = re.compile(r"(.*)/(.*)/(.+)_(\d+)_(\d+)_s(\d+)_c([\d.]+)_classified/sample=(.*)")                              # :53


def tsv_number(v):
    return java_double(v) if isinstance(v, float) else str(v)


def metrics_row(title, rank, taxon_metrics, read_metrics):
    """Metrics.toTSVString :55-64 -> (row or None, the line printed instead)"""
    m = TITLE.fullmatch(title)
    if not m:
        return None, f"Couldn't extract variables from filename: {title}. Omitting from output."
    family, group, library, k, mm, s, c, sample = m.groups()
    cols = [title, family, group, sample, library, k, mm, "0", "0", s, c, rank[0]] + [tsv_number(v) for v in taxon_metrics + read_metrics]
    return "\t".join(cols), None


def title_of(data_file, multi):
    spl = data_file.split("/")                                     # (Java's split drops trailing empty strings)
    while spl and spl[-1] == "":
        spl.pop()
    return "/".join(spl[-4:]) if multi else spl[-1]


def location_metrics(tax, ref_taxa, pairs, data_file, multi):
    """allMetrics :134-168 from what the join leaves -> (stdout lines, [(title, rank, per-taxon, per-read)] for Genus and Species)"""
    ref_by_taxon, unknown = filtered_reference(tax, ref_taxa)
    joined = joined_pairs(tax, pairs)
    out = [f"Reference contains unknown taxon, not known to taxonomy: {t}. It will be filtered out." for t in unknown]
    out += [f"Filtered reference size: {sum(ref_by_taxon.values())}", f"--------{data_file}--------"]
    metrics = []
    for rank in (GENUS, SPECIES):
        tm, o1 = per_taxon(tax, ref_by_taxon, joined, rank)
        rm, o2 = per_read(tax, joined, rank)
        out += o1 + o2
        metrics.append((title_of(data_file, multi), rank, tm, rm))
    return out, metrics


# ---- the command ----------------------------------------------------------------------------------------------------------------
def read_file(path):
    raw = open(path, "rb").read()
    if path.endswith(".bz2"):
        return bz2.decompress(raw)
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def location_files(location):
    """a file, or a directory's files whose names begin with neither _ nor ., by name"""
    if os.path.isdir(location):
        return [os.path.join(location, f) for f in sorted(os.listdir(location))
                if not f.startswith(("_", ".")) and os.path.isfile(os.path.join(location, f))]
    return [location]


def run(taxonomy_dir, reference, output=None, test_files=None, multi_dirs=None, id_col=2, taxon_col=3, header=False):
    """`compare` -> (stdout, the text of OUTPUT_metrics.tsv); written when output is given"""
    assert (test_files is None) != (multi_dirs is None)
    tax = Taxonomy.load(taxonomy_dir)
    locations = []                                                 # (data file, reference file)
    if test_files is not None:
        locations = [(f, reference) for f in test_files]
    else:
        for d in multi_dirs:                                       # processDirectories :90-103
            for sub in sorted(os.listdir(d)):
                m = re.search(r".*sample=(.+)", sub)
                if m and os.path.isdir(os.path.join(d, sub)):
                    locations.append((f"{d}/{sub}", f"{reference}/sample{m.group(1)}/reads_mapping.tsv"))
    out, rows_out, late = [], [HEADER], []
    for data_file, ref_file in locations:
        rows, _ = reference_rows(read_file(ref_file), id_col, taxon_col, header)
        tests = []
        for f in location_files(data_file):
            tests += kraken_rows(read_file(f))
        pairs, ref_taxa, _, _ = join(rows, tests)
        o, metrics = location_metrics(tax, ref_taxa, pairs, data_file, multi_dirs is not None)
        out += o
        for title, rank, tm, rm in metrics:
            row, complaint = metrics_row(title, rank, tm, rm)
            (rows_out if row else late).append(row or complaint)
    stdout = "".join(line + "\n" for line in out + late)
    tsv = "".join(line + "\n" for line in rows_out)
    if output is not None:
        with open(output + "_metrics.tsv", "w") as f:
            f.write(tsv)
    return stdout, tsv
