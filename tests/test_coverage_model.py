"""The CPU model of the genome coverage (coverage_model.py) against examples worked by hand, `slacken-amd coverage-report` (the
functions `coverage` hands the device's counts to) against the model byte for byte, and the command line of `coverage`: usage, what
is refused, --help.  `stats --library` stays refused."""
import math
import os
import subprocess

import numpy as np
import pytest

import coverage_model as cm
import hostmodel
import taxgen
from test_host_cli import CLI, _built, write_taxonomy  # noqa: F401

SUFFIXES = ("_support_report_minimizerCoverage.txt", "_support_report_minimizerDistinctCoverage.txt", "_min_report.txt")


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=60)


# ---- two short genomes, three taxa, a shared minimizer -------------------------------------------------------------------------
# k = 4, m = 2, no mask, not canonical: the minimizer of a window is the smallest of its three 2-mers in A < C < G < T.
#   taxon 3  AACCGG   windows AACC ACCG CCGG   minimizers AA AC CC   3 super-mers, 3 k-mers
#   taxon 4  TACCGT   windows TACC ACCG CCGT   minimizers AC AC CC   2 super-mers (the AC windows are one), 3 k-mers
#   taxon 4  ACCG     window  ACCG             minimizer  AC         1 super-mer, 1 k-mer
# records by LCA: AA -> 3 (species, depth 8), AC and CC -> 2 = LCA(3, 4) (genus, depth 7)
HAND_NODES = [(1, 1, "no rank"), (2, 1, "genus"), (3, 2, "species"), (4, 2, "species")]
HAND_SEQS = [b"AACCGG", b"TACCGT", b"ACCG"]
HAND_SOURCES = [3, 4, 4]


def hand_world(orc):
    p = orc.params(k=4, m=2, spaces=0, xor_mask=0, canonical=False)
    tax = hostmodel.Taxonomy(HAND_NODES, [(t, f"Taxon {t}") for t, _, _ in HAND_NODES])
    key = lambda s: np.array(orc.encode(s)[:1], np.uint64).astype(np.int64)[0]   # noqa: E731
    index = orc.Index(1, [key("AA"), key("AC"), key("CC")], [3, 2, 2])
    return p, tax, index


def test_hand_worked_coverage(orc):
    p, tax, index = hand_world(orc)
    assert [orc.decode([k & (2**64 - 1)], 2) for k in orc.library_minimizers(p, HAND_SEQS[1]).tolist()] == ["AC", "CC"]
    rows, totals, misses = cm.coverage(orc, p, index, lambda t: hostmodel.depth(tax, t), HAND_SEQS, HAND_SOURCES)
    assert rows == [(3, 7, 2, 2), (3, 8, 1, 1), (4, 7, 3, 2)]
    assert totals == [(3, 3, 3), (4, 4, 3)] and misses == 0
    assert cm.coverage_lines(rows) == ("3  7:2|8:1\n4  7:3\n", "3  7:2|8:1\n4  7:2\n")
    # the index built from the oracle's own build_records is the one written down above
    bases, offsets = cm.pack(HAND_SEQS)
    keys, taxa = orc.build_records(p, np.array(tax.parents, np.int32), bases, offsets, HAND_SOURCES)
    assert sorted(zip(keys.tolist(), taxa.tolist())) == sorted(zip(index.keys[:, 0].tolist(), index.taxa.tolist()))
    # a record missing from the index leaves the join; a NONE source is skipped; a fold between the sequences of one taxon counts
    # its minimizers once per group
    small = orc.Index(1, index.keys[:2, 0], index.taxa[:2])
    rows2, totals2, misses2 = cm.coverage(orc, p, small, lambda t: hostmodel.depth(tax, t), HAND_SEQS + [b"AACC"], HAND_SOURCES + [0])
    assert rows2 == [(3, 7, 1, 1), (3, 8, 1, 1), (4, 7, 2, 1)] and misses2 == 2 and totals2 == totals


def test_kmers_of_the_valid_segments():
    assert cm.segments(b"ACGTNNACgu-A") == [(0, 4), (6, 4), (11, 1)]
    assert cm.kmers(b"ACGTNNACGTA", 4) == 1 + 2 and cm.kmers(b"", 4) == 0 and cm.kmers(b"ACG", 4) == 0 and cm.kmers(b"NNNNNN", 4) == 0


# ---- TotalKmerSizeAggregator on a tree worked by hand --------------------------------------------------------------------------
#   1 root
#   └ 2 genus, own genome of 12 k-mers
#     ├ 5 species, leaf with a genome of 60
#     ├ 4 species, leaf without a genome
#     └ 3 species, no genome of its own
#       ├ 7 leaf, 40
#       └ 6 leaf, 20
# subtree (k-mers, genomes): 6 (20, 1)  7 (40, 1)  3 (60, 2)  4 (0, 0)  5 (60, 1)  2 (132, 4)  1 (132, 4)
TKC_NODES = [(1, 1, "no rank"), (2, 1, "genus"), (3, 2, "species"), (4, 2, "species"), (5, 2, "species"), (6, 3, "no rank"), (7, 3, "no rank")]
TKC_SIZES = [(2, 12), (5, 60), (6, 20), (7, 40)]
TKC_RECORDS = [(2, 5), (5, 3), (6, 2)]
TKC_REPORT = ("#Perc\tAggregate\tIn taxon\tTKC1-LeafOnly\tTKC2-FirstChildren\tTKC3-AllChildren\tRank\tTaxon\tName\n"
              "100.00\t10\t0\t33\t33\t33\tR\t1\tTaxon 1\n"
              "100.00\t10\t5\t33\t34\t33\tG\t2\t  Taxon 2\n"
              " 30.00\t3\t3\t60\t60\t60\tS\t5\t    Taxon 5\n"
              " 20.00\t2\t0\t30\t30\t30\tS\t3\t    Taxon 3\n"
              " 20.00\t2\t2\t20\t20\t20\tS1\t6\t      Taxon 6\n")


def tkc_tax():
    return hostmodel.Taxonomy(TKC_NODES, [(t, f"Taxon {t}") for t, _, _ in TKC_NODES])


def write_dmp(d, nodes):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        f.write("".join(f"{t}\t|\t{p}\t|\t{r}\t|\n" for t, p, r in nodes))
    with open(os.path.join(d, "names.dmp"), "w") as f:
        f.write("".join(f"{t}\t|\tTaxon {t}\t|\t\t|\tscientific name\t|\n" for t, _, _ in nodes))
    return str(d)


def test_hand_worked_tkc_columns():
    agg = cm.TotalKmerSizeAggregator(tkc_tax(), TKC_SIZES)
    assert agg.tree == {6: (20, 1), 7: (40, 1), 3: (60, 2), 4: (0, 0), 5: (60, 1), 2: (132, 4), 1: (132, 4)}
    # the inner node with a genome of its own: S1 = (60 + 0 + 60 + 12) / (1 + 0 + 2 + 1), S2 = (12 + 60 + 30) / 3,
    # S3 = (33 * 3 + 34 * 2) / (3 + 2)
    assert agg.columns(2) == [33.0, 34.0, 33.4]
    assert agg.columns(3) == [30.0, 30.0, 30.0]
    assert agg.columns(5) == [60.0, 60.0, 60.0]        # a leaf with a genome: S1 counts it twice over two, as the reference does
    s1, s2, s3 = agg.columns(4)                         # a leaf without one: 0 / 0, which Math.round prints as 0
    assert math.isnan(s1) and (s2, s3) == (0.0, 0.0) and cm.java_round(s1) == 0
    assert agg.columns(1) == [33.0, 33.0, 33.0]
    assert [cm.java_round(x) for x in (0.5, 1.5, 2.4999, 33.4, 0.0)] == [1, 2, 2, 33, 0]
    assert cm.min_report(tkc_tax(), TKC_RECORDS, TKC_SIZES) == TKC_REPORT
    assert cm.tie_distance(tkc_tax(), TKC_RECORDS, TKC_SIZES) > 0.05


def report_files(tmp_path, tdir, records, sizes, rows, name="out"):
    write = lambda path, lines: (open(path, "w").write("".join("\t".join(map(str, l)) + "\n" for l in lines)), str(path))[1]   # noqa: E731
    out = str(tmp_path / "sub" / name)
    r = cli("coverage-report", tdir, write(tmp_path / "records.tsv", records), write(tmp_path / "sizes.tsv", sizes),
            write(tmp_path / "rows.tsv", rows), out)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    return [open(out + s).read() for s in SUFFIXES]


def test_coverage_report_hand_written_cases(tmp_path):
    tdir = write_dmp(tmp_path / "tax", TKC_NODES)
    rows = [(4, 7, 3, 2), (3, 8, 1, 1), (3, 7, 2, 2)]                     # any order
    got = report_files(tmp_path, tdir, TKC_RECORDS[::-1], TKC_SIZES[::-1], rows)
    assert got == ["3  7:2|8:1\n4  7:3\n", "3  7:2|8:1\n4  7:2\n", TKC_REPORT]
    # sources the taxonomy lacks, negative depths and a source without a k-mer
    rows = [(9000000, -1, 5, 1), (9000000, 3, 2**40, 7), (-5, 0, 1, 1)]
    got = report_files(tmp_path, tdir, TKC_RECORDS, TKC_SIZES + [(9000000, 77), (4, 0)], rows, "odd")
    assert got[:2] == list(cm.coverage_lines(sorted(rows)))
    assert got[0] == f"-5  0:1\n9000000  -1:5|3:{2**40}\n"
    assert got[2] == cm.min_report(tkc_tax(), TKC_RECORDS, TKC_SIZES + [(9000000, 77), (4, 0)]) != TKC_REPORT


@pytest.mark.parametrize("seed,size", [(1, 40), (2, 400), (3, 2000)])
def test_coverage_report_matches_the_model(tmp_path, seed, size):
    rng = np.random.default_rng(seed)
    parents = taxgen.taxonomy(size, rng)
    tdir = str(tmp_path / "tax")
    tax = write_taxonomy(tdir, parents, rng, ranked=0.5)
    defined = taxgen.defined_taxa(parents)
    stored = sorted(int(t) for t in rng.choice(defined, size=max(3, len(defined) // 3), replace=False))
    records = [(t, int(rng.integers(1, 50)) if rng.random() < 0.9 else int(rng.integers(1, 2**40))) for t in stored]
    for attempt in range(200):     # genome sizes whose averages stay clear of a .5 tie: rounding cannot decide the comparison
                                   # (multiples of 12: the average of two, three or four genomes is a whole number)
        labelled = sorted(int(t) for t in rng.choice(defined, size=max(3, len(defined) // 4), replace=False))
        sizes = [(t, 12 * int(rng.integers(0, 400_000))) for t in labelled]
        if cm.tie_distance(tax, records, sizes) > 1e-6:
            break
    assert cm.tie_distance(tax, records, sizes) > 1e-6
    rows = sorted((s, int(d), int(rng.integers(1, 10**6)), int(rng.integers(1, 1000))) for s in labelled[::2] for d in rng.choice(10, size=3, replace=False) - 1)
    got = report_files(tmp_path, tdir, records, sizes, rows)
    assert got == [*cm.coverage_lines(rows), cm.min_report(tax, records, sizes)]
    inner = [t for t, _ in sizes if tax.children[t]]
    assert inner and any(not tax.children[t] for t, _ in sizes)            # genomes on inner nodes and on leaves


def test_usage_refusals_and_help():
    """Refused on the command line alone: before any library is read or any device call is made"""
    rest = ["-i", "a", "-l", "lib", "-o", "out"]
    r = cli("coverage", *rest, "--shard-table")
    assert r.returncode != 0 and "--shard-table is not supported by coverage" in r.stderr and r.stdout == ""
    for devices in ("0,1", "all"):
        r = cli("coverage", *rest, "--devices", devices)
        assert r.returncode != 0 and "must fit one GPU" in r.stderr and r.stdout == ""
    for args in ([], ["-i", "a"], ["-i", "a", "-l", "lib"], ["-i", "a", "-o", "out"], ["--library", "lib", "--output", "out"]):
        r = cli("coverage", *args)
        assert r.returncode != 0 and "usage: coverage -i INDEX -l LIBRARY_DIR -o OUTPUT" in r.stderr and "unknown command" not in r.stderr
    r = cli("coverage", *rest, "--histogram")
    assert r.returncode != 0 and "unknown option --histogram" in r.stderr
    r = cli("coverage-report", "a", "b")
    assert r.returncode != 0 and "usage: coverage-report" in r.stderr
    out = cli("--help").stdout
    for word in ("slacken-amd coverage -i INDEX -l|--library LIBRARY_DIR -o OUTPUT", "coverage-report TAXONOMY_DIR", "TKC1-LeafOnly",
                 "SLK_COVERAGE_MAX_PAIRS"):
        assert word in out
    r = cli("no-such-command")
    assert r.returncode != 0 and "`coverage`" in r.stderr


def test_the_old_flags_stay_refused():
    for cmd, rest in (("stats", ["-i", "a"]), ("inspect", ["-i", "a", "-o", "b"])):
        r = cli(cmd, *rest, "--library", "lib")
        assert r.returncode != 0 and "genome coverage" in r.stderr and "not supported" in r.stderr and r.stdout == ""
    r = cli("classify2", "-i", "a", "-o", "b", "--library", "lib", "--index-reports", "x.fq")
    assert r.returncode != 0 and r.stdout == ""
