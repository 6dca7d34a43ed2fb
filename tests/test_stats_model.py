"""The model of `stats` / `inspect` (stats_model.py) on a case worked out by hand from the Scala: a taxonomy with unranked nodes
(their depth is that of the nearest ranked ancestor), stored taxa that are inner nodes and leaves, ancestors shared between stored
taxa (counted once in the tree size), an id the taxonomy does not define, and a label file with a present and an absent taxon."""
import os

import hostmodel
import stats_model as sm

NODES = [(1, 1, "no rank"), (131567, 1, "no rank"), (2, 131567, "superkingdom"), (10, 2, "genus"), (11, 10, "species"),
         (12, 10, "species"), (20, 12, "no rank"), (30, 131567, "clade")]
NAMES = [(1, "root"), (131567, "cellular organisms"), (2, "Bacteria"), (10, "Genus ten"), (11, "Species eleven"),
         (12, "Species twelve"), (20, "Strain twenty"), (30, "Clade thirty")]
# inner nodes 2 and 10; leaves 11, 20 (unranked under a species: depth 8) and 30 (unranked under the unranked 131567: depth 0)
COUNTS = [(2, 1), (10, 5), (11, 7), (20, 3), (30, 2)]
# ... and 500, which the taxonomy does not define: a leaf of depth -1 without ancestors
COUNTS_UNDEFINED = COUNTS + [(500, 4)]

# tree: {2, 10, 11, 20, 30} and their ancestors {1, 131567, 12}; leaves 11, 20, 30 with 7 + 3 + 2 of the 18 records
STATS = ("Tree size: 8 taxa, stored taxa: 5, of which 3 leaf taxa (60.00%)\n"
         "Total 31-minimizers: 18, of which leaf records: 12 (66.67%)\n")
STATS_UNDEFINED = ("Tree size: 9 taxa, stored taxa: 6, of which 4 leaf taxa (66.67%)\n"
                   "Total 35-minimizers: 22, of which leaf records: 16 (72.73%)\n")
HISTOGRAMS = ("Minimizer depth histogram\n"
              "+-----+------------+-----+\n"
              "|depth|        rank|count|\n"
              "+-----+------------+-----+\n"
              "|    0|        root|    2|\n"
              "|    1|superkingdom|    1|\n"
              "|    7|       genus|    5|\n"
              "|    8|     species|   10|\n"
              "+-----+------------+-----+\n"
              "\n"
              "Taxon depth histogram\n"
              "+-----+------------+-----+\n"
              "|depth|        rank|count|\n"
              "+-----+------------+-----+\n"
              "|    0|        root|    1|\n"
              "|    1|superkingdom|    1|\n"
              "|    7|       genus|    1|\n"
              "|    8|     species|    2|\n"
              "+-----+------------+-----+\n"
              "\n")
KMER_HISTOGRAM_UNDEFINED = ("+-----+------------+-----+\n"
                            "|depth|        rank|count|\n"
                            "+-----+------------+-----+\n"
                            "|   -1|         ???|    4|\n"
                            "|    0|        root|    2|\n"
                            "|    1|superkingdom|    1|\n"
                            "|    7|       genus|    5|\n"
                            "|    8|     species|   10|\n"
                            "+-----+------------+-----+\n"
                            "\n")
HEAD = "#Perc\tAggregate\tIn taxon\tRank\tTaxon\tName\n"
MIN_REPORT = (HEAD +
              "100.00\t18\t0\tR\t1\troot\n"
              "100.00\t18\t0\tR1\t131567\t  cellular organisms\n"
              " 88.89\t16\t1\tD\t2\t    Bacteria\n"
              " 83.33\t15\t5\tG\t10\t      Genus ten\n"
              " 38.89\t7\t7\tS\t11\t        Species eleven\n"
              " 16.67\t3\t0\tS\t12\t        Species twelve\n"
              " 16.67\t3\t3\tS1\t20\t          Strain twenty\n"
              " 11.11\t2\t2\tR2\t30\t    Clade thirty\n")
# one per stored taxon; 12 and 11 tie under the genus: the children's own order (descending id) stays
GENOME_REPORT = (HEAD +
                 "100.00\t5\t0\tR\t1\troot\n"
                 "100.00\t5\t0\tR1\t131567\t  cellular organisms\n"
                 " 80.00\t4\t1\tD\t2\t    Bacteria\n"
                 " 60.00\t3\t1\tG\t10\t      Genus ten\n"
                 " 20.00\t1\t0\tS\t12\t        Species twelve\n"
                 " 20.00\t1\t1\tS1\t20\t          Strain twenty\n"
                 " 20.00\t1\t1\tS\t11\t        Species eleven\n"
                 " 20.00\t1\t1\tR2\t30\t    Clade thirty\n")
# 11 and 30 are stored, 12 (labelled twice) is not
LABELS = "seqA\t11\nseqB\t12\nseqC\t12\nseqD\t30\n"
MISSING_REPORT = (HEAD +
                  "100.00\t1\t0\tR\t1\troot\n"
                  "100.00\t1\t0\tR1\t131567\t  cellular organisms\n"
                  "100.00\t1\t0\tD\t2\t    Bacteria\n"
                  "100.00\t1\t0\tG\t10\t      Genus ten\n"
                  "100.00\t1\t1\tS\t12\t        Species twelve\n")
NOTHING_MISSING = HEAD + "   NaN\t0\t0\tR\t1\troot\n"


def tax():
    return hostmodel.Taxonomy(NODES, NAMES)


def write_dmp(d):
    """the taxonomy as nodes.dmp / names.dmp (for the command-line tests)"""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for t, p, r in NODES:
            f.write(f"{t}\t|\t{p}\t|\t{r}\t|\n")
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for t, nm in NAMES:
            f.write(f"{t}\t|\t{nm}\t|\t\t|\tscientific name\t|\n")
    return str(d)


def test_depth_falls_through_to_a_ranked_ancestor():
    t = tax()
    assert [sm.depth(t, x) for x in (1, 131567, 2, 10, 11, 12, 20, 30, 500, 10**7)] == [0, 0, 1, 7, 8, 8, 8, 0, -1, -1]
    assert [sm.is_leaf(t, x) for x in (1, 2, 10, 11, 12, 20, 30, 500)] == [False, False, False, True, False, True, True, True]
    assert sm.rank_of_depth(-1) == "???" and sm.rank_of_depth(0) == "root" and sm.rank_of_depth(8) == "species" and sm.rank_of_depth(9) == "???"


def test_tree_size_counts_shared_ancestors_once():
    t = tax()
    assert sm.taxa_with_ancestors(t, [11]) == {11, 10, 2, 131567, 1}
    assert sm.taxa_with_ancestors(t, [11, 20]) == {11, 20, 12, 10, 2, 131567, 1}
    assert sm.taxa_with_ancestors(t, [t0 for t0, _ in COUNTS]) == {1, 131567, 2, 10, 11, 12, 20, 30}


def test_stats_lines():
    t = tax()
    assert sm.index_stats(t, COUNTS, 31) == STATS == sm.stats(t, COUNTS, 31, False)
    assert sm.index_stats(t, COUNTS_UNDEFINED, 35) == STATS_UNDEFINED
    assert sm.index_stats(t, [], 31) == ("Tree size: 0 taxa, stored taxa: 0, of which 0 leaf taxa (NaN%)\n"
                                         "Total 31-minimizers: 0, of which leaf records: 0 (NaN%)\n")
    # Java rounds the shortest decimal digits half up
    assert [sm.format_perc(x) for x in (0.0, 1.0, 0.00125, 1 / 3, 2 / 3)] == ["0.00%", "100.00%", "0.13%", "33.33%", "66.67%"]


def test_histograms():
    t = tax()
    assert sm.stats(t, COUNTS, 31, True) == HISTOGRAMS
    assert sm.depth_histogram(t, COUNTS_UNDEFINED, True) == KMER_HISTOGRAM_UNDEFINED
    assert sm.depth_histogram(t, [], False) == "+-----+----+-----+\n|depth|rank|count|\n+-----+----+-----+\n+-----+----+-----+\n\n"
    # a count wider than its header widens the column
    assert sm.depth_histogram(t, [(11, 12345678901)], True) == (
        "+-----+-------+-----------+\n|depth|   rank|      count|\n+-----+-------+-----------+\n|    8|species|12345678901|\n"
        "+-----+-------+-----------+\n\n")


def test_reports():
    t = tax()
    assert sm.reports(t, COUNTS) == {"_min_report.txt": MIN_REPORT, "_genome_report.txt": GENOME_REPORT}
    got = sm.reports(t, COUNTS, LABELS)
    assert sorted(got) == ["_genome_report.txt", "_min_report.txt", "_missing_report.txt"]
    assert got["_missing_report.txt"] == MISSING_REPORT
    assert sm.label_taxa(LABELS) == {11, 12, 30}
    assert sm.reports(t, COUNTS, "seqA\t11\n")["_missing_report.txt"] == NOTHING_MISSING
