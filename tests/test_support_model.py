"""The CPU model of the sample support (support_model.py) against an example worked by hand, its report texts, and the command line
of `support`: usage errors raised before any device is opened, and --help."""
import subprocess

import numpy as np

import hostmodel
import support_model as sm
from test_host_cli import CLI, _built  # noqa: F401


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=60)


# ---- six sequences, three taxa ------------------------------------------------------------------------------------------------
# k = 5, m = 3, no mask, not canonical: the minimizer of a window is the smallest of its three 3-mers in A < C < G < T.
# records: AAC -> 3 (species), ACA -> 4 (species), ATT -> 4, AAG -> 2 (their genus); ACT is in no record.
#   TAACTT          windows TAACT AACTT     minimizers AAC AAC     one super-mer of 2 k-mers -> 3
#   AACTTT          windows AACTT ACTTT     minimizers AAC ACT     AAC again (shared with the read above) -> 3; ACT: the miss
#   AAGTT           window  AAGTT           minimizer  AAG         -> 2, above the species rank
#   ACATTNACATTG    ACATT | N | ACATTG      ACA | ACA ATT          the N splits the read: ACA twice and ATT -> 4
#   AACTT + TACAT   a pair                  AAC | border | ACA     -> 3 and -> 4; the mate-pair border never counts
HAND_NODES = [(1, 1, "no rank"), (2, 1, "genus"), (3, 2, "species"), (4, 2, "species")]
HAND_READS = ["TAACTT", "AACTTT", "AAGTT", "ACATTNACATTG", ("AACTT", "TACAT")]


def hand_world(orc):
    p = orc.params(k=5, m=3, spaces=0, xor_mask=0, canonical=False)
    tax = hostmodel.Taxonomy(HAND_NODES, [(t, f"Taxon {t}") for t, _, _ in HAND_NODES])
    key = lambda s: np.array(orc.encode(s)[:1], np.uint64).astype(np.int64)[0]   # noqa: E731
    index = orc.Index(1, [key("AAC"), key("ACA"), key("ATT"), key("AAG")], [3, 4, 4, 2])
    return p, tax, index


def test_hand_worked_support(orc):
    p, tax, index = hand_world(orc)
    depth_of = lambda t: hostmodel.depth(tax, t)   # noqa: E731
    assert [(orc.decode(list(sp["key"]), 3), sp["kmers"], sp["flag"]) for sp in orc.spans(p, "ACATTNACATTG")] == \
        [("ACA", 1, 1), ("ACA", 1, 1), ("ATT", 1, 1)]
    got = sm.support(orc, p, index, depth_of, HAND_READS)
    assert got.rows(8) == [(3, 4, 3, 1), (4, 4, 4, 2)]
    assert got.totals(8) == (6, 9, 8, 7)                       # one miss (ACT), one hit above the rank (AAG)
    assert got.rows(8, want_distinct=False) == [(3, 4, 3, 0), (4, 4, 4, 0)]
    assert got.rows(7) == [(2, 1, 1, 1), (3, 4, 3, 1), (4, 4, 4, 2)] and got.totals(7) == (6, 9, 8, 8)
    assert got.rows(0) == got.rows(7) and got.rows(9) == []
    # the two reads that share AAC, alone: one distinct minimizer, two super-mers, three k-mers
    assert sm.support(orc, p, index, depth_of, HAND_READS[:2]).rows(8) == [(3, 3, 2, 1)]
    # any order gives the same
    assert sm.support(orc, p, index, depth_of, HAND_READS[::-1]).rows(8) == got.rows(8)


def test_report_texts(orc):
    p, tax, index = hand_world(orc)
    rows = sm.support(orc, p, index, lambda t: hostmodel.depth(tax, t), HAND_READS).rows(7)
    texts = sm.report_texts(tax, rows, [(4, 2), (3, 1)])
    assert set(texts) == set(sm.SUFFIXES)
    head = "#Perc\tAggregate\tIn taxon\tRank\tTaxon\tName\n"
    assert texts["totalKmerCount"] == head + ("100.00\t9\t0\tR\t1\tTaxon 1\n100.00\t9\t1\tG\t2\t  Taxon 2\n"
                                              " 44.44\t4\t4\tS\t4\t    Taxon 4\n 44.44\t4\t4\tS\t3\t    Taxon 3\n")
    assert texts["totalMinimizerCount"] == head + ("100.00\t8\t0\tR\t1\tTaxon 1\n100.00\t8\t1\tG\t2\t  Taxon 2\n"
                                                   " 50.00\t4\t4\tS\t4\t    Taxon 4\n 37.50\t3\t3\tS\t3\t    Taxon 3\n")
    assert texts["distinctMinimizerCount"] == head + ("100.00\t4\t0\tR\t1\tTaxon 1\n100.00\t4\t1\tG\t2\t  Taxon 2\n"
                                                      " 50.00\t2\t2\tS\t4\t    Taxon 4\n 25.00\t1\t1\tS\t3\t    Taxon 3\n")
    assert texts["classifiedReadCount"] == head + ("100.00\t3\t0\tR\t1\tTaxon 1\n100.00\t3\t0\tG\t2\t  Taxon 2\n"
                                                   " 66.67\t2\t2\tS\t4\t    Taxon 4\n 33.33\t1\t1\tS\t3\t    Taxon 3\n")


def test_usage_errors_and_help():
    """Refused on the command line alone: before any library is read or any device call is made"""
    usage = "usage: support -i INDEX -o OUTPUT [--rank RANK (species)] [--min-hits N] [-p] [--devices D] FILES..."
    for args in ([], ["-i", "a", "x.fq"], ["-o", "out", "x.fq"], ["-i", "a", "-o", "out"], ["--index", "a", "reads.fq"]):
        r = cli("support", *args)
        assert r.returncode != 0 and usage in r.stderr and "unknown command" not in r.stderr and r.stdout == ""
    rest = ["-i", "a", "-o", "out", "x.fq"]
    r = cli("support", *rest, "--rank", "tribe")
    assert r.returncode != 0 and "unknown rank tribe" in r.stderr and r.stdout == ""
    r = cli("support", *rest, "--shard-table")
    assert r.returncode != 0 and "--shard-table is not supported by support" in r.stderr and usage in r.stderr and r.stdout == ""
    r = cli("support", *rest, "--histogram")
    assert r.returncode != 0 and "unknown option --histogram" in r.stderr and r.stdout == ""
    r = cli("support", "-i", "a", "-o", "out", "-p", "x_1.fq")
    assert r.returncode != 0 and "pairs of files" in r.stderr
    out = cli("--help").stdout
    for word in ("slacken-amd support -i INDEX -o OUTPUT [--rank RANK (species)] [--min-hits N] [-p] [--devices D] FILES...",
                 "OUTPUT_support_report_totalKmerCount.txt", "OUTPUT_support_report_distinctMinimizerCount.txt",
                 "OUTPUT_support_report_totalMinimizerCount.txt", "OUTPUT_support_report_classifiedReadCount.txt", "first of --devices"):
        assert word in out
    r = cli("no-such-command")
    assert r.returncode != 0 and "`support`" in r.stderr
    r = cli("classify2", "-i", "a", "-o", "b", "--library", "lib", "--index-reports", "x.fq")
    assert r.returncode != 0 and "not supported" in r.stderr and r.stdout == ""
