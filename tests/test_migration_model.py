"""compare-index without a GPU: the model (migration_model.py) on a case written out by hand, the same case through
`slacken-amd migration-report` (the function compare-index hands the device's triples to), and the command line."""
import os
import subprocess

import hostmodel
import migration_model as mm
from test_host_cli import CLI, _built  # noqa: F401

# three ranks (superkingdom, genus, species) under the root and "cellular organisms"; 500 and 600 are not in the taxonomy
NODES = [(1, 1, "no rank"), (131567, 1, "no rank"), (2, 131567, "superkingdom"), (10, 2, "genus"), (11, 10, "species"),
         (12, 10, "species")]
NAMES = [(1, "root"), (131567, "cellular organisms"), (2, "Bacteria"), (10, "Genus ten"), (11, "Species eleven"),
         (12, "Species twelve")]
# (key, t1) of the subject, key -> t2 of the reference
SUBJECT = [(100, 11),       # species -> its genus: 1 step
           (102, 12),       # species -> ROOT: 8 steps, and the one line of the report
           (103, 131567),   # cellular organisms -> ROOT: inside {1, 131567}, not in the report
           (104, 500),      # t1 unknown to the taxonomy: -100
           (105, 11),       # t2 unknown to the taxonomy: -200
           (106, 12)]       # the reference lacks the key: leaves the join
REFERENCE = {100: 10, 102: 1, 103: 1, 104: 11, 105: 600, 999: 12}

TRIPLES = [(11, 10, 1, 1), (11, 600, -200, 1), (12, 1, 8, 1), (500, 11, -100, 1), (131567, 1, 0, 1)]
TABLE = ("+-----+------------+\n"
         "|steps|count(steps)|\n"
         "+-----+------------+\n"
         "| -200|           1|\n"
         "| -100|           1|\n"
         "|    0|           1|\n"
         "|    1|           1|\n"
         "|    8|           1|\n"
         "+-----+------------+\n"
         "\n")
REPORT = ("#Perc\tAggregate\tIn taxon\tRank\tTaxon\tName\n"
          "100.00\t1\t0\tR\t1\troot\n"
          "100.00\t1\t0\tR1\t131567\t  cellular organisms\n"
          "100.00\t1\t0\tD\t2\t    Bacteria\n"
          "100.00\t1\t0\tG\t10\t      Genus ten\n"
          "100.00\t1\t1\tS\t12\t        Species twelve\n")


def write_dmp(d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for t, p, r in NODES:
            f.write(f"{t}\t|\t{p}\t|\t{r}\t|\n")
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for t, nm in NAMES:
            f.write(f"{t}\t|\t{nm}\t|\t\t|\tscientific name\t|\n")
    return str(d)


def test_model_on_a_hand_written_case():
    tax = hostmodel.Taxonomy(NODES, NAMES)
    pairs, matched, unmatched = mm.join(SUBJECT, REFERENCE)
    assert (matched, unmatched) == (5, 1)
    trip = mm.triples(pairs, tax)
    assert trip == TRIPLES
    assert mm.triples(pairs, None, with_depths=False) == [(a, b, 0, c) for a, b, _, c in TRIPLES]
    assert mm.show(trip) == TABLE
    assert mm.to_root(trip) == [(12, 1)]
    assert mm.report(tax, trip) == REPORT
    # wider cells widen their column; no rows leaves the rules and the header
    assert mm.show([(5, 5, -100, 3), (6, 6, 0, 1234567890123), (7, 8, 2, 17)]) == (
        "+-----+-------------+\n|steps| count(steps)|\n+-----+-------------+\n| -100|            3|\n"
        "|    0|1234567890123|\n|    2|           17|\n+-----+-------------+\n\n")
    assert mm.show([]) == "+-----+------------+\n|steps|count(steps)|\n+-----+------------+\n+-----+------------+\n\n"


def test_migration_report_helper(tmp_path):
    """No index is created: this runs without a GPU"""
    tdir = write_dmp(tmp_path / "tax")
    pairs = tmp_path / "pairs.tsv"
    # out of order
    rows = [(12, 1, 1), (11, 10, 1), (131567, 1, 1), (500, 11, 1), (11, 600, 1)]
    pairs.write_text("".join(f"{a}\t{b}\t{c}\n" for a, b, c in rows))
    out = tmp_path / "sub" / "cmp"
    r = subprocess.run([CLI, "migration-report", tdir, tdir, str(pairs), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    tax = hostmodel.Taxonomy(NODES, NAMES)
    trip = mm.triples(mm.join(SUBJECT, REFERENCE)[0], tax)
    assert r.stdout == mm.show(trip) == TABLE
    assert open(str(out) + "_taxaToRoot_report.txt").read() == mm.report(tax, trip) == REPORT
    # counts add up per steps value and per t1; wide counts widen the column
    rows2 = [(12, 1, 5), (12, 131567, 7), (11, 1, 40000000000), (11, 11, 3), (12, 12, 4), (131567, 1, 9), (1, 131567, 2)]
    pairs.write_text("".join(f"{a}\t{b}\t{c}\n" for a, b, c in rows2))
    r = subprocess.run([CLI, "migration-report", tdir, tdir, str(pairs), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    trip2 = [(a, b, mm.steps(tax, a, b), c) for a, b, c in sorted(rows2)]
    assert mm.to_root(trip2) == [(11, 40000000000), (12, 12)]
    assert r.stdout == mm.show(trip2)
    assert open(str(out) + "_taxaToRoot_report.txt").read() == mm.report(tax, trip2)


def test_compare_index_argument_errors():
    """Refused on the command line alone: before any library is read or any device call is made"""
    for args in ([], ["--shard-table"], ["-i", "a", "-r", "b", "-o", "c", "--shard-table"], ["-i", "a"], ["-i", "a", "-r", "b"]):
        r = subprocess.run([CLI, "compare-index", *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "usage: compare-index -i SUBJECT" in r.stderr, r.stderr
        assert r.stdout == ""
    r = subprocess.run([CLI, "compare-index", "-i", "a", "-r", "b", "-o", "c", "--devices", "0,1"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "must fit one GPU" in r.stderr


def test_compare_index_is_a_known_command():
    for cmd in ("compareIndex", "compare-index"):
        r = subprocess.run([CLI, cmd], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "unknown command" not in r.stderr and "usage: compare-index" in r.stderr
    r = subprocess.run([CLI, "stats"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown command" in r.stderr and "compare-index" in r.stderr
    assert "compare-index" in subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
