"""`stats` and `inspect` without a GPU: `slacken-amd stats-report` (the functions `stats` and `inspect` hand the device's counts
to) against stats_model.py, byte for byte -- the hand-written case of test_stats_model.py and random stored sets on taxgen
taxonomies --, and the command line: what is refused, and --help."""
import os
import subprocess

import numpy as np
import pytest

import stats_model as sm
import taxgen
import test_stats_model as hand
from test_host_cli import CLI, _built, write_taxonomy  # noqa: F401

SUFFIXES = ("_min_report.txt", "_genome_report.txt", "_missing_report.txt")


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=60)


def write_counts(path, counts):
    with open(path, "w") as f:
        f.write("".join(f"{t}\t{c}\n" for t, c in counts))
    return str(path)


def check_against_model(tmp_path, tdir, tax, counts, m, labels_text):
    """every output of stats-report for one (taxonomy, counts): stats lines, histograms, the two reports, and the third with labels"""
    tsv = write_counts(tmp_path / "counts.tsv", counts)
    r = cli("stats-report", tdir, tsv, m)
    assert r.returncode == 0, r.stderr
    assert r.stdout == sm.stats(tax, counts, m, False)
    r = cli("stats-report", tdir, tsv, m, "--histogram")
    assert r.returncode == 0, r.stderr
    assert r.stdout == sm.stats(tax, counts, m, True)
    out = str(tmp_path / "sub" / "dir" / "lib")
    r = cli("stats-report", tdir, tsv, m, "-o", out)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    want = sm.reports(tax, counts)
    for suffix in SUFFIXES[:2]:
        assert open(out + suffix).read() == want[suffix]
    assert not os.path.exists(out + SUFFIXES[2])
    labels = tmp_path / "labels.tsv"
    labels.write_text(labels_text)
    out = str(tmp_path / "with_labels")
    r = cli("stats-report", tdir, tsv, m, "--output", out, "--labels", labels)
    assert r.returncode == 0, r.stderr
    want = sm.reports(tax, counts, labels_text)
    for suffix in SUFFIXES:
        assert open(out + suffix).read() == want[suffix], suffix


def test_stats_report_hand_written_case(tmp_path):
    tdir = hand.write_dmp(tmp_path / "tax")
    tsv = write_counts(tmp_path / "c.tsv", hand.COUNTS[::-1])        # any order
    assert cli("stats-report", tdir, tsv, 31).stdout == hand.STATS
    assert cli("stats-report", tdir, tsv, 31, "--histogram").stdout == hand.HISTOGRAMS
    assert cli("stats-report", tdir, write_counts(tmp_path / "u.tsv", hand.COUNTS_UNDEFINED), 35).stdout == hand.STATS_UNDEFINED
    labels = tmp_path / "labels.tsv"
    labels.write_text(hand.LABELS)
    out = str(tmp_path / "o")
    assert cli("stats-report", tdir, tsv, 31, "-o", out, "--labels", labels).returncode == 0
    assert [open(out + s).read() for s in SUFFIXES] == [hand.MIN_REPORT, hand.GENOME_REPORT, hand.MISSING_REPORT]
    labels.write_text("seqA\t11\n")
    assert cli("stats-report", tdir, tsv, 31, "-o", out, "--labels", labels).returncode == 0
    assert open(out + SUFFIXES[2]).read() == hand.NOTHING_MISSING
    # no stored taxon at all
    empty = write_counts(tmp_path / "e.tsv", [])
    assert cli("stats-report", tdir, empty, 31).stdout == sm.stats(hand.tax(), [], 31, False)
    assert cli("stats-report", tdir, empty, 31, "--histogram").stdout == sm.stats(hand.tax(), [], 31, True)


@pytest.mark.parametrize("seed,size,ranked", [(1, 40, 0.5), (2, 400, 0.2), (3, 2000, 0.9)])
def test_stats_report_matches_the_model(tmp_path, seed, size, ranked):
    rng = np.random.default_rng(seed)
    parents = taxgen.taxonomy(size, rng)
    tdir = str(tmp_path / "tax")
    tax = write_taxonomy(tdir, parents, rng, ranked=ranked)
    defined = taxgen.defined_taxa(parents)
    stored = sorted(int(t) for t in rng.choice(defined, size=max(3, len(defined) // 3), replace=False))
    # a few taxa hold most records, some counts are beyond 32 bits
    counts = [(t, int(rng.integers(1, 50)) if rng.random() < 0.9 else int(rng.integers(1, 2**40))) for t in stored]
    pool = stored[:5] + [int(t) for t in rng.choice(defined, size=10, replace=False)]
    labels_text = "".join(f"seq{i}\t{t}\n" for i, t in enumerate(pool + pool[:3]))
    assert sm.label_taxa(labels_text) - set(stored) and sm.label_taxa(labels_text) & set(stored)
    check_against_model(tmp_path, tdir, tax, counts, 31, labels_text)


def test_refusals():
    """Refused on the command line alone: before any library is read or any device call is made"""
    for cmd, rest in (("stats", ["-i", "a"]), ("inspect", ["-i", "a", "-o", "b"])):
        r = cli(cmd, *rest, "--library", "lib")
        assert r.returncode != 0 and "genome coverage" in r.stderr and "not supported" in r.stderr and r.stdout == ""
        r = cli(cmd, *rest, "--shard-table")
        assert r.returncode != 0 and f"--shard-table is not supported by {cmd}" in r.stderr and r.stdout == ""
        for devices in ("0,1", "all"):
            r = cli(cmd, *rest, "--devices", devices)
            assert r.returncode != 0 and "must fit one GPU" in r.stderr and r.stdout == ""
        r = cli(cmd, "--devices", "0")                                               # no index
        assert r.returncode != 0 and f"usage: {cmd} -i INDEX" in r.stderr and "unknown command" not in r.stderr
        r = cli(cmd)                                                                  # nothing at all: the list of commands
        assert r.returncode != 0 and f"`{cmd} -i INDEX" in r.stderr and r.stdout == ""
    assert "usage: inspect" in cli("inspect", "-i", "a").stderr                     # -o is required
    assert cli("stats", "-i", "a", "--labels", "x").returncode != 0                  # an option of inspect
    for args in (["stats-report"], ["stats-report", "a", "b"], ["stats-report", "a", "b", "31", "--labels", "x"],
                 ["stats-report", "a", "b", "31", "--shard-table"], ["stats-report", "a", "b", "31", "--devices", "0,1"]):
        r = cli(*args)
        assert r.returncode != 0 and "usage: stats-report" in r.stderr


def test_help_names_the_commands():
    out = cli("--help").stdout
    for word in ("slacken-amd stats -i INDEX", "slacken-amd inspect -i INDEX", "stats-report TAXONOMY_DIR"):
        assert word in out
    r = cli("no-such-command")
    assert r.returncode != 0 and "unknown command" in r.stderr and "`stats -i INDEX` and `inspect -i INDEX -o OUTPUT`" in r.stderr
