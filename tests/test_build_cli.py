"""`slacken-amd build` without a GPU: the usage line, what is refused on the command line alone (before any file is read, nothing
written), `--check` (host only), the help text and the unknown-command message."""
import os
import subprocess

import pytest

from slacken_amd import capi
from test_host_cli import CLI, _built  # noqa: F401

USAGE = "usage: [--partitions N] build -i INDEX -t TAXONOMY_DIR -l LIBRARY_DIR"


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=60)


def test_usage_for_each_missing_required_option(tmp_path):
    i, t, l = ["-i", tmp_path / "out" / "lib"], ["-t", tmp_path / "tax"], ["-l", tmp_path / "k2"]
    for args in (t + l, i + l, i + t, i, []):
        r = cli("build", *args)
        assert r.returncode != 0 and USAGE in r.stderr and r.stdout == "" and "unknown command" not in r.stderr
    r = cli("build", *i, *t, *l, "--no-such-option")
    assert r.returncode != 0 and "unknown option --no-such-option" in r.stderr and USAGE in r.stderr
    assert os.listdir(tmp_path) == []


REFUSALS = [
    (["--ordering", "frequency"], "--ordering frequency is not supported"),
    (["--ordering", "lexicographic"], "--ordering lexicographic is not supported"),
    (["-k", "30", "-m", "31"], "-m must be <= -k"),
    (["-k", "40", "-m", "33"], "minimizers of up to 32 nt"),
    (["-k", "60", "-m", "31"], "windows of up to 28 m-mers (k - m + 1 = 30)"),
    (["-m", "20", "-k", "35", "--spaces", "11"], "at most 10"),
    (["--shard-table"], "--shard-table is not supported by build"),
    (["--devices", "0,1"], "build takes one device"),
    (["--devices", "all"], "build takes one device"),
    (["--format", "orc"], "parquet or slkrec"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=[" ".join(e) for e, _ in REFUSALS])
def test_refusals_read_no_file_and_write_nothing(tmp_path, extra, message):
    """the taxonomy and the library do not exist: a command that read either would say so instead"""
    out = tmp_path / "out" / "lib"
    for check in ([], ["--check"]):
        r = cli("build", "-i", out, "-t", tmp_path / "no_tax", "-l", tmp_path / "no_lib", *extra, *check)
        assert r.returncode != 0 and message in r.stderr and r.stdout == "", r.stderr
        assert "no_tax" not in r.stderr and "no_lib" not in r.stderr
    assert os.listdir(tmp_path) == []
    r = cli("--partitions", "0", "build", "-i", out, "-t", tmp_path / "no_tax", "-l", tmp_path / "no_lib")
    assert r.returncode != 0 and "--partitions must be positive" in r.stderr and os.listdir(tmp_path) == []


def write_fna(path, records):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for sid, seq in records:
            f.write(f">{sid} some organism\n" + "\n".join(seq[j:j + 60] for j in range(0, len(seq), 60)) + "\n")


def test_check(tmp_path):
    """a sequence id has no minimizer exactly when none of its records has a run of k valid bases"""
    good = "ACGT" * 20                                               # 80 valid bases
    broken = ("ACGTACGTAC" * 3 + "ACGT" + "N") * 4                   # runs of 34: one short of k = 35
    lib = tmp_path / "k2"
    write_fna(str(lib / "library" / "a" / "one.fna"),
              [("seq_good", good), ("seq_short", "ACGTACGT"), ("seq_broken_by_n", broken), ("seq_lower", good.lower()),
               ("a_sequence_id_of_more_than_twenty_characters", "NNNNNNNNNN" * 5)])
    write_fna(str(lib / "library" / "b" / "deep" / "two.fna"), [("seq_twice", "ACGT"), ("seq_twice", good), ("seq_exact", "A" * 34 + "c")])
    (lib / "library" / "ignored.fa").write_text(">not_read\nAC\n")
    out = tmp_path / "out" / "lib"
    r = cli("build", "-i", out, "-t", tmp_path / "no_tax", "-l", lib, "--check")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    mask = capi.DEFAULT_TOGGLE_MASK - (1 << 64) if capi.DEFAULT_TOGGLE_MASK >> 63 else capi.DEFAULT_TOGGLE_MASK
    assert lines[0] == f"Splitter randomXOR k=35 m=31 XORmask={mask} canonical=true minimizerSpaces=7"
    assert lines[1] == "Some input sequences had no minimizers (total 3): "
    assert lines[2:] == ["+--------------------+---+",
                         "|               seqId|sum|",
                         "+--------------------+---+",
                         "|a_sequence_id_of_...|  0|",
                         "|     seq_broken_by_n|  0|",
                         "|           seq_short|  0|",
                         "+--------------------+---+", "", ""]
    # with k = 34 the broken sequence has windows; with the short ones gone all have
    r = cli("build", "-i", out, "-t", tmp_path / "no_tax", "-l", lib, "--check", "-k", "34")
    assert r.returncode == 0 and "(total 2): " in r.stdout and "seq_broken_by_n" not in r.stdout
    os.remove(lib / "library" / "a" / "one.fna")
    write_fna(str(lib / "library" / "a" / "one.fna"), [("seq_good", good), ("seq_lower", good.lower())])
    r = cli("build", "-i", out, "-t", tmp_path / "no_tax", "-l", lib, "--check")
    assert r.returncode == 0 and r.stdout.split("\n")[1:] == ["Input sequences checked, all had minimizers.", ""]
    assert sorted(os.listdir(tmp_path)) == ["k2"]                    # nothing was written
    r = cli("build", "-i", out, "-t", tmp_path / "no_tax", "-l", tmp_path / "no_lib", "--check")
    assert r.returncode != 0 and "no such directory" in r.stderr


def test_help_and_unknown_command():
    help_text = cli("--help").stdout
    assert "slacken-amd [--partitions N] build -i INDEX -t TAXONOMY_DIR -l LIBRARY_DIR [-k 35] [-m 31] [-s|--spaces 7] [--check]" in help_text
    assert "SLK_BUILD_BATCH_BASES" in help_text and "SLK_EXPORT_PIECE_BUCKETS" in help_text
    assert "slacken-amd respace -i INDEX -o OUTPUT --spaces S" in help_text
    r = cli("no-such-command")
    assert r.returncode != 0
    for part in ("`build`", "`respace`", "`stats -i INDEX` and `inspect -i INDEX -o OUTPUT`", "unknown command"):
        assert part in r.stderr
    assert "build" in cli().stderr
