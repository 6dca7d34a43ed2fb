"""`classify --split-long LEN --split-hits` through the command line: contig-length records are split over many waves also where
per-read lines are written (hit lists on the piece route), and the files of the run -- per-read lines, Kraken reports --
are those of the same command without the flags, byte for byte; --split-hits is refused, before any device is opened, where it does
not apply."""
import glob
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from test_config1 import NAMES, load
from test_host_cli import CLI, ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = (9000, 12500, 17000, 21000, 26000, 30000)


def run(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def contigs(tmp_path_factory):
    """test_gpu_pieces_cli.py's recipe: the config1 library in Slacken's on-disk layout, and a FASTA of six contig-length records strung
    together from its reads, one with a run of Ns across the border between its first two pieces, plus 50 short records"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import parquet_to_slkrec as conv
    d = tmp_path_factory.mktemp("pieces_hits_cli")
    exp, lib, _, _ = load()
    loc = str(d / "mini_35_31_s7")
    conv.write_parquet_dir(loc, lib["keys"], lib["taxa"], buckets=4)
    with open(loc + ".properties", "w") as f:
        f.write(f"k={exp['k']}\nm={exp['m']}\nbuckets=4\nversion=1\nsplitter=randomXOR\nminimizerSpaces={exp['spaces']}\ncanonical=true\n")
    os.makedirs(loc + "_taxonomy")
    with open(loc + "_taxonomy/nodes.dmp", "w") as f:
        for t, par, r in [(1, 1, "no rank")] + [(t, 1, NAMES[t][1]) for t in exp["taxa"]]:
            f.write(f"{t}\t|\t{par}\t|\t{r}\t|\n")
    with open(loc + "_taxonomy/names.dmp", "w") as f:
        for t, nm in [(1, "root")] + [(t, NAMES[t][0]) for t in exp["taxa"]]:
            f.write(f"{t}\t|\t{nm}\t|\t\t|\tscientific name\t|\n")
    seqs = [l.strip() for l in gzip.open(os.path.join(GOLD, "config1_reads.fasta.gz"), "rt") if l.strip() and not l.startswith(">")]
    rng = np.random.default_rng(16)
    records = []
    for i, n in enumerate(LENGTHS):
        parts, have = [], 0
        while have < n:
            parts.append(seqs[int(rng.integers(0, len(seqs)))])
            have += len(parts[-1])
        s = "".join(parts)[:n]
        if i == 2:
            s = s[:4096 - 20] + "N" * 60 + s[4096 + 40:]      # pieces of 4 096 windows: the run lies across the first border
        records.append((f"contig{i}", s))
    records += [(f"short{i}", seqs[int(rng.integers(0, len(seqs)))]) for i in range(50)]
    fa = d / "SRR094926_contigs.fasta"
    with open(fa, "w") as f:
        for title, s in records:
            f.write(f">{title}\n{s}\n")
    return loc, fa, d


def tree(out):
    files = {}
    for path in sorted(glob.glob(f"{out}_c*/**", recursive=True)):
        if os.path.isfile(path):
            data = gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()
            files[os.path.relpath(path, os.path.dirname(str(out)))[len(os.path.basename(str(out))):]] = data
    return files


def test_split_hits_writes_the_same_files(contigs):
    loc, fa, d = contigs
    plain, split = d / "plain" / "out", d / "split" / "out"
    ran = "slk split: 6 fragments, %d pieces" % sum(-(-(n - 34) // 4096) for n in LENGTHS)
    for out, extra in ((plain, ()), (split, ("--split-long", "8193", "--split-hits"))):
        r = run("classify", "-i", loc, "-o", out, "-c", "0.0", "0.1", *extra, fa, env={"SLK_PIECE_WINDOWS": "4096", "SLK_DEBUG_SPLIT": "1"})
        assert r.returncode == 0, r.stderr
        assert (ran in r.stderr) == bool(extra), r.stderr
        assert ("slk split:" in r.stderr) == bool(extra), r.stderr
        assert "has no effect" not in r.stderr, r.stderr
    want, got = tree(plain), tree(split)
    assert want and sorted(want) == sorted(got)
    assert any(k.endswith("_kreport.txt") for k in want) and any(k.endswith(".txt.gz") for k in want)
    for k in want:
        assert got[k] == want[k], k
    lines = b"".join(v for k, v in want.items() if k.endswith(".txt.gz")).decode().splitlines()
    assert sum("contig" in l for l in lines) == 2 * len(LENGTHS)          # (two thresholds: the contigs' per-read lines are among them)


def test_split_hits_is_refused_where_it_does_not_apply(contigs):
    loc, fa, d = contigs
    # HIP_VISIBLE_DEVICES names no device: a run that got as far as opening one would say so instead
    cases = ((("--split-hits",), "--split-long"),                                           # alone
             (("--split-long", "0", "--split-hits"), "--split-long"),                       # ... or with the route off
             (("--split-long", "8193", "--split-hits", "-p", fa), "-p"),
             (("--split-long", "8193", "--split-hits", "--shard-table"), "--shard-table"))
    for extra, word in cases:
        r = run("classify", "-i", loc, "-o", d / "refused" / "out", *extra, fa, env={"HIP_VISIBLE_DEVICES": "-1"})
        assert r.returncode != 0 and word in r.stderr and "split" in r.stderr, (extra, r.stderr)
        assert not glob.glob(str(d / "refused" / "*"))
    r = run("classify2", "-i", loc, "-o", d / "refused" / "out", "--library", d, "--split-hits", fa, env={"HIP_VISIBLE_DEVICES": "-1"})
    assert r.returncode != 0 and "split" in r.stderr and "classify2" in r.stderr, r.stderr
    assert not glob.glob(str(d / "refused" / "*"))


def test_help_names_the_flag():
    r = run("--help")
    assert "--split-hits" in r.stdout + r.stderr
