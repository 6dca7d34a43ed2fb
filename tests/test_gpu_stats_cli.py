"""`slacken-amd stats`, `stats --histogram` and `inspect --labels` end to end on the golden library (tests/golden/library.npz
written out in Slacken's on-disk layout, as test_host_classify_gpu.py does): the library goes to HBM, the records per taxon are
counted there, and what follows the splitter lines is compared byte for byte with stats_model.py fed with the library's own records."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import stats_model as sm
from test_host_cli import CLI
from test_host_classify_gpu import GOLD, make_library   # (puts tools/ on sys.path: parquet_to_slkrec)

pytestmark = pytest.mark.gpu


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240)


def splitter_lines(g):
    """Slacken.scala:291-302 with this engine's third line: SpacedSeed.spaceMask and RandomXOR.mask as Long.toBinaryString"""
    m, s = g["m"], g["spaces"]
    assert 0 < m < 32 and s > 0
    word = (1 << 64) - 1
    space = (word << ((32 - m) * 2)) & word
    for _ in range(s):
        space = ((space << 4) | (3 << (64 - m * 2))) & word
    xor = 0xe37e28c4271b5a2d
    signed = xor - (1 << 64)
    return (f"Spaced mask (left aligned) {space:b}\nToggle mask (left aligned) {(xor << (64 - m * 2)) & word:b}\n"
            f"Inner splitter randomXOR m={m} XORmask={signed} canonical=true\n")


def test_stats_and_inspect_on_the_golden_library(tmp_path):
    g, loc, tax, _ = make_library(tmp_path, convert=True)
    lib = np.load(os.path.join(GOLD, "library.npz"))
    taxa = lib["taxa"][lib["taxa"] != 0]
    t, c = np.unique(taxa, return_counts=True)
    counts = list(zip(t.tolist(), c.tolist()))
    assert len(counts) > 3 and json.load(open(os.path.join(GOLD, "golden_classify.json")))["m"] == g["m"]
    head = splitter_lines(g)

    r = cli("stats", "-i", loc)
    assert r.returncode == 0, r.stderr
    assert r.stdout == head + sm.stats(tax, counts, g["m"], False)
    r = cli("stats", "--index", loc, "--histogram", "--devices", "0")
    assert r.returncode == 0, r.stderr
    assert r.stdout == head + sm.stats(tax, counts, g["m"], True)

    # inspect: the golden library stores every taxon of its taxonomy, so a second copy is written without the records of seven taxa --
    # those are what a label file can name that the library lacks
    import parquet_to_slkrec as conv
    dropped = [a for a, _ in counts][-7:]
    keep = ~np.isin(lib["taxa"], dropped)
    loc2 = str(tmp_path / "golden_less")
    conv.write_parquet_dir(loc2, lib["keys"][keep], lib["taxa"][keep], buckets=3)
    shutil.copy(loc + ".properties", loc2 + ".properties")
    shutil.copytree(loc + "_taxonomy", loc2 + "_taxonomy")
    counts2 = [(a, n) for a, n in counts if a not in dropped]
    stored = [a for a, _ in counts2]
    labels_text = "".join(f"seq{i}\t{a}\n" for i, a in enumerate(stored[:5] + dropped + dropped[:2]))
    labels = tmp_path / "seqid2taxid.map"
    labels.write_text(labels_text)
    out = str(tmp_path / "reports" / "golden")
    r = cli("inspect", "-i", loc2, "-o", out, "--labels", labels)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    want = sm.reports(tax, counts2, labels_text)
    assert len(want["_missing_report.txt"].split("\n")) > 8
    for suffix in ("_min_report.txt", "_genome_report.txt", "_missing_report.txt"):
        assert open(out + suffix).read() == want[suffix], suffix
    out2 = str(tmp_path / "reports2" / "golden")
    assert cli("inspect", "-i", loc, "-o", out2).returncode == 0           # the whole library, no labels: two files
    assert open(out2 + "_min_report.txt").read() == sm.reports(tax, counts)["_min_report.txt"]
    assert open(out2 + "_genome_report.txt").read() == sm.reports(tax, counts)["_genome_report.txt"]
    assert not os.path.exists(out2 + "_missing_report.txt")
