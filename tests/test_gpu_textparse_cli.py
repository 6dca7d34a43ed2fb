"""The device parser through the command line: `parse --device` prints what `parse` prints, `classify --device-parse` writes the files
`classify` writes, byte for byte, and the flag is refused where it does not apply."""
import glob
import gzip
import os
import subprocess
import sys

import pytest

from test_config1 import NAMES, load
from test_host_cli import CLI, ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cli(*args, env=None):
    r = subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("chunk", ["4096", None], ids=["chunk4096", "default_chunk"])
@pytest.mark.parametrize("name", ["config1_reads.fasta.gz", "config1_reads2.fastq.gz", "akashinriki_10k.fasta.gz"])
def test_parse_device_equals_parse(name, chunk):
    path = os.path.join(GOLD, name)
    want = cli("parse", path)
    assert want.count("\n") >= 1 and len(want) > 10000   # (the third file is one record of 10 kbp)
    got = cli("parse", "--device", path, env={"SLK_IO_CHUNK": chunk} if chunk else None)
    assert got == want


@pytest.fixture(scope="module")
def config1(tmp_path_factory):
    """the config1 library in Slacken's on-disk layout, and its two read files under names that carry a sample id"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import parquet_to_slkrec as conv
    d = tmp_path_factory.mktemp("config1")
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
    fa, fq = d / "SRR094926_10k.fasta.gz", d / "ERR599052_10k.fastq.gz"
    fa.write_bytes(open(os.path.join(GOLD, "config1_reads.fasta.gz"), "rb").read())
    fq.write_bytes(open(os.path.join(GOLD, "config1_reads2.fastq.gz"), "rb").read())
    plain = d / "ERR599052_10k.fastq"
    plain.write_bytes(gzip.open(fq, "rb").read())
    return loc, [fa, fq, plain], d


def tree(out):
    """every file under the output locations of a run: per-read files after gunzip, reports as they are"""
    files = {}
    for path in sorted(glob.glob(f"{out}_c*/**", recursive=True)):
        if os.path.isfile(path):
            data = gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()
            files[os.path.relpath(path, os.path.dirname(str(out)))[len(os.path.basename(str(out))):]] = data
    return files


def same_files(loc, d, tag, flags, file, chunk):
    host, dev = d / f"host_{tag}" / "out", d / f"dev_{tag}" / "out"
    cli("classify", "-i", loc, "-o", host, *flags, file)
    cli("classify", "-i", loc, "-o", dev, "--device-parse", *flags, file, env={"SLK_IO_CHUNK": chunk} if chunk else None)
    want, got = tree(host), tree(dev)
    assert want and sorted(want) == sorted(got)
    assert any(k.endswith("_kreport.txt") for k in want)
    assert any(k.endswith(".txt.gz") for k in want) == ("--nodetailed" not in flags)
    for k in want:
        assert got[k] == want[k], k


# (one input file per run: several files are read side by side by the host parser and one after the other by this route, so the
#  order of the lines differs between the two, as it may between two runs of the reference)
@pytest.mark.parametrize("flags", [(), ("--sample-regex", r"\.(\d)"), ("--nodetailed",)], ids=["plain", "sample_regex", "nodetailed"])
def test_classify_device_parse_writes_the_same_files(config1, flags):
    loc, files, d = config1
    tag = flags[0].strip("-") if flags else "plain"
    for i, file in enumerate(files[:2]):   # the gzipped FASTA and FASTQ files, several chunks each
        same_files(loc, d, f"{tag}{i}", flags, file, "65536")


def test_plain_file_is_mapped_and_cut_in_place(config1):
    """a plain file is not read through the chunk buffer: its chunks are ranges of the mapping, cut where the records end"""
    loc, files, d = config1
    same_files(loc, d, "default_chunk", ("-c", "0.0", "0.15"), files[2], None)
    same_files(loc, d, "small_chunks", (), files[2], "65536")
    want = cli("parse", files[2])
    for chunk in ("4096", "1000", None):
        assert cli("parse", "--device", files[2], env={"SLK_IO_CHUNK": chunk} if chunk else None) == want


def refused(*args):
    r = subprocess.run([CLI, *map(str, args)], capture_output=True, text=True)
    assert r.returncode != 0
    return r.stderr


def test_the_four_refusals(config1, tmp_path):
    loc, files, d = config1
    o = tmp_path / "o"
    assert "unpaired" in refused("classify", "-i", loc, "-o", o, "-p", "--device-parse", files[1], files[1])
    assert "--shard-table" in refused("classify", "-i", loc, "-o", o, "--shard-table", "--device-parse", files[1])
    assert "classify2" in refused("classify2", "-i", loc, "-o", o, "--library", d, "--device-parse", files[1])
    wide = str(tmp_path / "wide")
    with open(wide + ".properties", "w") as f:
        f.write("k=63\nm=45\nversion=1\nsplitter=randomXOR\nminimizerSpaces=7\n")
    assert "m=45" in refused("classify", "-i", wide, "-o", o, "--device-parse", files[1])
    assert not glob.glob(f"{o}*")
