"""The paired device route through the command line: `classify -p --device-pairs` writes the files `classify -p` writes, byte for byte,
on pairs made from the config1 reads, and ends with a message where the mates are out of order."""
import gzip
import os
import subprocess

import pytest

import hostmodel
from test_gpu_textparse_cli import GOLD, cli, config1, tree   # noqa: F401  (config1 is a fixture)
from test_host_cli import CLI

pytestmark = pytest.mark.gpu

N_PAIRS = 1500


@pytest.fixture(scope="module")
def halves():
    """[(title, first half, second half)] of the first config1 FASTQ reads: each read's second half is its mate"""
    text = gzip.open(os.path.join(GOLD, "config1_reads2.fastq.gz"), "rt").read()
    recs = hostmodel.parse_fastq(text)[:N_PAIRS]
    assert len(recs) == N_PAIRS and len({t for t, _ in recs}) == N_PAIRS
    return [(t, s[:len(s) // 2], s[len(s) // 2:]) for t, s in recs]


def fastq(records):
    return "".join(f"@{t}\n{s}\n+\n{'I' * len(s)}\n" for t, s in records)


def fasta(records):
    return "".join(f">{t}\n{s[:40]}\n{s[40:]}\n" for t, s in records)


def write(path, text):
    if str(path).endswith(".gz"):
        with gzip.open(path, "wt") as f:
            f.write(text)
    else:
        path.write_text(text)
    return path


def mates(halves, suffixes=("/1", "/2"), desc=" a description"):
    return ([(t + suffixes[0] + desc, a) for t, a, _ in halves], [(t + suffixes[1] + desc, b) for t, _, b in halves])


def same_files(loc, d, tag, flags, files, chunk, ordered=True):
    host, dev = d / f"pair_host_{tag}" / "out", d / f"pair_dev_{tag}" / "out"
    cli("classify", "-i", loc, "-o", host, "-p", *flags, *files)
    cli("classify", "-i", loc, "-o", dev, "-p", "--device-pairs", *flags, *files, env={"SLK_IO_CHUNK": chunk} if chunk else None)
    want, got = tree(host), tree(dev)
    assert want and sorted(want) == sorted(got)
    assert any(k.endswith("_kreport.txt") for k in want)
    assert any(k.endswith(".txt.gz") for k in want) == ("--nodetailed" not in flags)
    for k in want:
        if ordered or not k.endswith(".txt.gz"):
            assert got[k] == want[k], k
        else:   # several file pairs: their batches interleave differently, as they may between two runs of the reference
            assert sorted(got[k].split(b"\n")) == sorted(want[k].split(b"\n")), k
    return want


CASES = {
    "plain_suffixes_4096": ((".fastq", ".fastq"), ("/1", "/2"), (), "4096"),
    "gz_no_suffixes_65536": ((".fastq.gz", ".fastq.gz"), ("", ""), ("--sample-regex", r"\.(\d)"), "65536"),
    "fasta_fastq_default": ((".fasta", ".fastq"), ("/1", ""), ("--nodetailed",), None),
    "gz_two_thresholds": ((".fasta.gz", ".fastq.gz"), ("", "/2"), ("-c", "0.0", "0.15"), "65536"),
    "plain_default": ((".fastq", ".fastq"), ("/1", "/2"), (), None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_pairs_writes_the_same_files(config1, halves, case):
    loc, _, d = config1
    exts, suffixes, flags, chunk = CASES[case]
    r1, r2 = mates(halves, suffixes)
    f1 = write(d / f"ERR599052_{case}_1{exts[0]}", (fasta if "fasta" in exts[0] else fastq)(r1))
    f2 = write(d / f"ERR599052_{case}_2{exts[1]}", (fasta if "fasta" in exts[1] else fastq)(r2))
    want = same_files(loc, d, case, flags, (f1, f2), chunk)
    if "--nodetailed" not in flags:
        assert sum(v.count(b"\n") for k, v in want.items() if k.endswith(".txt.gz")) >= N_PAIRS // 2   # (a row per fragment with a span)


@pytest.mark.parametrize("side", [1, 2])
def test_surplus_at_the_end_of_a_file(config1, halves, side):
    """what one file holds beyond the other's end becomes no fragment; a surplus title of file 1 that repeats a paired title sends that
    title through the regrouping of repeated titles, on both routes"""
    loc, _, d = config1
    r1, r2 = mates(halves)
    extra = [(halves[3][0] + "/%d" % side, halves[7][1] + halves[7][2]), ("ERR599052.surplus/%d" % side, halves[9][1])] + \
            [(f"ERR599052.more{i}/{side}", halves[i][2]) for i in range(40)]
    if side == 1:
        r1 = r1 + extra
    else:
        r2 = r2 + extra
    f1 = write(d / f"surplus{side}_1.fastq", fastq(r1))
    f2 = write(d / f"surplus{side}_2.fastq.gz", fastq(r2))
    same_files(loc, d, f"surplus{side}", (), (f1, f2), "4096")


def test_two_file_pairs_in_one_run(config1, halves):
    loc, _, d = config1
    files = []
    for k, part in enumerate((halves[:700], halves[700:])):
        r1, r2 = mates(part)
        files += [write(d / f"two_{k}_1.fastq", fastq(r1)), write(d / f"two_{k}_2.fastq.gz", fastq(r2))]
    same_files(loc, d, "two_pairs", ("--sample-regex", r"\.(\d)"), files, "65536", ordered=False)


def test_mates_out_of_order_end_the_run(config1, halves, tmp_path):
    loc, _, d = config1
    r1, r2 = mates(halves[:400], desc="")
    j = 301
    r2[j], r2[j + 1] = r2[j + 1], r2[j]
    f1, f2 = write(tmp_path / "ooo_1.fastq", fastq(r1)), write(tmp_path / "ooo_2.fastq", fastq(r2))
    o = tmp_path / "o"
    r = subprocess.run([CLI, "classify", "-i", loc, "-o", str(o), "-p", "--device-pairs", str(f1), str(f2)], capture_output=True, text=True,
                       env=dict(os.environ, SLK_IO_CHUNK="4096"))
    assert r.returncode != 0
    msg = [line for line in r.stderr.splitlines() if "out of order" in line]
    assert len(msg) == 1, r.stderr
    assert str(f1) in msg[0] and str(f2) in msg[0] and f"pair {j + 1} " in msg[0]
    assert f"'{halves[j][0]}'" in msg[0] and f"'{halves[j + 1][0]}'" in msg[0] and "without --device-pairs" in msg[0]
    # the host route joins them
    cli("classify", "-i", loc, "-o", o, "-p", f1, f2)
    assert tree(o)
