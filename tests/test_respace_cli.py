"""The library writer without a GPU: `slacken-amd copy-records` reads the golden library with the readers and writes it with the
writer (library_writer.hpp, parquet_sink.cpp), and what it wrote is read back with pyarrow and with the project's own converter.
And the command line of `respace`, whose errors come before any GPU call."""
import filecmp
import glob
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import CLI
from test_host_classify_gpu import GOLD, make_library   # (puts tools/ on sys.path: parquet_to_slkrec)


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=120)


def murmur3_long(v, seed=42):
    """org.apache.spark.unsafe.hash.Murmur3_x86_32.hashLong, restated independently of the writer"""
    M = 0xFFFFFFFF

    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & M

    def mix_k1(k):
        return (rotl((k * 0xcc9e2d51) & M, 15) * 0x1b873593) & M

    def mix_h1(h, k):
        return (rotl(h ^ k, 13) * 5 + 0xe6546b64) & M
    v &= (1 << 64) - 1
    h = mix_h1(mix_h1(seed, mix_k1(v & M)), mix_k1(v >> 32))
    h ^= 8
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M
    h ^= h >> 16
    return h - (1 << 32) if h >> 31 else h


def records_sorted(keys, taxa):
    o = np.argsort(keys, kind="stable")
    return keys[o], taxa[o]


def bucket_files(loc):
    return sorted(glob.glob(os.path.join(loc, "*.parquet")))


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("golden")
    g, loc, tax, _ = make_library(tmp, convert=False)   # (the Parquet files alone: 7 buckets)
    lib = np.load(os.path.join(GOLD, "library.npz"))
    return dict(tmp=tmp, loc=loc, keys=lib["keys"], taxa=lib["taxa"], props=cli("props", loc).stdout)


def same_taxonomy(a, b):
    cmp = filecmp.dircmp(a, b)
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)) and not cmp.diff_files and not cmp.funny_files
    assert all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in names)


def test_copy_records_parquet_to_parquet(golden):
    import parquet_to_slkrec as conv
    import pyarrow.parquet as pq
    want = records_sorted(golden["keys"], golden["taxa"])
    placed = []
    for run in ("a", "b"):
        out = str(golden["tmp"] / f"copy_{run}" / "lib_s7")
        r = cli("copy-records", "-i", golden["loc"], "-o", out, "--format", "parquet")
        assert r.returncode == 0, r.stderr
        files = bucket_files(out)
        assert len(files) == 7                                        # buckets=7 in the golden library's properties
        assert [os.path.basename(f)[-26:] for f in files] == [f"_{b:05d}.c000.snappy.parquet" for b in range(7)]
        where = {}
        for b, f in enumerate(files):
            t = pq.read_table(f)
            assert t.column_names == ["id1", "taxon"] and str(t.schema.field("id1").type) == "int64" and str(t.schema.field("taxon").type) == "int32"
            assert pq.ParquetFile(f).metadata.row_group(0).column(0).compression == "SNAPPY"
            for k in t.column("id1").to_numpy().tolist():
                assert k not in where                                  # every key in exactly one file
                where[k] = b
                assert b == murmur3_long(k) % 7                        # ... Spark's bucket (Python's % is pmod)
        placed.append(where)
        got = conv.read_parquet_dir(out)
        assert all(np.array_equal(a, b) for a, b in zip(records_sorted(*got), want))
        assert cli("props", out).stdout == golden["props"] != ""
        assert "buckets=7\n" in open(out + ".properties").read()
        same_taxonomy(golden["loc"] + "_taxonomy", out + "_taxonomy")
        assert not os.path.exists(out + ".writing") and not os.path.exists(out + ".slkrec")
        assert cli("records", out).stdout == cli("records", golden["loc"]).stdout.split("\n")[0] + "\n"
    assert placed[0] == placed[1] and len(set(placed[0].values())) == 7


def test_copy_records_parquet_to_slkrec_and_back(golden):
    import parquet_to_slkrec as conv
    want = records_sorted(golden["keys"], golden["taxa"])
    out = str(golden["tmp"] / "flat" / "lib_s7")
    r = cli("copy-records", "-i", golden["loc"], "-o", out, "--format", "slkrec")
    assert r.returncode == 0, r.stderr
    raw = open(out + ".slkrec", "rb").read()
    n = len(want[0])
    assert raw[:8] == b"SLKREC1\0" and np.frombuffer(raw[8:24], "<u8,<u4,<u4")[0].tolist() == (n, 1, int(golden["taxa"].max()))
    keys = np.frombuffer(raw[24:24 + 8 * n], np.int64)
    taxa = np.frombuffer(raw[24 + 8 * n:], np.int32)
    assert len(taxa) == n and all(np.array_equal(a, b) for a, b in zip(records_sorted(keys, taxa), want))
    assert not os.path.isdir(out) and cli("props", out).stdout == golden["props"]
    same_taxonomy(golden["loc"] + "_taxonomy", out + "_taxonomy")
    line = cli("records", out).stdout
    assert line.startswith("slkrec n=%d " % n) and line.split(" ", 1)[1] == cli("records", golden["loc"]).stdout.split("\n")[0].split(" ", 1)[1] + "\n"
    # slkrec -> parquet: the other reader into the same writer
    back = str(golden["tmp"] / "back" / "lib_s7")
    assert cli("copy-records", "-i", out, "-o", back).returncode == 0
    assert all(np.array_equal(a, b) for a, b in zip(records_sorted(*conv.read_parquet_dir(back)), want))


def test_copy_records_errors(golden, tmp_path):
    assert "usage: copy-records" in cli("copy-records", "-i", golden["loc"]).stderr
    assert "usage: copy-records" in cli("copy-records").stderr
    r = cli("copy-records", "-i", golden["loc"], "-o", tmp_path / "x_s7", "--format", "orc")
    assert r.returncode != 0 and "parquet or slkrec" in r.stderr and os.listdir(tmp_path) == []
    r = cli("copy-records", "-i", tmp_path / "no_such", "-o", tmp_path / "x_s7")
    assert r.returncode != 0 and os.listdir(tmp_path) == []
    # a source whose records end early: nothing that loads is left behind
    cut = str(tmp_path / "cut_s7")
    for suffix in (".properties",):
        open(cut + suffix, "w").write(open(golden["loc"] + ".properties").read())
    os.symlink(golden["loc"] + "_taxonomy", cut + "_taxonomy")
    full = str(golden["tmp"] / "flat" / "lib_s7.slkrec")
    if not os.path.exists(full):
        assert cli("copy-records", "-i", golden["loc"], "-o", full[:-7], "--format", "slkrec").returncode == 0
    raw = open(full, "rb").read()
    open(cut + ".slkrec", "wb").write(raw[:len(raw) - 1000])
    out = str(tmp_path / "out" / "cut_s7")
    r = cli("copy-records", "-i", cut, "-o", out)
    assert r.returncode != 0 and "truncated" in r.stderr
    assert not os.path.exists(out + ".properties") and not os.path.exists(out) and not os.path.exists(out + ".slkrec")
    assert cli("props", out).returncode != 0


def test_respace_command_line(golden, tmp_path):
    usage = "usage: respace -i INDEX -o OUTPUT --spaces S [S ...]"
    out = tmp_path / "o_s7"
    for args in (["-i", golden["loc"], "-o", out], ["-i", golden["loc"], "-o", out, "--spaces"], ["-o", out, "--spaces", "9"],
                 ["-i", golden["loc"], "--spaces", "9"], []):
        r = cli("respace", *args)
        assert r.returncode != 0 and usage in r.stderr and r.stdout == "" and "unknown command" not in r.stderr
    for bad in ("plain", "lib_sx", "lib_s", "s12"):
        r = cli("respace", "-i", golden["loc"], "-o", tmp_path / bad, "--spaces", "9", "12")
        assert r.returncode != 0 and r.stdout == ""
        assert f"Unable to guess the correct output location for new indexes at: {tmp_path / bad}" in r.stderr
    r = cli("respace", "-i", golden["loc"], "-o", out, "--spaces", "9", "--shard-table")
    assert r.returncode != 0 and "--shard-table is not supported by respace" in r.stderr
    for devices in ("0,1", "all"):
        r = cli("respace", "-i", golden["loc"], "-o", out, "--spaces", "9", "--devices", devices)
        assert r.returncode != 0 and "must fit one GPU" in r.stderr
    assert cli("respace", "-i", golden["loc"], "-o", out, "--spaces", "9", "--format", "orc").returncode != 0
    assert os.listdir(tmp_path) == []
    help_text = cli("--help").stdout
    assert "slacken-amd respace -i INDEX -o OUTPUT --spaces S" in help_text and "copy-records -i INDEX -o OUTPUT" in help_text
    r = cli("no-such-command")
    assert "`respace`" in r.stderr
