"""`slacken-amd merge` and `build --base` end to end on the world of test_host_classify2_gpu.setup: its sequences are split into two
genome directories that both hold sequences of every genome, each half is built into a library, and the two libraries merged -- or
one of them taken as the base of a build of the other half -- must be on disk what `build` of the whole writes and what the oracle's
build_records gives.  Then the merged library in use, the seams, and destinations with another taxonomy."""
import filecmp
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import merge_model as mm
import stats_model as sm
from test_build_cli import write_fna
from test_gpu_build_cli import records_of, same
from test_gpu_respace_cli import counts_of, on_disk
from test_host_classify2_gpu import setup
from test_host_classify_gpu import read_out
from test_host_cli import CLI
from test_respace_cli import murmur3_long

pytestmark = pytest.mark.gpu


def cli(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240,
                          env=None if env is None else dict(os.environ, **env))


def in_a(i):
    """of each genome's three sequences the short middle one and, by turns, the first or the last: both halves hold sequences of every
    genome, and the stretch that all genomes share (in their first sequences) lies in both"""
    genome, part = divmod(i, 3)
    return part == 1 or (part == 0) == (genome % 2 == 0)


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("merge")
    S = setup(tmp, orc)
    S["tmp"], S["orc"], S["taxdir"] = tmp, orc, S["loc"] + "_taxonomy"
    for name, keep in (("a", in_a), ("b", lambda i: not in_a(i))):
        lib = tmp / f"k2_{name}"
        idx = [i for i in range(len(S["seqs"])) if keep(i)]
        write_fna(str(lib / "library" / "x" / "one.fna"), [(S["seq_ids"][i], S["seqs"][i]) for i in idx[::2]])
        write_fna(str(lib / "library" / "y" / "two.fna"), [(S["seq_ids"][i], S["seqs"][i]) for i in idx[1::2]])
        with open(lib / "seqid2taxid.map", "w") as f:
            f.write("".join(f"{S['seq_ids'][i]}\t{S['seq_taxa'][i]}\n" for i in idx))
        S[f"k2_{name}"] = str(lib)
        S[name] = str(tmp / "built" / name)
        r = cli("--partitions", 3, "build", "-i", S[name], "-t", S["taxdir"], "-l", lib)
        assert r.returncode == 0, r.stderr
        S[f"rec_{name}"] = on_disk(S[name])
        assert same(S[f"rec_{name}"], records_of(orc, S, S["p"], keep=keep))
    S["whole"] = str(tmp / "built" / "whole")
    r = cli("--partitions", 5, "build", "-i", S["whole"], "-t", S["taxdir"], "-l", S["lib"])
    assert r.returncode == 0, r.stderr
    S["want"] = records_of(orc, S, S["p"])
    shared = len(S["rec_a"][0]) + len(S["rec_b"][0]) - len(S["want"][0])
    assert shared >= 300                        # (the stretch of 1 500 bases that the genomes share: about 2 / (w + 1) = a third as many keys)
    S["two_lines"] = sm.stats(S["tax"], counts_of(S["want"][1]), 31, False)
    S["m"] = str(tmp / "merged" / "m")
    S["run"] = cli("--partitions", 5, "merge", "-i", S["m"], S["a"], S["b"])
    return S


def test_merged_library_is_the_whole(world):
    r, out = world["run"], world["m"]
    assert r.returncode == 0, r.stderr
    assert same(on_disk(out), on_disk(world["whole"])) and same(on_disk(out), world["want"]) and len(world["want"][0]) > 10_000
    files = sorted(glob.glob(os.path.join(out, "*.parquet")))
    assert [os.path.basename(f)[-26:] for f in files] == [f"_{b:05d}.c000.snappy.parquet" for b in range(5)] == [f[-26:] for f in sorted(os.listdir(out))]
    import pyarrow.parquet as pq
    seen = 0
    for b, f in enumerate(files):
        keys = pq.read_table(f).column("id1").to_numpy().tolist()
        assert keys and all(murmur3_long(k) % 5 == b for k in keys)      # every key in its Spark bucket
        seen += len(keys)
    assert seen == len(world["want"][0])
    assert open(out + ".properties").read() == open(world["whole"] + ".properties").read() and "buckets=5\n" in open(out + ".properties").read()
    names = sorted(os.listdir(world["taxdir"]))
    assert names == sorted(os.listdir(out + "_taxonomy")) == ["names.dmp", "nodes.dmp"]
    assert all(filecmp.cmp(os.path.join(world["taxdir"], n), os.path.join(out + "_taxonomy", n), shallow=False) for n in names)
    assert not os.path.exists(out + ".writing") and not os.path.exists(out + ".slkrec")
    # stdout: the two lines `stats` prints of the whole
    s = cli("stats", "-i", world["whole"])
    assert s.returncode == 0 and s.stdout.endswith(world["two_lines"]) and r.stdout == world["two_lines"] and r.stdout.count("\n") == 2
    assert f"{world['a']} {len(world['rec_a'][0])}, {world['b']} {len(world['rec_b'][0])}; {len(world['want'][0])} records out" in r.stderr


def test_the_other_order_and_three_sources(world):
    out = str(world["tmp"] / "merged" / "ba")
    r = cli("--partitions", 2, "merge", "-i", out, world["b"], world["a"], "--format", "slkrec")
    assert r.returncode == 0, r.stderr
    assert not os.path.isdir(out) and same(on_disk(out), world["want"]) and r.stdout == world["two_lines"]
    assert "buckets=2\n" in open(out + ".properties").read()
    out3 = str(world["tmp"] / "merged" / "aba")
    r = cli("merge", "-i", out3, "-t", world["taxdir"], world["a"], world["m"], world["b"], "--format", "slkrec")
    assert r.returncode == 0 and same(on_disk(out3), world["want"]), r.stderr


def test_build_with_a_base(world):
    out = str(world["tmp"] / "based" / "lib")
    r = cli("--partitions", 5, "build", "-i", out, "-t", world["taxdir"], "-l", world["k2_b"], "--base", world["a"])
    assert r.returncode == 0, r.stderr
    assert same(on_disk(out), world["want"])
    whole_stdout = cli("--partitions", 5, "build", "-i", str(world["tmp"] / "based" / "again"), "-t", world["taxdir"], "-l", world["lib"],
                       "--format", "slkrec").stdout
    first = whole_stdout.split("\n")[0] + "\n"
    assert whole_stdout.startswith(first + world["two_lines"]) and r.stdout.startswith(first + world["two_lines"])
    assert f"--base {world['a']}: {len(world['rec_a'][0])} records merged" in r.stderr
    assert open(out + ".properties").read() == open(world["whole"] + ".properties").read()
    # the other way round, and the base's splitter repeated on the command line
    out2 = str(world["tmp"] / "based" / "lib2")
    r = cli("build", "-i", out2, "-t", world["taxdir"], "-l", world["k2_a"], "--base", world["b"], "-k", 35, "-m", 31, "-s", 7, "--format", "slkrec")
    assert r.returncode == 0 and same(on_disk(out2), world["want"]), r.stderr


def test_classify_with_the_merged_library(world):
    res = {}
    for name, loc in (("merged", world["m"]), ("whole", world["whole"])):
        res[name] = str(world["tmp"] / f"classified_{name}" / "r")
        r = cli("classify", "-i", loc, "-o", res[name], world["fq"])
        assert r.returncode == 0, r.stderr
    lines = read_out(res["merged"] + "_c0.0")
    assert lines == read_out(res["whole"] + "_c0.0") and sum(1 for l in lines if l.startswith("C")) >= 500
    assert open(res["merged"] + "_c0.0/all_kreport.txt", "rb").read() == open(res["whole"] + "_c0.0/all_kreport.txt", "rb").read()


@pytest.mark.parametrize("seam", ["pieces", "growth", "slkrec"])
def test_seams_give_the_same_records(world, seam):
    out = str(world["tmp"] / f"seam_{seam}" / "lib")
    env, extra = {"pieces": ({"SLK_EXPORT_PIECE_BUCKETS": "300"}, []), "growth": ({}, ["--expected-records", 1024]),
                  "slkrec": ({}, ["--format", "slkrec"])}[seam]
    r = cli("--partitions", 5, "merge", "-i", out, world["a"], world["b"], *extra, env=env)
    assert r.returncode == 0, r.stderr
    assert same(on_disk(out), world["want"]) and r.stdout == world["two_lines"]
    if seam == "pieces":
        assert int(r.stderr.split(" s in ")[1].split(" pieces")[0]) >= 10
    if seam == "growth":
        assert int(r.stderr.split("(table grown ")[1].split(" times")[0]) >= 1
    if seam == "slkrec":
        assert not os.path.isdir(out) and os.path.exists(out + ".slkrec")


def other_taxonomy(world, name, without, merged=None):
    """the world's taxonomy files without the node `without`; merged = the node merged.dmp sends it to"""
    d = str(world["tmp"] / name)
    os.makedirs(d)
    rows = [l for l in open(os.path.join(world["taxdir"], "nodes.dmp")).read().split("\n") if l and int(l.split("|")[0]) != without]
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        f.write("\n".join(rows) + "\n")
    os.symlink(os.path.join(world["taxdir"], "names.dmp"), os.path.join(d, "names.dmp"))
    if merged is not None:
        with open(os.path.join(d, "merged.dmp"), "w") as f:
            f.write(f"{without}\t|\t{merged}\t|\n")
    parents = np.array(world["parents"], np.int32)
    parents[without] = 0
    return d, mm.Tax(parents.tolist(), [(without, merged)] if merged is not None else ())


def test_a_destination_taxonomy_that_merged_a_species(world):
    gone, into = world["seq_taxa"][0], world["seq_taxa"][3]           # two species with sequences in A and in B
    assert gone != into and (world["rec_a"][1] == gone).sum() > 100
    taxdir, dst = other_taxonomy(world, "tax_merged", gone, into)
    remap, identity = mm.taxon_remap(mm.Tax(list(world["parents"])), dst)
    assert not identity and remap[gone] == into
    want = mm.as_arrays(mm.merge(dst.parents, [world["rec_a"], world["rec_b"]], remaps=[remap, remap]))
    assert gone not in want[1] and not same(want, world["want"])
    out = str(world["tmp"] / "retaxed" / "lib")
    r = cli("merge", "-i", out, "-t", taxdir, world["a"], world["b"], "--format", "slkrec")
    assert r.returncode == 0, r.stderr
    assert same(on_disk(out), want)
    assert sorted(os.listdir(out + "_taxonomy")) == ["merged.dmp", "names.dmp", "nodes.dmp"]


def test_a_destination_taxonomy_that_lacks_a_species(world):
    gone = world["seq_taxa"][0]
    taxdir, _ = other_taxonomy(world, "tax_lacking", gone)
    out = str(world["tmp"] / "lacking" / "lib")
    r = cli("merge", "-i", out, "-t", taxdir, world["a"], world["b"])
    n_bad = int((world["rec_a"][1] == gone).sum())
    assert r.returncode != 0 and r.stdout == ""
    # (the run ends with the first batch of A's records that holds such a taxon: its count, at most all of A's)
    said = re.search(re.escape(world["a"]) + r": (\d+) records name a taxon the destination's taxonomy does not define \(smallest: (\d+)\)", r.stderr)
    assert said and 0 < int(said.group(1)) <= n_bad and int(said.group(2)) == gone, r.stderr
    parent = os.path.dirname(out)
    assert not os.path.exists(out) and not os.path.exists(out + ".properties") and not os.path.exists(out + ".writing")
    assert not os.path.exists(parent) or os.listdir(parent) == []
    # build --base ends the same way
    r = cli("build", "-i", out, "-t", taxdir, "-l", world["k2_b"], "--base", world["a"])
    assert r.returncode != 0 and "records name a taxon the destination's taxonomy does not define" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".properties") and not os.path.exists(out + ".writing")
