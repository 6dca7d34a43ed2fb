"""`slacken-amd build` end to end on the library test_host_classify2_gpu.setup writes (three sequences per genome, Ns, line breaks,
two directories, a file that is not .fna): what is on disk against the oracle's build_records of the labelled sequences, what is
printed against stats_model.py and build_model.py, and the built library in use by `props`, `stats` and `classify`."""
import filecmp
import glob
import os
import subprocess

import numpy as np
import pytest

import build_model as bm
import hostmodel
import stats_model as sm
from test_gpu_respace_cli import counts_of, on_disk
from test_host_classify2_gpu import setup
from test_host_classify_gpu import read_out
from test_host_cli import CLI
from test_respace_cli import murmur3_long

pytestmark = pytest.mark.gpu


def cli(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240,
                          env=None if env is None else dict(os.environ, **env))


def records_of(orc, S, p, keep=None, taxa=None):
    """orc.build_records of the sequences keep(i) says are labelled, sorted by key"""
    sel = [i for i in range(len(S["seqs"])) if keep is None or keep(i)]
    b = np.frombuffer("".join(S["seqs"][i] for i in sel).encode(), np.uint8)
    o = np.zeros(len(sel) + 1, np.uint64)
    np.cumsum([len(S["seqs"][i]) for i in sel], out=o[1:])
    k, t = orc.build_records(p, S["parents"], b, o, [(taxa or S["seq_taxa"])[i] for i in sel])
    order = np.argsort(k, kind="stable")
    return k[order], t[order]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("build")
    S = setup(tmp, orc)
    S["tmp"], S["orc"] = tmp, orc
    S["taxdir"] = S["loc"] + "_taxonomy"
    S["want"] = records_of(orc, S, S["p"])
    assert same(S["want"], records_of(orc, S, S["p"])) and same(S["want"], tuple(a[np.argsort(S["base"][0], kind="stable")] for a in S["base"]))
    S["out"] = str(tmp / "built" / "lib")
    S["run"] = cli("--partitions", 5, "build", "-i", S["out"], "-t", S["taxdir"], "-l", S["lib"])
    return S


def test_records_files_properties_taxonomy(world):
    r, out = world["run"], world["out"]
    assert r.returncode == 0, r.stderr
    assert same(on_disk(out), world["want"]) and len(world["want"][0]) > 10_000
    files = sorted(glob.glob(os.path.join(out, "*.parquet")))
    assert [os.path.basename(f)[-26:] for f in files] == [f"_{b:05d}.c000.snappy.parquet" for b in range(5)] == [f[-26:] for f in sorted(os.listdir(out))]
    import pyarrow.parquet as pq
    seen = 0
    for b, f in enumerate(files):
        keys = pq.read_table(f).column("id1").to_numpy().tolist()
        assert keys and all(murmur3_long(k) % 5 == b for k in keys)      # every key in its Spark bucket
        seen += len(keys)
    assert seen == len(world["want"][0])
    props = open(out + ".properties").read()
    mask = bm.splitter_line().split("XORmask=")[1].split(" ")[0]
    assert "buckets=5\n" in props and f"XORmask={mask}\n" in props and "k=35\n" in props and "minimizerSpaces=7\n" in props
    assert cli("props", out).stdout == cli("props", world["loc"]).stdout != ""
    names = sorted(os.listdir(world["taxdir"]))
    assert names == sorted(os.listdir(out + "_taxonomy")) == ["names.dmp", "nodes.dmp"]
    assert all(filecmp.cmp(os.path.join(world["taxdir"], n), os.path.join(out + "_taxonomy", n), shallow=False) for n in names)
    assert not os.path.exists(out + ".writing") and not os.path.exists(out + ".slkrec")


def test_what_build_prints_and_stats_on_the_result(world):
    r, out, tax = world["run"], world["out"], world["tax"]
    label_file = world["lib"] + "/seqid2taxid.map"
    two_lines = sm.stats(tax, counts_of(world["want"][1]), 31, False)
    assert r.stdout == bm.splitter_line() + two_lines + bm.input_stats(label_file, bm.read_labels(label_file), tax)
    assert "non-leaf genomes" in r.stdout and "unknown genomes" not in r.stdout      # (two genus-level labels)
    s = cli("stats", "-i", out)
    assert s.returncode == 0 and s.stdout.endswith(two_lines) and two_lines.count("\n") == 2


def test_classify_with_the_built_library(world):
    res = {}
    for name, loc in (("built", world["out"]), ("converted", world["loc"])):
        res[name] = str(world["tmp"] / f"classified_{name}" / "r")
        r = cli("classify", "-i", loc, "-o", res[name], world["fq"])
        assert r.returncode == 0, r.stderr
    lines = read_out(res["built"] + "_c0.0")
    assert lines == read_out(res["converted"] + "_c0.0") and sum(1 for l in lines if l.startswith("C")) >= 500
    assert open(res["built"] + "_c0.0/all_kreport.txt", "rb").read() == open(res["converted"] + "_c0.0/all_kreport.txt", "rb").read()


def test_slkrec_format(world):
    out = str(world["tmp"] / "flat" / "lib")
    r = cli("--partitions", 5, "build", "-i", out, "-t", world["taxdir"], "-l", world["lib"], "--format", "slkrec")
    assert r.returncode == 0, r.stderr
    assert not os.path.isdir(out) and same(on_disk(out), world["want"]) and "buckets=5\n" in open(out + ".properties").read()
    assert r.stdout == world["run"].stdout


@pytest.mark.parametrize("k,m,spaces", [(31, 21, 0), (33, 25, 5)])
def test_other_parameters(world, k, m, spaces):
    orc = world["orc"]
    out = str(world["tmp"] / f"p_{k}_{m}_{spaces}" / "lib")
    r = cli("build", "-i", out, "-t", world["taxdir"], "-l", world["lib"], "-k", k, "-m", m, "--spaces", spaces, "--format", "slkrec")
    assert r.returncode == 0, r.stderr
    want = records_of(orc, world, orc.params(k=k, m=m, spaces=spaces))
    assert same(on_disk(out), want) and not same(want, world["want"])
    assert r.stdout.startswith(bm.splitter_line(k, m, spaces) + sm.stats(world["tax"], counts_of(want[1]), m, False))
    assert "buckets=200\n" in open(out + ".properties").read() and f"minimizerSpaces={spaces}\n" in open(out + ".properties").read()


@pytest.mark.parametrize("seam", ["batches", "pieces", "growth"])
def test_seams_give_the_same_records(world, seam):
    out = str(world["tmp"] / f"seam_{seam}" / "lib")
    env, extra = {"batches": ({"SLK_BUILD_BATCH_BASES": "10000"}, []), "pieces": ({"SLK_EXPORT_PIECE_BUCKETS": "300"}, []),
                  "growth": ({}, ["--expected-records", 1024])}[seam]
    r = cli("--partitions", 5, "build", "-i", out, "-t", world["taxdir"], "-l", world["lib"], *extra, env=env)
    assert r.returncode == 0, r.stderr
    assert same(on_disk(out), world["want"]) and r.stdout == world["run"].stdout
    if seam == "batches":     # 24 sequences of 12 000, 20 and 17 980 bases: the long ones are batches of their own
        assert int(r.stderr.split(" bases in ")[1].split(" batches")[0]) >= 16
    if seam == "pieces":
        assert int(r.stderr.split(" s in ")[1].split(" pieces")[0]) >= 10
        files = sorted(glob.glob(os.path.join(out, "*.parquet")))
        import pyarrow.parquet as pq
        assert len(files) == 5 and all(murmur3_long(k) % 5 == b for b, f in enumerate(files) for k in pq.read_table(f).column("id1").to_numpy().tolist()[::7])
    if seam == "growth":
        assert int(r.stderr.split("(table grown ")[1].split(" times")[0]) >= 1


def test_labels(world, tmp_path):
    """a label whose taxon is undefined, one whose taxon is outside the taxonomy, a sequence without a label"""
    orc, parents = world["orc"], world["parents"]
    lib = tmp_path / "k2lib"
    os.makedirs(lib)
    os.symlink(os.path.join(world["lib"], "library"), lib / "library")
    # the taxonomy without one of its species (a leaf no sequence belongs to, not the largest id): that id is undefined
    undefined = next(t for t in range(len(parents) - 2, 2, -1) if t not in world["seq_taxa"])
    taxdir = str(tmp_path / "tax")
    os.makedirs(taxdir)
    rows = lambda name: [[c.strip() for c in l.split("|")] for l in open(os.path.join(world["taxdir"], name)).read().split("\n") if l]   # noqa: E731
    nodes = [(int(r[0]), int(r[1]), r[2]) for r in rows("nodes.dmp") if int(r[0]) != undefined]
    names = [(int(r[0]), r[1]) for r in rows("names.dmp")]
    with open(os.path.join(taxdir, "nodes.dmp"), "w") as f:
        f.write("".join(f"{t}\t|\t{q}\t|\t{rank}\t|\n" for t, q, rank in nodes))
    os.symlink(os.path.join(world["taxdir"], "names.dmp"), os.path.join(taxdir, "names.dmp"))
    tax = hostmodel.Taxonomy(nodes, names)
    assert not bm.is_defined(tax, undefined) and bm.is_defined(tax, undefined + 1)
    outside = len(parents) + 1000
    taxa = list(world["seq_taxa"])
    taxa[3], taxa[8] = undefined, outside          # (sequences 3k + 1 are 20 bases long: they have no record to lose)
    unlabelled = 9
    with open(lib / "seqid2taxid.map", "w") as f:
        for i, (sid, t) in enumerate(zip(world["seq_ids"], taxa)):
            if i != unlabelled:
                f.write(f"{sid}\t{t}\n")
        f.write("NC_missing.1\t5\n")
    out = str(tmp_path / "out" / "lib")
    r = cli("--partitions", 5, "build", "-i", out, "-t", taxdir, "-l", lib, "--format", "slkrec")
    assert r.returncode == 0, r.stderr
    want = records_of(orc, world, world["p"], keep=lambda i: i not in (3, 8, unlabelled))
    assert same(on_disk(out), want) and len(want[0]) < len(world["want"][0])
    label_file = str(lib) + "/seqid2taxid.map"
    text = bm.input_stats(label_file, bm.read_labels(label_file), tax)
    assert f"2 unknown genomes in {label_file} were not indexed (missing from the taxonomy):\nList({undefined}, {outside})\n" in text
    assert r.stdout == bm.splitter_line() + sm.stats(tax, counts_of(want[1]), 31, False) + text


def test_a_failed_build_leaves_nothing_that_loads(world, tmp_path):
    lib = tmp_path / "k2lib"
    os.makedirs(lib)
    (lib / "seqid2taxid.map").write_text(open(world["lib"] + "/seqid2taxid.map").read())
    out = str(tmp_path / "out" / "lib")
    r = cli("build", "-i", out, "-t", world["taxdir"], "-l", lib)
    assert r.returncode != 0 and "no such directory" in r.stderr
    assert not os.path.exists(out + ".properties") and cli("props", out).returncode != 0
