"""`slacken-amd support` end to end against support_model.py, byte for byte: the four reports of a FASTQ sample, of the same reads
gzipped and of a paired sample, at the species and at the genus rank, on one device and with two named; and `classify2 -C` / `-D`,
whose counts come from the same pass, with one device and with two."""
import gzip
import os
import subprocess

import pytest

import hostmodel
import support_model as sm
from test_host_cli import CLI
from test_host_classify2_gpu import run2, setup

pytestmark = pytest.mark.gpu
NOTE = "the support pass counts on one device: device 0, the first of the 2 named by --devices"


@pytest.fixture(scope="module")
def S(orc, tmp_path_factory):
    return setup(tmp_path_factory.mktemp("support_cli"), orc, seed=21)


def support(*args):
    r = subprocess.run([CLI, "support", *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def files_of(out):
    return {name: open(f"{out}_support_report_{name}.txt").read() for name in sm.SUFFIXES}


def model_texts(orc, S, reads, rank_depth):
    """reads: sequences or (mate 1, mate 2) pairs, every one under a title of its own"""
    p, parents, tax = S["p"], S["parents"], S["tax"]
    base = orc.Index(1, *S["base"])
    model = sm.support(orc, p, base, lambda t: hostmodel.depth(tax, t), reads)
    classified = {}
    for r in reads:
        s1, s2 = r if isinstance(r, tuple) else (r, None)
        res, hits = orc.classify_read(p, base, parents, s1, s2, 2, 0.0)
        if hits and res["classified"]:
            classified[res["taxon"]] = classified.get(res["taxon"], 0) + 1
    rows = model.rows(rank_depth)
    assert len(rows) > 1 and model.totals(rank_depth)[2] > model.totals(rank_depth)[3] > 0 and classified
    return sm.report_texts(tax, rows, classified.items())


def test_support_reports(S, orc, tmp_path):
    reads = [s for _, s in S["reads"]]
    species = model_texts(orc, S, reads, 8)
    r = support("-i", S["loc"], "-o", tmp_path / "fq", S["fq"])
    assert files_of(tmp_path / "fq") == species and NOTE not in r.stderr
    assert f"support: {len(reads)} sequences" in r.stdout
    # the same reads gzipped
    gz = str(tmp_path / "sample.fq.gz")
    with open(S["fq"], "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    support("-i", S["loc"], "-o", tmp_path / "gz", gz)
    assert files_of(tmp_path / "gz") == species
    # --rank genus lets the hits on genus nodes in
    genus = model_texts(orc, S, reads, 7)
    assert genus["totalMinimizerCount"] != species["totalMinimizerCount"] and genus["classifiedReadCount"] == species["classifiedReadCount"]
    support("-i", S["loc"], "-o", tmp_path / "genus", "--rank", "genus", S["fq"])
    assert files_of(tmp_path / "genus") == genus
    # two devices named: counted on the first, and said so
    r = support("-i", S["loc"], "-o", tmp_path / "two", "--devices", "0,0", S["fq"])
    assert files_of(tmp_path / "two") == species and NOTE in r.stderr


def test_support_of_a_paired_sample(S, orc, tmp_path):
    reads = [s for _, s in S["reads"]]
    pairs = [(reads[2 * i], reads[2 * i + 1]) for i in range(300)]
    for mate in (1, 2):
        with open(tmp_path / f"pairs_{mate}.fq", "w") as f:
            for i, pr in enumerate(pairs):
                f.write(f"@pair{i}/{mate}\n{pr[mate - 1]}\n+\n{'I' * len(pr[mate - 1])}\n")
    support("-i", S["loc"], "-o", tmp_path / "paired", "-p", tmp_path / "pairs_1.fq", tmp_path / "pairs_2.fq")
    assert files_of(tmp_path / "paired") == model_texts(orc, S, pairs, 8)


@pytest.mark.parametrize("flag,threshold", [("-C", 400), ("-D", 300)])
def test_classify2_counts_on_one_device(S, tmp_path, flag, threshold):
    err = {}
    for name, devices in (("one", "0"), ("two", "0,0")):
        os.makedirs(tmp_path / name)
        err[name] = run2("-i", S["loc"], "-o", tmp_path / name / "dyn", "--library", S["lib"], flag, threshold, "--rank", "genus", "--devices", devices,
                         S["fq"])
    sets = [open(tmp_path / name / "dyn_taxonSet.txt").read() for name in ("one", "two")]
    assert sets[0] == sets[1] and sets[0].split()
    assert NOTE in err["two"] and NOTE not in err["one"]
