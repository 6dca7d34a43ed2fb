"""`slacken-amd respace` end to end: a generated library at 7 spaces on disk (Parquet and .slkrec), respaced on the GPU to 10 and 12
spaces, written by the library writer, and what is on disk compared with respace_model.py; then the written library is used --
`stats` and `classify` on it give what stats_model.py, hostmodel.py and the oracle give for the model's records."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import hostmodel
import respace_model as rm
import stats_model as sm
import synth
from test_gpu_migration_cli import write_library       # (puts tools/ on sys.path: parquet_to_slkrec)
from test_gpu_stats_cli import splitter_lines
from test_host_cli import CLI
from test_host_classify_gpu import read_out

pytestmark = pytest.mark.gpu


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240)


def counts_of(taxa):
    t, c = np.unique(taxa, return_counts=True)
    return list(zip(t.tolist(), c.tolist()))


def on_disk(loc):
    import parquet_to_slkrec as conv
    if os.path.isdir(loc):
        keys, taxa = conv.read_parquet_dir(loc)
    else:
        raw = open(loc + ".slkrec", "rb").read()
        n = int(np.frombuffer(raw[8:16], "<u8")[0])
        keys, taxa = np.frombuffer(raw[24:24 + 8 * n], np.int64), np.frombuffer(raw[24 + 8 * n:], np.int32)
    o = np.argsort(keys, kind="stable")
    return keys[o], taxa[o]


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("respace")
    rng = np.random.default_rng(712)
    g = rm.generate(3000, rng)
    # the generated set has no genomes behind it, so no read would hit it: beside it the minimizers of six small genomes at 7 spaces
    # (LCA records where they share stretches), which the reads for `classify` are drawn from
    lib = synth.Library(orc, orc.params(spaces=7), g["parents"], n_genomes=6, genome_len=8000)
    new = ~np.isin(lib.keys, g["keys"])
    g["keys"], g["taxa"] = np.concatenate([g["keys"], lib.keys[new]]), np.concatenate([g["taxa"], lib.taxa[new]])
    g["orc"] = orc
    g["reads"] = [(f"read{i}", r.tobytes().decode()) for i, r in enumerate(synth.make_reads(lib, 300, rng))]
    g["tmp"] = tmp
    g["model"] = {s: rm.respace(g["keys"], g["taxa"], g["parents"], 31, s) for s in (10, 12)}
    for form, parquet in (("parquet", True), ("slkrec", False)):
        os.makedirs(tmp / form)
        g[form] = write_library(str(tmp / form / "lib_35_31_s7"), g["keys"], g["taxa"], g["parents"], parquet)
    return g


@pytest.mark.parametrize("form", ["parquet", "slkrec"])
def test_respace_writes_the_models_libraries(world, form):
    from test_host_classify2_gpu import write_ranked_taxonomy
    src = world[form]
    tax = write_ranked_taxonomy(str(world["tmp"] / f"tax_{form}"), world["parents"])   # (the same files write_library wrote)
    out = world["tmp"] / f"out_{form}" / "out_35_31_s7"
    extra = ("--format", "slkrec") if form == "slkrec" else ()
    r = cli("respace", "-i", src, "-o", out, "--spaces", "10", "12", *extra)
    assert r.returncode == 0, r.stderr
    want_stdout = ""
    for s in (10, 12):
        loc = str(out)[:-3] + f"_s{s}"
        mk, mt = world["model"][s]
        got = on_disk(loc)
        assert np.array_equal(got[0], mk) and np.array_equal(got[1], mt)
        assert os.path.isdir(loc) == (form == "parquet") and os.path.exists(loc + ".slkrec") == (form == "slkrec")
        if form == "parquet":
            assert len(os.listdir(loc)) == 3
        assert cli("props", loc).stdout == cli("props", src).stdout.replace("spaces=7", f"spaces={s}") != ""
        assert "buckets=3\n" in open(loc + ".properties").read()
        names = sorted(os.listdir(src + "_taxonomy"))
        assert names == sorted(os.listdir(loc + "_taxonomy")) == ["names.dmp", "nodes.dmp"]
        assert all(filecmp.cmp(os.path.join(src + "_taxonomy", n), os.path.join(loc + "_taxonomy", n), shallow=False) for n in names)
        want_stdout += f"Stats for {loc}\n" + sm.stats(tax, counts_of(mt), 31, False)
    assert r.stdout == want_stdout
    # the written library is a library: stats ...
    loc = str(out)[:-3] + "_s12"
    mk, mt = world["model"][12]
    r = cli("stats", "-i", loc)
    assert r.returncode == 0, r.stderr
    assert r.stdout == splitter_lines(dict(m=31, spaces=12)) + sm.stats(tax, counts_of(mt), 31, False)
    if form == "slkrec":
        return
    # ... and classify
    orc, parents = world["orc"], world["parents"]
    p12 = orc.params(spaces=12)
    oix = orc.Index(1, mk, mt)
    reads = world["reads"]
    fq = world["tmp"] / "reads.fq"
    with open(fq, "w") as f:
        for t, s in reads:
            f.write(f"@{t}\n{s}\n+\n{'I' * len(s)}\n")
    res = world["tmp"] / "classified" / "r"
    r = cli("classify", "-i", loc, "-o", res, str(fq))
    assert r.returncode == 0, r.stderr
    want, counts = [], {}
    for t, s in reads:
        out_r, hits = orc.classify_read(p12, oix, parents, s, None, 2, 0.0)
        if hits:
            want.append(orc.output_line(out_r["classified"], t, out_r["taxon"], hits, 35))
            counts[out_r["taxon"]] = counts.get(out_r["taxon"], 0) + 1
    assert sum(1 for l in want if l.startswith("C")) >= 100
    assert read_out(f"{res}_c0.0") == want
    rep = open(f"{res}_c0.0/all_kreport.txt").read().rstrip("\n").split("\n")
    assert rep == hostmodel.kraken_report(tax, sorted(counts.items()))[0]


def test_respace_refuses_and_stops(world):
    src = world["slkrec"]
    out = world["tmp"] / "stops" / "o_35_31_s7"
    r = cli("respace", "-i", src, "-o", out, "--spaces", "7", "--format", "slkrec")
    assert r.returncode != 0 and r.stdout == ""
    assert "Respacing to a smaller or identical number of spaces is not meaningful. (was 7, requested 7)" in r.stderr
    assert not os.path.exists(out.parent) or os.listdir(out.parent) == []
    r = cli("respace", "-i", src, "-o", out, "--spaces", "10", "5", "12", "--format", "slkrec")
    assert r.returncode != 0 and "not meaningful. (was 7, requested 5)" in r.stderr
    base = str(out)[:-3]
    got = on_disk(base + "_s10")
    assert np.array_equal(got[0], world["model"][10][0]) and np.array_equal(got[1], world["model"][10][1])
    assert r.stdout.startswith(f"Stats for {base}_s10\n") and r.stdout.count("Stats for") == 1
    assert sorted(os.listdir(out.parent)) == ["o_35_31_s10.properties", "o_35_31_s10.slkrec", "o_35_31_s10_taxonomy"]
