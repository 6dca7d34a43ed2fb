"""`slacken-amd coverage` end to end on the library test_host_classify2_gpu.setup writes (three sequences per genome, Ns, line
breaks, two directories, two genus-level labels): the three files and the printed line against coverage_model.py, the same files
from several groups of sources and small batches, and the stop when one source alone exceeds the budget."""
import os
import subprocess

import pytest

import coverage_model as cm
import migration_model as mm
from test_gpu_respace_cli import counts_of
from test_host_classify2_gpu import setup
from test_host_cli import CLI

pytestmark = pytest.mark.gpu
SUFFIXES = ("_support_report_minimizerCoverage.txt", "_support_report_minimizerDistinctCoverage.txt", "_min_report.txt")


def cli(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240,
                          env=None if env is None else dict(os.environ, **env))


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    for seed in (9, 10, 11, 12):      # a library none of whose averages lies at a .5 tie: rounding cannot decide a comparison
        tmp = tmp_path_factory.mktemp("coverage")
        S = setup(tmp, orc, seed=seed)
        index = orc.Index(1, *S["base"])
        rows, totals, misses = cm.coverage(orc, S["p"], index, lambda t: mm.depth(S["tax"], t), [s.encode() for s in S["seqs"]], S["seq_taxa"])
        S["records"] = counts_of(S["base"][1])
        S["sizes"] = [(s, k) for s, k, _ in totals]
        if cm.tie_distance(S["tax"], S["records"], S["sizes"]) > 1e-6:
            break
    assert cm.tie_distance(S["tax"], S["records"], S["sizes"]) > 1e-6
    S["tmp"], S["rows"], S["totals"] = tmp, rows, totals
    S["files"] = [*cm.coverage_lines(rows), cm.min_report(S["tax"], S["records"], S["sizes"])]
    S["need"] = {}
    for q, t in zip(S["seqs"], S["seq_taxa"]):
        S["need"][t] = S["need"].get(t, 0) + max(0, len(q) - 35 + 1)
    return S


def line_of(S, groups):
    return (f"coverage: {len(S['seqs'])} sequences, {len(S['totals'])} source taxa, {sum(k for _, k, _ in S['totals'])} k-mers, "
            f"{sum(n for _, _, n in S['totals'])} super-mers, {sum(a for _, _, a, _ in S['rows'])} matched super-mers, {groups} groups, ")


def test_files_and_line(world):
    S = world
    out = str(S["tmp"] / "one" / "cov")
    r = cli("coverage", "-i", S["loc"], "--library", S["lib"], "-o", out)
    assert r.returncode == 0, r.stderr
    assert [open(out + s).read() for s in SUFFIXES] == S["files"]
    assert r.stdout.startswith(line_of(S, 1)) and r.stdout.endswith(" s\n") and r.stdout.count("\n") == 1
    # the inputs say something: several depths per source, eight labelled taxa
    assert all(l.count("|") >= 1 for l in S["files"][0].split("\n")[:-1])
    assert len(S["totals"]) == 8 and "TKC3-AllChildren" in S["files"][2]

def test_groups_and_batches_give_the_same_files(world):
    S = world
    budget = 2 * max(S["need"].values()) + 10                             # two or three genomes per group
    groups, used = 1, 0
    for t in sorted(S["need"]):
        if used + S["need"][t] > budget:
            groups, used = groups + 1, 0
        used += S["need"][t]
    assert groups >= 3
    out = str(S["tmp"] / "many" / "cov")
    r = cli("coverage", "-i", S["loc"], "-l", S["lib"], "-o", out, "--devices", 0,
            env={"SLK_COVERAGE_MAX_PAIRS": str(budget), "SLK_BUILD_BATCH_BASES": "10000"})
    assert r.returncode == 0, r.stderr
    assert [open(out + s).read() for s in SUFFIXES] == S["files"]
    assert r.stdout.startswith(line_of(S, groups))


def test_a_source_beyond_the_budget_stops_the_run(world):
    S = world
    worst = max(S["need"].values())
    first = min(t for t in S["need"] if S["need"][t] > worst - 100)
    out = str(S["tmp"] / "none" / "cov")
    r = cli("coverage", "-i", S["loc"], "-l", S["lib"], "-o", out, env={"SLK_COVERAGE_MAX_PAIRS": str(worst - 100)})
    assert r.returncode != 0 and r.stdout == ""
    assert f"taxon {first} alone needs {S['need'][first]} (minimizer, source) pairs" in r.stderr and str(worst - 100) in r.stderr
    assert not any(os.path.exists(out + s) for s in SUFFIXES)
