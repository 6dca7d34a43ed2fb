"""`slacken-amd compare-index` end to end: two libraries on disk in Slacken's layout (Parquet records or the flat .slkrec,
.properties, _taxonomy), the REFERENCE built from all genomes of test_host_classify2_gpu.setup and the SUBJECT from one of them
plus a sequence of its own; stdout and OUTPUT_taxaToRoot_report.txt against migration_model.py, byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import migration_model as mm
import synth
from test_host_cli import CLI, ROOT
from test_host_classify2_gpu import setup, write_ranked_taxonomy

sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

PROPERTIES = "k=35\nm=31\nbuckets=3\nversion=1\nsplitter=randomXOR\nminimizerSpaces={spaces}\ncanonical=true\n"


def write_library(loc, keys, taxa, parents, parquet, spaces=7):
    import parquet_to_slkrec as conv
    if parquet:
        conv.write_parquet_dir(loc, keys, taxa, buckets=3)
    else:
        conv.write_slkrec(loc + ".slkrec", keys, taxa)
    with open(loc + ".properties", "w") as f:
        f.write(PROPERTIES.format(spaces=spaces))
    write_ranked_taxonomy(loc + "_taxonomy", parents)
    return loc


def build_libraries(tmp_path, orc):
    S = setup(tmp_path, orc)
    p, parents = S["p"], S["parents"]
    rk, rt = S["base"]
    # SUBJECT: genome 0 alone of those that share a stretch (its minimizers there are the species' own; in the REFERENCE they are the
    # LCA of all genomes, ROOT), and a sequence of its own under the genus of genome 6: a piece of genome 2 (a species in the
    # REFERENCE: one rank DOWN) followed by bases the REFERENCE lacks
    rng = np.random.default_rng(77)
    sel = [i for i, sid in enumerate(S["seq_ids"]) if int(sid[3:6]) == 0]
    seqs = [S["seqs"][i] for i in sel] + [S["seqs"][6][5000:8000] + synth.random_dna(4000, rng).tobytes().decode()]
    taxa = [S["seq_taxa"][i] for i in sel] + [S["seq_taxa"][18]]
    bases = np.frombuffer("".join(seqs).encode(), np.uint8)
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    sk, stx = orc.build_records(p, parents, bases, offsets, taxa)
    locs = {}
    for form, parquet in (("parquet", True), ("slkrec", False)):
        locs["ref_" + form] = write_library(str(tmp_path / ("ref_" + form)), rk, rt, parents, parquet)
        locs["sub_" + form] = write_library(str(tmp_path / ("sub_" + form)), sk, stx, parents, parquet)
    locs["sub_other_spaces"] = write_library(str(tmp_path / "sub_other"), sk, stx, parents, False, spaces=5)
    pairs, matched, unmatched = mm.join(zip(np.asarray(sk).tolist(), np.asarray(stx).tolist()),
                                        dict(zip(np.asarray(rk).tolist(), np.asarray(rt).tolist())))
    trip = mm.triples(pairs, S["tax"])
    return S, locs, trip, matched, unmatched, len(sk)


def check_model_preconditions(trip, unmatched):
    assert len({s for _, _, s, _ in trip}) >= 3
    assert any(t2 == mm.ROOT and t1 != mm.ROOT for t1, t2, _, _ in trip)
    assert mm.to_root(trip)
    assert unmatched >= 1


def compare(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240)


def test_compare_index(tmp_path, orc):
    S, locs, trip, matched, unmatched, n_subject = build_libraries(tmp_path, orc)
    check_model_preconditions(trip, unmatched)
    table, report = mm.show(trip), mm.report(S["tax"], trip)
    for n, (cmd, form, extra) in enumerate((("compare-index", "parquet", ()), ("compare-index", "slkrec", ("--devices", "0")),
                                            ("compareIndex", "slkrec", ()))):
        out = str(tmp_path / f"out{n}" / "cmp")
        ref_flag = "-r" if n else "--reference"
        r = compare(cmd, "-i", locs["sub_" + form], ref_flag, locs["ref_" + form], "-o", out, *extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == table
        assert open(out + "_taxaToRoot_report.txt").read() == report
        summary = [line for line in r.stderr.split("\n") if line.startswith("compare-index: ")]
        assert len(summary) == 1
        assert (f"{n_subject} records read, {matched} matched, {unmatched} unmatched, {len(trip)} distinct pairs") in summary[0]
    # another splitter: the minimizers of the two libraries cannot be compared
    out = str(tmp_path / "refused" / "cmp")
    r = compare("compare-index", "-i", locs["sub_other_spaces"], "-r", locs["ref_slkrec"], "-o", out)
    assert r.returncode != 0 and "do not share a minimizer scheme" in r.stderr and r.stdout == ""
    assert not os.path.exists(out + "_taxaToRoot_report.txt")
