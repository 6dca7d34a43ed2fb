"""`slacken-amd bracken-build` and `classify2 --bracken-length` end to end on the library layout of test_host_classify2_gpu,
against the Bracken model (tests/bracken_model.py) driven by the CPU oracle."""
import os
import subprocess

import numpy as np
import pytest

import bracken_model as bm
from test_bracken_cli import kmer_distrib_of
from test_host_classify2_gpu import setup
from test_host_cli import CLI

pytestmark = pytest.mark.gpu


def tree(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_bracken_build_and_classify2(tmp_path, orc):
    S = setup(tmp_path, orc)
    base = orc.Index(1, *S["base"])
    want = kmer_distrib_of(bm.fast(orc, S["p"], base, S["parents"], [s.encode() for s in S["seqs"]], S["seq_taxa"], 100))
    for devices in ("0", "0,0"):
        subprocess.run([CLI, "bracken-build", "-i", S["loc"], "--library", S["lib"], "--devices", devices], check=True,
                       capture_output=True)
        got = open(S["loc"] + "_bracken/database100mers.kmer_distrib").read()
        assert got == want, devices
    # classify2: the file appears beside the other outputs, which stay byte for byte those of a run without the flag
    outs = {}
    for flag in ([], ["--bracken-length", "100"]):
        out = str(tmp_path / ("with" if flag else "without"))
        subprocess.run([CLI, "classify2", "-i", S["loc"], "-o", out, "--library", S["lib"], "-R", "50", *flag, S["fq"]],
                       check=True, capture_output=True)
        outs[bool(flag)] = (tree(out), open(out + "_taxonSet.txt", "rb").read())
    kd = outs[True][0].pop("database100mers.kmer_distrib").decode()
    assert outs[True] == outs[False]
    # the model on the dynamic library: the sequences labelled with a taxon of the detected set or below it (Dynamic.scala:
    # 362-373), against the records built from them
    keep = {int(x) for x in outs[True][1].split()}
    parents = S["parents"]

    def in_set(t):
        while t != 0:
            if t in keep:
                return True
            t = int(parents[t])
        return False
    chosen = [i for i, t in enumerate(S["seq_taxa"]) if in_set(t)]
    assert 0 < len(chosen) < len(S["seqs"])
    seqs = [S["seqs"][i].encode() for i in chosen]
    taxa = [S["seq_taxa"][i] for i in chosen]
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.uint64)
    dk, dt = orc.build_records(S["p"], parents, bases, offsets, np.array(taxa, np.int32))
    assert kd == kmer_distrib_of(bm.fast(orc, S["p"], orc.Index(1, dk, dt), parents, seqs, taxa, 100))
    r = subprocess.run([CLI, "classify2", "-i", S["loc"], "-o", str(tmp_path / "short"), "--library", S["lib"],
                        "--bracken-length", "20", S["fq"]], capture_output=True, text=True)
    assert r.returncode != 0 and "shorter than k" in r.stderr
