"""`slacken-amd mask` and `build --mask` end to end on one small library (three files, about 100 kb, planted repeats): the device
and the host route write the same bytes, `build --mask` of the unmasked genomes stores the records that `build` stores from the
masked files, and `build` without the flag stores what the oracle's build_records gives for the unmasked ones."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mask_model as mm
import taxgen
from test_gpu_respace_cli import on_disk
from test_host_classify2_gpu import write_ranked_taxonomy
from test_host_cli import CLI
from test_mask_host_cpu import expected_text

pytestmark = pytest.mark.gpu


def cli(*args, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=240,
                          env=None if env is None else dict(os.environ, **env))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def fna_files(lib):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(lib) for f in fs if f.endswith(".fna"))


def records_of(orc, S, seqs):
    b = np.frombuffer("".join(seqs).encode(), np.uint8)
    o = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=o[1:])
    k, t = orc.build_records(S["p"], S["parents"], b, o, S["seq_taxa"])
    order = np.argsort(k, kind="stable")
    return k[order], t[order]


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mask")
    rng = np.random.default_rng(15)
    parents = taxgen.taxonomy(8 * 12, rng)
    ls = (len(parents) - 2) // taxgen.N_RANKS
    species = list(range(7 * ls + 2, 8 * ls + 2))
    # six genomes of about 17 kb with microsatellites and homopolymers of 20..300 letters, an N stretch, a lower-case stretch
    seqs, seq_taxa, seq_ids = [], [], []
    for g in range(6):
        s = mm.planted(rng, int(rng.integers(15000, 19000)), 14, 4, 20, 300)
        s = s[:4000] + "N" * 25 + s[4025:9000] + s[9000:9400].lower() + s[9400:]
        seqs.append(s)
        seq_taxa.append(species[g])
        seq_ids.append(f"NC_{g:03d}.1")
    lib = tmp / "unmasked"
    for sub, idx, width in (("bacteria", (0, 1), 80), ("archaea/deep", (2, 3, 4), 60), ("viral", (5,), 70)):
        os.makedirs(lib / "library" / sub)
        with open(lib / "library" / sub / "library.fna", "w") as f:
            for i in idx:
                f.write(f">{seq_ids[i]} some organism\n" + "".join(seqs[i][j:j + width] + "\n" for j in range(0, len(seqs[i]), width)))
    with open(lib / "seqid2taxid.map", "w") as f:
        for sid, t in zip(seq_ids, seq_taxa):
            f.write(f"{sid}\t{t}\n")
    taxdir = str(tmp / "taxonomy")
    write_ranked_taxonomy(taxdir, parents)
    S = dict(tmp=tmp, p=orc.params(), parents=parents, seqs=seqs, seq_taxa=seq_taxa, lib=str(lib), taxdir=taxdir)
    for name in ("device", "host"):
        shutil.copytree(lib, tmp / name)
        S[name] = str(tmp / name)
    S["run_device"] = cli("mask", "-l", S["device"])
    S["run_host"] = cli("mask", "-l", S["host"], "--host")
    return S


def test_device_and_host_write_the_same_files(world):
    for r in (world["run_device"], world["run_host"]):
        assert r.returncode == 0, r.stderr
    files = fna_files(world["lib"])
    assert len(files) == 3 and 90_000 < sum(os.path.getsize(f) for f in files) < 130_000
    masked = 0
    for f in files:
        rel = os.path.relpath(f, world["lib"])
        before = open(f, "rb").read()
        dev, host = (open(os.path.join(world[k], rel), "rb").read() for k in ("device", "host"))
        want, n, _ = expected_text(before)
        assert dev == host == want and n > 500 and dev != before
        masked += n
        for k in ("device", "host"):
            assert os.path.exists(os.path.join(world[k], rel) + ".masked") and not os.path.exists(os.path.join(world[k], rel) + ".tmp")
    line = world["run_device"].stdout
    assert f" {masked} letters masked" in line and "3 files," in line and "0 files skipped" in line
    assert line.split(" files skipped")[0] == world["run_host"].stdout.split(" files skipped")[0]
    again = cli("mask", "-l", world["device"])
    assert again.returncode == 0 and "3 files skipped" in again.stdout and " 0 letters masked" in again.stdout


def test_small_pieces_and_soft_masking_on_the_device(world):
    lib = str(world["tmp"] / "soft")
    shutil.copytree(world["lib"], lib)
    r = cli("mask", "-l", lib, "--soft", "--window", 32, "--threshold", 15, env={"SLK_MASK_BATCH_BASES": "5000"})
    assert r.returncode == 0, r.stderr
    for f in fna_files(world["lib"]):
        want, n, _ = expected_text(open(f, "rb").read(), window=32, threshold=15, replacement=0)
        assert open(os.path.join(lib, os.path.relpath(f, world["lib"])), "rb").read() == want and n > 0


def test_build_mask_stores_what_build_stores_from_the_masked_files(world, orc):
    outs = {}
    for name, lib, extra in (("plain", world["lib"], []), ("flag", world["lib"], ["--mask"]), ("files", world["device"], []),
                             ("flag-batches", world["lib"], ["--mask"])):
        outs[name] = str(world["tmp"] / f"built_{name}" / "lib")
        env = {"SLK_BUILD_BATCH_BASES": "20000"} if name == "flag-batches" else None
        r = cli("build", "-i", outs[name], "-t", world["taxdir"], "-l", lib, "--format", "slkrec", *extra, env=env)
        assert r.returncode == 0, r.stderr
        assert ("low-complexity letters masked" in r.stderr) == bool(extra)
    rec = {k: on_disk(v) for k, v in outs.items()}
    assert same(rec["flag"], rec["files"]) and same(rec["flag-batches"], rec["files"])
    assert not same(rec["flag"], rec["plain"]) and len(rec["flag"][0]) < len(rec["plain"][0])
    # without the flag: what the build gave before there was one -- the oracle's records of the unmasked genomes
    assert same(rec["plain"], records_of(orc, world, world["seqs"]))
    # and the masked genomes through the oracle: a masked letter ends a run
    b = np.frombuffer("".join(world["seqs"]).encode(), np.uint8)
    o = np.concatenate([[0], np.cumsum([len(s) for s in world["seqs"]])]).astype(np.uint64)
    text = bytes(mm.mask_dp(b, o)[0]).decode()
    assert same(rec["flag"], records_of(orc, world, [text[int(o[i]):int(o[i + 1])] for i in range(len(world["seqs"]))]))
    # the genome files of the unmasked library are as they were
    assert not any(os.path.exists(f + ".masked") for f in fna_files(world["lib"]))
