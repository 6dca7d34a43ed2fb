#!/usr/bin/env python3
"""The paired device route measured (profiles/r13_device_pairs.json).  R pairs of synthetic 150-base reads with 40-byte titles as two
FASTQ files:
  pairing   the two texts resident on the device: slk_pair_device beside the two slk_parse_device calls it follows and beside a plain
            read of as many bytes as the titles have (tools/stream_sum.hip: the floor);
  classify  wall time of `slacken-amd classify -p`, reports only and detailed, on the plain files and on their .gz, in three columns:
            the parent commit's binary (SLK_PARENT_CLI), this binary without the flag -- the same code path, so their difference is the
            noise floor -- and this binary with --device-pairs; and one row with SLK_IO_CHUNK at 64 MiB, which shows what the serial
            calls of a file pair cost.
Run on the GPU machine; prints one JSON object.  R (environment, default 1 000 000), SLK_BENCH_PAIRS_CASES (default pairing,classify),
SLK_BENCH_REPS (runs per classify case after one warm-up run, the best counts; default 3)."""
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")
TITLE = 40
PREFIX = b"M01234:56:000000000-ABCDE:1:"   # + 10 digits + "/1": 40 bytes


def records(bases, starts, first, mate):
    """pairs first .. first + len(starts) as fixed-width FASTQ records: '@' + a 40-byte title, 150 bases, '+', 150 quality bytes"""
    n = len(starts)
    assert len(PREFIX) + 10 + 2 == TITLE
    w = 1 + TITLE + 1 + 150 + 1 + 2 + 150 + 1
    a = np.empty((n, w), np.uint8)
    a[:, 0] = ord("@")
    a[:, 1:1 + len(PREFIX)] = np.frombuffer(PREFIX, np.uint8)
    ids = np.arange(first, first + n, dtype=np.int64)
    p = 1 + len(PREFIX)
    for d in range(10):
        a[:, p + 9 - d] = ord("0") + (ids // 10 ** d) % 10
    a[:, p + 10] = ord("/")
    a[:, p + 11] = ord("2" if mate else "1")
    q = 1 + TITLE
    a[:, q] = 10
    a[:, q + 1:q + 151] = bases[starts[:, None] + np.arange(150)[None, :]]
    a[:, q + 151] = 10
    a[:, q + 152] = ord("+")
    a[:, q + 153] = 10
    a[:, q + 154:q + 304] = ord("I")
    a[:, q + 304] = 10
    return a.reshape(-1)


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def bench_pairing(out, paths):
    import torch
    import slacken_amd
    from slacken_amd import capi
    L = capi.lib()
    ix = slacken_amd.Index(expected_records=1024)
    st = ix.stream()
    dev = torch.device("cuda:0")
    ss = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    ss.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    R = out["pairs"]
    side = []
    for path in paths:
        text = np.fromfile(path, np.uint8)
        side.append(dict(n=int(text.size), text=torch.from_numpy(text).to(dev), bases=torch.empty(150 * R + 16, dtype=torch.uint8, device=dev),
                         offsets=torch.empty(R + 1, dtype=torch.int64, device=dev), tpos=torch.empty(R, dtype=torch.int64, device=dev),
                         tlen=torch.empty(R, dtype=torch.int32, device=dev), counts=torch.zeros(4, dtype=torch.int64, device=dev)))
    pair = torch.zeros(8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def parse():
        for t in side:
            rc = L.slk_parse_device(st.h, t["text"].data_ptr(), t["n"], capi.FORMAT_FASTQ, 1, t["bases"].data_ptr(), 150 * R, t["offsets"].data_ptr(),
                                    t["tpos"].data_ptr(), t["tlen"].data_ptr(), R, t["counts"].data_ptr())
            assert rc == 0, L.slk_last_error()
        st.synchronize()

    def pairing():
        a, b = side
        rc = L.slk_pair_device(st.h, a["text"].data_ptr(), a["n"], a["tpos"].data_ptr(), a["tlen"].data_ptr(), a["offsets"].data_ptr(),
                               a["counts"].data_ptr(), R, b["text"].data_ptr(), b["n"], b["tpos"].data_ptr(), b["tlen"].data_ptr(),
                               b["offsets"].data_ptr(), b["counts"].data_ptr(), R, pair.data_ptr())
        assert rc == 0, L.slk_last_error()
        st.synchronize()
    parse()   # (sizes the stream's scratch)
    t_parse = timed(parse)
    pairing()
    assert pair.cpu().tolist()[:2] == [R, 0]
    t_pair = timed(lambda: (parse(), pairing())) - t_parse   # (the first pairing strips the titles: every run starts from parsed ones)
    t_pair_again = timed(pairing)
    assert pair.cpu().tolist() == [R, 0, side[0]["n"], side[1]["n"], R, R, 150 * R, 150 * R], pair.cpu().tolist()
    ms, total = C.c_float(0), C.c_ulonglong(0)
    title_bytes = 2 * R * TITLE
    rc = ss.slk_stream_sum(side[0]["text"].data_ptr(), title_bytes, 256 * 8, 3, C.byref(ms), C.byref(total))
    assert rc == 0, rc
    out["pairing"] = dict(text_bytes=[t["n"] for t in side], title_bytes=title_bytes, two_parses_ms=round(t_parse * 1e3, 3),
                          pairing_after_parses_ms=round(t_pair * 1e3, 3), pairing_alone_ms=round(t_pair_again * 1e3, 3),
                          plain_read_of_title_bytes_ms=round(ms.value, 4), M_pairs_per_s=round(R / t_pair_again / 1e6, 1))
    st.close()
    ix.close()


def bench_classify(out, loc, d, plain, gz):
    parent = os.environ.get("SLK_PARENT_CLI")
    reps = int(os.environ.get("SLK_BENCH_REPS", 3))
    binaries = ([("parent", parent, [])] if parent else []) + [("host_pairs", CLI, []), ("device_pairs", CLI, ["--device-pairs"])]
    out["parent_binary"] = bool(parent)
    out["classify_reps"] = reps

    def run(tag, exe, args, env=None):
        best = None
        o = os.path.join(d, "out_" + tag)
        for i in range(reps + 1):   # (the first run warms the page cache and the device and does not count)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "classify", "-i", loc, "-o", o, "-p", *args], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr
            if i:
                best = dt if best is None else min(best, dt)
        print(tag, round(best, 3), file=sys.stderr, flush=True)
        out["classify_" + tag] = dict(seconds=round(best, 3), M_pairs_per_s=round(out["pairs"] / best / 1e6, 2))
        report = open(o + "_c0.0/all_kreport.txt").read()
        for loc_out in glob.glob(o + "_c*"):   # (the per-read files of 10 M pairs are a gigabyte per run)
            shutil.rmtree(loc_out, ignore_errors=True)
        return report

    for mode, extra in (("reports_only", ["--nodetailed"]), ("detailed", [])):
        for fname, files in (("plain", plain), ("gz", gz)):
            reports = {name: run(f"{mode}_{fname}_{name}", exe, [*extra, *flag, *files]) for name, exe, flag in binaries}
            assert len(set(reports.values())) == 1, "the reports differ between the binaries"
    for fname, files in (("plain", plain), ("gz", gz)):
        run(f"reports_only_{fname}_device_pairs_chunk64MiB", CLI, ["--nodetailed", "--device-pairs", *files], env={"SLK_IO_CHUNK": str(64 << 20)})


def main():
    import torch  # noqa: F401  (before the engine's library: whichever HIP runtime is loaded first opens the GPU)
    import slacken_amd
    import taxgen
    import parquet_to_slkrec as conv
    from test_host_classify2_gpu import write_ranked_taxonomy
    R = int(os.environ.get("R", 1_000_000))
    cases = os.environ.get("SLK_BENCH_PAIRS_CASES", "pairing,classify").split(",")
    rng = np.random.default_rng(3)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    G, Lg = 64, 1 << 20
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * Lg, dtype=np.uint8)]
    d = tempfile.mkdtemp(prefix="slkpairs_")
    out = dict(pairs=R, read_length=150, title_bytes=TITLE)
    starts = rng.integers(0, G * Lg - 500, R)
    plain = [os.path.join(d, "reads_1.fq"), os.path.join(d, "reads_2.fq")]
    for path, mate in zip(plain, (False, True)):
        with open(path, "wb") as f:
            for s in range(0, R, 1 << 20):
                records(bases, starts[s:s + (1 << 20)] + (300 if mate else 0), s, mate).tofile(f)
    print("files written", file=sys.stderr, flush=True)
    if "pairing" in cases:
        bench_pairing(out, plain)
    if "classify" in cases:
        offsets = np.arange(G + 1, dtype=np.uint64) * np.uint64(Lg)
        ix = slacken_amd.Index(expected_records=G * Lg // 2, max_taxon=len(parents) - 1)
        ix.set_taxonomy(parents)
        ix.add_sequences(bases, offsets, rng.choice(taxa[len(taxa) // 2:], G).astype(np.int32))
        keys, tx = ix.export()
        ix.close()
        loc = os.path.join(d, "lib")
        conv.write_slkrec(loc + ".slkrec", keys, tx)
        with open(loc + ".properties", "w") as f:
            f.write("k=35\nm=31\nversion=1\nsplitter=randomXOR\nminimizerSpaces=7\n")
        write_ranked_taxonomy(loc + "_taxonomy", parents)
        gz = [p + ".gz" for p in plain]
        procs = [subprocess.Popen(["gzip", "-1", "-c", p], stdout=open(g, "wb")) for p, g in zip(plain, gz)]
        assert all(p.wait() == 0 for p in procs)
        print("files compressed", file=sys.stderr, flush=True)
        bench_classify(out, loc, d, plain, gz)
    shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
