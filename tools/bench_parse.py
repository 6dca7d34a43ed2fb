#!/usr/bin/env python3
"""The device parser measured (profiles/r12_device_parse.json): slk_parse_device in GB/s of text on R synthetic 150-base reads as
FASTQ and as FASTA, beside a plain read of the same bytes (tools/stream_sum.hip: the floor) and beside `slacken-amd parse --count` on
the host; then `slacken-amd classify`, reports only and detailed, on the plain file and on its .gz, with and without --device-parse --
and, where SLK_PARENT_CLI names the parent commit's binary, that binary on the same files in the same run order.  Run on the GPU box;
prints one JSON object.  R (environment, default 10 000 000), SLK_BENCH_PARSE_CASES (default parse,classify), SLK_BENCH_REPS (runs per
classify case, the best counts; default 2)."""
import ctypes as C
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


def records(bases, starts, first, fastq):
    """reads first .. first + len(starts) as fixed-width records, built column by column: '@r%09d' / '>r%09d', 150 bases"""
    n = len(starts)
    w = 11 + 1 + 150 + 1 + ((1 + 1 + 150 + 1) if fastq else 0)
    a = np.empty((n, w), np.uint8)
    a[:, 0] = ord("@" if fastq else ">")
    a[:, 1] = ord("r")
    ids = np.arange(first, first + n, dtype=np.int64)
    for d in range(9):
        a[:, 10 - d] = ord("0") + (ids // 10 ** d) % 10
    a[:, 11] = 10
    a[:, 12:162] = bases[starts[:, None] + np.arange(150)[None, :]]
    a[:, 162] = 10
    if fastq:
        a[:, 163] = ord("+")
        a[:, 164] = 10
        a[:, 165:315] = ord("I")
        a[:, 315] = 10
    return a.reshape(-1)


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def bench_parse_device(out, texts):
    import torch
    import slacken_amd
    from slacken_amd import capi
    L = capi.lib()
    ix = slacken_amd.Index(expected_records=1024)
    st = ix.stream()
    dev = torch.device("cuda:0")
    ss = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    ss.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    for fmt, path in texts.items():
        text = np.fromfile(path, np.uint8)
        n = text.size
        R = out["reads"]
        d_text = torch.from_numpy(text).to(dev)
        bases = torch.empty(150 * R + 16, dtype=torch.uint8, device=dev)
        offsets = torch.empty(R + 1, dtype=torch.int64, device=dev)
        tpos = torch.empty(R, dtype=torch.int64, device=dev)
        tlen = torch.empty(R, dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def run():
            rc = L.slk_parse_device(st.h, d_text.data_ptr(), n, capi._format(fmt), 1, bases.data_ptr(), 150 * R, offsets.data_ptr(), tpos.data_ptr(),
                                    tlen.data_ptr(), R, counts.data_ptr())
            assert rc == 0, L.slk_last_error()
            st.synchronize()
        run()   # (sizes the stream's scratch)
        dt = timed(run)
        c = counts.cpu().tolist()
        assert c == [R, 150 * R, n, 0], c
        ms, total = C.c_float(0), C.c_ulonglong(0)
        rc = ss.slk_stream_sum(d_text.data_ptr(), n, 256 * 8, 3, C.byref(ms), C.byref(total))
        assert rc == 0, rc
        out["parse_device_" + fmt] = dict(text_bytes=int(n), seconds=round(dt, 5), GB_per_s=round(n / dt / 1e9, 1),
                                          M_reads_per_s=round(R / dt / 1e6, 1), plain_read_ms=round(ms.value, 4),
                                          plain_read_GB_per_s=round(n / (ms.value / 1e3) / 1e9, 1) if ms.value else None)
        t0 = time.perf_counter()
        r = subprocess.run([CLI, "parse", "--count", path], capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr
        out["host_parse_count_" + fmt] = dict(seconds=round(dt, 3), GB_per_s=round(n / dt / 1e9, 2), line=r.stdout.strip())
        del d_text, bases, offsets, tpos, tlen
        torch.cuda.empty_cache()
    st.close()
    ix.close()


def bench_classify(out, loc, d, fq, gz):
    parent = os.environ.get("SLK_PARENT_CLI")
    binaries = ([("parent", parent, [])] if parent else []) + [("host_parse", CLI, []), ("device_parse", CLI, ["--device-parse"])]
    out["parent_binary"] = bool(parent)
    for mode, extra in (("reports_only", ["--nodetailed"]), ("detailed", [])):
        for fname, path in (("plain", fq), ("gz", gz)):
            reports = {}
            for name, exe, flag in binaries:   # (the same order every time: parent, host parser, device parser)
                best = None
                for _ in range(int(os.environ.get("SLK_BENCH_REPS", 2))):
                    o = os.path.join(d, f"out_{mode}_{fname}_{name}")
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, "classify", "-i", loc, "-o", o, *extra, *flag, path], capture_output=True, text=True)
                    dt = time.perf_counter() - t0
                    assert r.returncode == 0, r.stderr
                    best = dt if best is None else min(best, dt)
                reports[name] = open(o + "_c0.0/all_kreport.txt").read()
                out[f"classify_{mode}_{fname}_{name}"] = dict(seconds=round(best, 2), M_reads_per_s=round(out["reads"] / best / 1e6, 2))
            assert len(set(reports.values())) == 1, "the reports differ between the binaries"
    if parent:
        out["device_parse_beats_parent_on_plain_file"] = {
            mode: out[f"classify_{mode}_plain_device_parse"]["seconds"] < out[f"classify_{mode}_plain_parent"]["seconds"]
            for mode in ("reports_only", "detailed")}


def main():
    import torch  # noqa: F401  (before the engine's library: whichever HIP runtime is loaded first opens the GPU)
    import slacken_amd
    import taxgen
    import parquet_to_slkrec as conv
    from test_host_classify2_gpu import write_ranked_taxonomy
    R = int(os.environ.get("R", 10_000_000))
    cases = os.environ.get("SLK_BENCH_PARSE_CASES", "parse,classify").split(",")
    rng = np.random.default_rng(3)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    G, Lg = 64, 1 << 20
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * Lg, dtype=np.uint8)]
    d = tempfile.mkdtemp(prefix="slkparse_")
    out = dict(reads=R, read_length=150)
    starts = rng.integers(0, G * Lg - 150, R)
    fq, fa = os.path.join(d, "reads.fq"), os.path.join(d, "reads.fa")
    for path, fastq in ((fq, True), (fa, False)):
        with open(path, "wb") as f:
            for s in range(0, R, 1 << 20):
                records(bases, starts[s:s + (1 << 20)], s, fastq).tofile(f)
    if "parse" in cases:
        bench_parse_device(out, {"fastq": fq, "fasta": fa})
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
        gz = fq + ".gz"
        with open(gz, "wb") as f:
            subprocess.check_call(["gzip", "-1", "-c", fq], stdout=f)
        bench_classify(out, loc, d, fq, gz)
    shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
