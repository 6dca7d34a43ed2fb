#!/usr/bin/env python3
"""What the genome coverage costs on one MI355X.  Best of --reps after a warm-up; one JSON line on stdout.

On --genomes synthetic genomes of --length bases (every genome shares a tenth with its neighbour, so the records' LCAs lie at several
depths), against an index built from them:
  coverage_add       slk_coverage_add of all sequences in one call: the copy to the device, the scan, one table lookup and one pair-map
                     atomic per matched super-mer, the map's growth from 2^20 slots
  coverage_fold      slk_coverage_result behind it: the fold of the pair map into (source, depth) rows
  add_sequences      slk_index_add_sequences of the same sequences into an empty table sized for them: the same copy and scan with one
                     random access and one atomic per super-mer -- the natural yardstick
  read_and_sum       tools/stream_sum.hip over as many bytes as the sequences have: the bases read once, already on the device
Not part of bench.py; no test gates on these numbers.

  python tools/bench_coverage.py > profiles/r10_coverage.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--length", type=float, default=2e6)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import slacken_amd
    import taxgen
    rng = np.random.default_rng(10)
    G, L = a.genomes, int(a.length)
    parents = taxgen.taxonomy(8 * max(G, 8), rng)
    ls = (len(parents) - 2) // taxgen.N_RANKS
    taxa = np.array([7 * ls + 2 + g % ls for g in range(G)], np.int32)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * L, dtype=np.uint8)]
    for g in range(1, G):
        bases[g * L:g * L + L // 10] = bases[(g - 1) * L:(g - 1) * L + L // 10]
    offsets = (np.arange(G + 1, dtype=np.uint64) * np.uint64(L))
    depths = np.zeros(len(parents), np.int32)
    for t in range(2, len(parents)):
        depths[t] = (t - 2) // ls + 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"genomes": G, "genome_bases": L, "bases": int(G * L), "reps": a.reps, "runs": 1, "device": torch.cuda.get_device_name(0),
           "compute_units": cus, "k": 35, "m": 31, "spaces": 7}
    expected = int(G * L * 0.45)

    def fresh_index():
        ix = slacken_amd.Index(expected_records=expected, max_taxon=len(parents) - 1, device=0)
        ix.set_taxonomy(parents)
        return ix

    def build_once():
        ix = fresh_index()
        t = time.perf_counter()
        ix.add_sequences(bases, offsets, taxa)
        dt = time.perf_counter() - t
        ix.close()
        return dt

    build_once()
    res["add_sequences_s"] = min(build_once() for _ in range(a.reps))
    ix = fresh_index()
    ix.add_sequences(bases, offsets, taxa)
    ix.finalize()
    info = ix.info()
    res.update(records=int(info.records), table_bytes=int(info.table_bytes), buckets=int(info.buckets))
    st = ix.stream()
    adds, folds = [], []
    for r in range(a.reps + 1):
        cov = slacken_amd.Coverage(ix, depths, stream=st)
        t0 = time.perf_counter()
        cov.add(bases, offsets, taxa)
        t1 = time.perf_counter()
        rows = cov.result()
        t2 = time.perf_counter()
        totals = cov.totals()
        cov.close()
        if r:
            adds.append(t1 - t0)
            folds.append(t2 - t1)
    res.update(coverage_add_s=min(adds), coverage_fold_s=min(folds), rows=int(len(rows[0])), pairs=int(rows[3].sum()),
               matched_supermers=int(rows[2].sum()), supermers=int(totals[2].sum()), kmers=int(totals[1].sum()))
    S = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    S.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    buf = torch.from_numpy(bases.copy()).cuda()
    ms = C.c_float(0)
    rc = S.slk_stream_sum(buf.data_ptr(), buf.numel(), cus * 4, a.reps, C.byref(ms), None)
    assert rc == 0, rc
    res["read_and_sum_s"] = ms.value / 1e3
    res["coverage_over_add_sequences"] = round((res["coverage_add_s"] + res["coverage_fold_s"]) / res["add_sequences_s"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
