#!/usr/bin/env python3
"""What the sample support costs on one MI355X.  Best of --reps after a warm-up; one JSON line on stdout.

On --reads synthetic reads of --read-len bases drawn from --genomes genomes of --length bases (every genome shares a tenth with its
neighbour, so the records' LCAs lie at several depths; one base in a hundred is substituted), against an index built from the genomes:
  support          slk_support_add of all reads in one call plus slk_support_result: the copy to the device, the scan, one table lookup
                   per super-mer, the cell bitmap and the three counting levels; a few rows come back
  classify         slk_classify_batch of the same reads without hit lists: the same scan and the same lookups -- the yardstick
  host_route       the route `classify2 -D` took before: slk_classify_batch with hit lists and slk_spans_batch, every list downloaded
                   (host_route_device), then the hits at or below the rank counted per taxon and their keys sorted and made unique on
                   the host (host_route_count; numpy's sort on one thread here, std::sort of (taxon, key) pairs and a std::map in the
                   command line it stands for)
The three give the same counts (checked).  Not part of bench.py; no test gates on these numbers.

  python tools/bench_support.py > profiles/r11_support.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--length", type=float, default=2e6)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import slacken_amd
    import taxgen
    rng = np.random.default_rng(11)
    G, L, R, RL = a.genomes, int(a.length), int(a.reads), a.read_len
    parents = taxgen.taxonomy(8 * max(G, 8), rng)
    ls = (len(parents) - 2) // taxgen.N_RANKS
    taxa = np.array([7 * ls + 2 + g % ls for g in range(G)], np.int32)
    genomes = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * L, dtype=np.uint8)]
    for g in range(1, G):
        genomes[g * L:g * L + L // 10] = genomes[(g - 1) * L:(g - 1) * L + L // 10]
    g_offsets = np.arange(G + 1, dtype=np.uint64) * np.uint64(L)
    depths = np.zeros(len(parents), np.int32)
    for t in range(2, len(parents)):
        depths[t] = (t - 2) // ls + 1
    min_depth = 8
    # the reads: whole windows of a genome, one substitution per hundred bases
    bases = np.empty(R * RL, np.uint8)
    for r0 in range(0, R, 100_000):
        n = min(100_000, R - r0)
        start = rng.integers(0, G, n) * L + rng.integers(0, L - RL, n)
        bases[r0 * RL:(r0 + n) * RL] = genomes[(start[:, None] + np.arange(RL)[None, :]).ravel()]
    subs = rng.random(R * RL) < 0.01
    bases[subs] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(subs.sum()), dtype=np.uint8)]
    offsets = np.arange(R + 1, dtype=np.uint64) * np.uint64(RL)

    ix = slacken_amd.Index(expected_records=int(G * L * 0.45), max_taxon=len(parents) - 1, device=0)
    ix.set_taxonomy(parents)
    ix.add_sequences(genomes, g_offsets, taxa)
    ix.finalize()
    info = ix.info()
    st = ix.stream()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"reads": R, "read_len": RL, "bases": int(R * RL), "genomes": G, "genome_bases": L, "reps": a.reps, "runs": 1,
           "device": torch.cuda.get_device_name(0), "compute_units": cus, "k": 35, "m": 31, "spaces": 7, "min_depth": min_depth,
           "records": int(info.records), "table_bytes": int(info.table_bytes), "bitmap_bytes": int(info.buckets * info.bucket_cells // 8)}

    adds, results = [], []
    for r in range(a.reps + 1):
        sup = slacken_amd.Support(ix, depths, min_depth=min_depth, stream=st)
        t0 = time.perf_counter()
        sup.add(bases, offsets)
        t1 = time.perf_counter()
        rows = sup.result()
        t2 = time.perf_counter()
        totals = sup.totals()
        sup.close()
        if r:
            adds.append(t1 - t0)
            results.append(t2 - t1)
    res.update(support_add_s=min(adds), support_result_s=min(results), rows=int(len(rows[0])), supermers=totals[1], matched=totals[2],
               kept=totals[3], kmers=int(rows[1].sum()), distinct=int(rows[3].sum()))

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    st.classify_batch(bases, offsets, with_hits=False)
    res["classify_s"] = min(timed(lambda: st.classify_batch(bases, offsets, with_hits=False))[0] for _ in range(a.reps))

    def host_route():
        t0 = time.perf_counter()
        got = st.classify_batch(bases, offsets, with_hits=True)
        _, spans = st.spans_batch(bases, offsets)
        t1 = time.perf_counter()
        taxon = got["hits"]["taxon"]
        keep = taxon > 0
        keep[keep] = depths[taxon[keep]] >= min_depth
        taxon, key = taxon[keep], spans["key"][keep]
        total = np.bincount(taxon)
        # (a key has one taxon, so the distinct (taxon, key) pairs are the distinct keys: one sort of 8-byte keys, where the command
        #  line sorted 16-byte pairs)
        _, first = np.unique(key, return_index=True)
        distinct = np.bincount(taxon[first])
        return t1 - t0, time.perf_counter() - t1, total, distinct

    host_route()
    runs = [host_route() for _ in range(a.reps)]
    res.update(host_route_device_s=min(r[0] for r in runs), host_route_count_s=min(r[1] for r in runs))
    total, distinct = runs[0][2], runs[0][3]
    assert all(int(total[t]) == int(m) and int(distinct[t]) == int(d) for t, m, d in zip(rows[0], rows[2], rows[3])), "the routes disagree"
    assert int(total.sum()) == int(rows[2].sum()) and int(distinct.sum()) == int(rows[3].sum()), "the routes disagree"
    res["support_over_classify"] = round((res["support_add_s"] + res["support_result_s"]) / res["classify_s"], 3)
    res["host_route_over_support"] = round((res["host_route_device_s"] + res["host_route_count_s"]) / (res["support_add_s"] + res["support_result_s"]), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
