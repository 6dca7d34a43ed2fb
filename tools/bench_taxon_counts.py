#!/usr/bin/env python3
"""Time of slk_index_taxon_counts (taxstats.hip: one streaming pass over the table with a three-level count) on a resident table,
in three taxon distributions:
  one        every record on one taxon
  skewed     95 % of the records on 16 taxa, the rest over 4 096
  uniform    uniform over 300 000 taxa (far more than the blocks' LDS maps hold: most lanes add to the device counters directly)
against a plain coalesced read-and-sum of as many bytes as the table has (tools/stream_sum.hip: the same loads without the count),
and against today's only alternative, slk_index_export of every record followed by numpy.unique on the host.  Also the part of a call
that does not depend on the table's size (a call on a 512 KiB table: launches, the compaction kernel, the pairs' way to the host),
next to what a download of the whole counter array and a host loop over it would cost instead.
Best of --reps after a warm-up call.  One JSON line on stdout.  Not part of bench.py; no test gates on these numbers.

  python tools/bench_taxon_counts.py --records 2e8 > profiles/r07_taxon_counts.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--records", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=float, default=5e7, help="records appended per call")
    ap.add_argument("--no-export", action="store_true", help="skip the export + numpy.unique comparison")
    a = ap.parse_args()
    import torch
    import slacken_amd
    n, chunk = int(a.records), int(a.chunk)
    S = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    S.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    max_taxon = (1 << 19) - 1          # 19 taxon bits: a counter array of 4 MiB
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"records": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "compute_units": cus}

    def taxa_of(name, m, g):
        if name == "one":
            return torch.full((m,), 7, dtype=torch.int32, device="cuda")
        if name == "uniform":
            return torch.randint(1, 300_001, (m,), dtype=torch.int32, device="cuda", generator=g)
        rest = torch.randint(1, 4097, (m,), dtype=torch.int32, device="cuda", generator=g)
        hot = torch.randint(5000, 5016, (m,), dtype=torch.int32, device="cuda", generator=g)
        return torch.where(torch.rand(m, device="cuda", generator=g) < 0.95, hot, rest).contiguous()

    for name in ("one", "skewed", "uniform"):
        g = torch.Generator(device="cuda").manual_seed(1)
        ix = slacken_amd.Index(expected_records=n, max_taxon=max_taxon, device=0)
        for o in range(0, n, chunk):
            m = min(chunk, n - o)
            k = torch.randint(-2**63, 2**63 - 1, (m,), dtype=torch.int64, device="cuda", generator=g) & ~3
            t = taxa_of(name, m, g)
            ix.append_device(k.data_ptr(), t.data_ptr(), m)
            del k, t
        ix.finalize()
        info = ix.info()
        taxa, counts = ix.taxon_counts()
        assert int(counts.sum()) == info.records
        t_count = best(ix.taxon_counts, a.reps)
        # the yardstick: as many bytes, read and summed
        buf = torch.empty(info.table_bytes // 8, dtype=torch.int64, device="cuda")
        ms = C.c_float(0)
        rc = S.slk_stream_sum(buf.data_ptr(), info.table_bytes, cus * 4, a.reps, C.byref(ms), None)
        assert rc == 0, rc
        del buf
        r = {"table_bytes": int(info.table_bytes), "stored_records": int(info.records), "distinct_taxa": int(len(taxa)),
             "taxon_counts_ms": round(t_count * 1e3, 3), "read_and_sum_ms": round(ms.value, 3),
             "taxon_counts_over_read_and_sum": round(t_count * 1e3 / ms.value, 2),
             "taxon_counts_GB_per_s": round(info.table_bytes / t_count / 1e9, 1),
             "read_and_sum_GB_per_s": round(info.table_bytes / (ms.value * 1e-3) / 1e9, 1)}
        if name == "skewed" and not a.no_export:
            def alt():
                _, tx = ix.export()
                return np.unique(tx, return_counts=True)
            t0 = time.perf_counter()
            at, ac = alt()
            r["export_and_unique_ms"] = round((time.perf_counter() - t0) * 1e3, 1)     # (one run: it takes seconds)
            assert np.array_equal(at, taxa) and np.array_equal(ac.astype(np.uint64), counts)
            r["export_and_unique_over_taxon_counts"] = round(r["export_and_unique_ms"] / r["taxon_counts_ms"], 1)
        res[name] = r
        ix.close()
        torch.cuda.empty_cache()

    # What a call costs beside the pass: a table of 512 KiB (9 taxon bits; the cell layout ties the smallest table to the taxon bits,
    # so the counters here are small too) -- launches, the compaction kernel, the pairs' way to the host.  Next to it what the other
    # way to the pairs would cost, modelled with torch and numpy: the whole counter array to the host and a loop over it there, for
    # the 2^19 counters of the tables above and for the largest array, 2^22.
    ix = slacken_amd.Index(expected_records=8, max_taxon=511, device=0)
    ids = np.arange(1, 401, dtype=np.int32)
    ix.append(np.arange(1, 401, dtype=np.int64) * 4, ids)
    ix.finalize()
    t_small = best(ix.taxon_counts, a.reps)
    beside = {"small_table_bytes": int(ix.info().table_bytes), "small_table_call_ms": round(t_small * 1e3, 3)}
    for bits in (19, 22):
        whole = torch.zeros(1 << bits, dtype=torch.int64, device="cuda")
        whole[torch.arange(1, 4001, device="cuda") * 100] = 1

        def host_loop():
            h = whole.cpu().numpy()
            nz = np.nonzero(h)[0]
            return nz, h[nz]
        beside[f"download_and_host_loop_2^{bits}_counters_ms"] = round(best(host_loop, a.reps) * 1e3, 3)
    res["beside_the_pass"] = beside
    print(json.dumps(res))


if __name__ == "__main__":
    main()
