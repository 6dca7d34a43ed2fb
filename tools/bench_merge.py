#!/usr/bin/env python3
"""Time of the merge entries (merge.hip) on one MI355X, synthetic records -- unique random keys at 7 spaces, taxa uniform over a
taxgen.taxonomy(400) -- beside their yardsticks, all measured in the same run:
  append        slk_index_append_device of N records into an empty table: the plain insert (first record of a key kept, duplicates
                counted), the code there was before.  THE yardstick of
  merge_empty   slk_index_merge_records_device of the same N records into an empty table of the same geometry: every record an
                insert, after the taxon check
  merge_full    the same N records merged into a table that already holds their keys with other taxa: every record a merge, with
                the parent walks of tax_lca and a CAS where the LCA differs from what the cell holds
  merge_index   slk_index_merge_index of a resident, finalized table of the N records into an empty one, beside
  respace       slk_index_respace of the same source (7 -> 12 spaces: the same walk plus a mask; of random keys next to none merge) and
  read          a plain coalesced read of the source table's bytes (tools/stream_sum.hip): what the walk cannot beat
  host_route    what there was before for two libraries: slk_index_export of both, numpy.concatenate and numpy.unique on the host,
                slk_index_append -- WITHOUT the LCA of the shared keys (the host has none: each keeps its first taxon), so a lower
                bound for that route -- beside slk_index_merge_index of both into an empty table
Every table is created for N expected records at the default load factor, so the geometry is the same throughout and is reported.
Every figure: the times of --reps runs after a warm-up run (the host route: one run), their minimum and their spread (max / min).
One JSON line on stdout.  Not part of bench.py; no test gates on it.

  python tools/bench_merge.py --records 1e8 > profiles/r19_merge.json"""
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


def timed(fn, reps, prepare=None):
    """fn() timed `reps` times after a warm-up; prepare() (untimed) before each -> [seconds]"""
    out = []
    for r in range(reps + 1):
        state = prepare() if prepare else None
        t = time.perf_counter()
        fn(state)
        dt = time.perf_counter() - t
        if r:
            out.append(dt)
        if state is not None:
            state.close()
    return out


def figures(name, ts, n):
    return {f"{name}_ms": [round(t * 1e3, 2) for t in ts], f"{name}_best_ms": round(min(ts) * 1e3, 2), f"{name}_spread": round(max(ts) / min(ts), 3),
            f"{name}_records_per_s": round(n / min(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    import torch
    import respace_model as rm
    import slacken_amd
    import taxgen
    from slacken_amd import capi
    dev = "cuda"
    n, m, s_old, s_new = int(a.records), 31, 7, 12
    g = torch.Generator(device=dev).manual_seed(19)
    rng = np.random.default_rng(19)
    parents = taxgen.taxonomy(400, rng)
    defined = torch.tensor(np.array(taxgen.defined_taxa(parents), np.int32), device=dev)
    mask7 = rm.mask(m, s_old)
    mask7 = mask7 - (1 << 64) if mask7 >> 63 else mask7
    keys = torch.unique(torch.randint(-2**63, 2**63 - 1, (n + n // 64,), dtype=torch.int64, device=dev, generator=g) & mask7)
    keys = keys[torch.randperm(len(keys), device=dev, generator=g)][:n].contiguous()
    assert len(keys) == n
    taxa = defined[torch.randint(0, len(defined), (n,), device=dev, generator=g)].contiguous()
    taxa2 = defined[torch.randint(0, len(defined), (n,), device=dev, generator=g)].contiguous()
    torch.cuda.synchronize()

    def table(taxonomy=True):
        ix = slacken_amd.Index(spaces=s_old, expected_records=n, max_taxon=len(parents) - 1, device=0)
        if taxonomy:
            ix.set_taxonomy(parents)
        return ix

    def filled():
        ix = table()
        ix.append_device(keys.data_ptr(), taxa2.data_ptr(), n)
        return ix

    probe = table()
    info = probe.info()
    probe.close()
    res = {"records": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "taxonomy_nodes": int(len(defined)),
           "table_bytes": int(info.table_bytes), "table_buckets": int(info.buckets), "bucket_cells": int(info.bucket_cells),
           "table_load": round(n / (info.buckets * info.bucket_cells), 3), "taxon_bits": int(info.taxon_bits), "disp_bits": int(info.disp_bits)}

    def check(ix, grown=0):
        i = ix.info()
        assert i.records == n and i.grown == grown and i.duplicate_keys == 0, (i.records, i.grown, i.duplicate_keys)

    # alternating, so that what else runs on the machine meets both alike
    t_append, t_merge = [], []
    for r in range(a.reps + 1):
        for which, out in (("append", t_append), ("merge", t_merge)):
            ix = table()
            t = time.perf_counter()
            if which == "append":
                ix.append_device(keys.data_ptr(), taxa.data_ptr(), n)
            else:
                ix.merge_records_device(keys.data_ptr(), taxa.data_ptr(), n)
            dt = time.perf_counter() - t
            check(ix)
            ix.close()
            if r:
                out.append(dt)
    res.update(figures("append", t_append, n))
    res.update(figures("merge_empty", t_merge, n))
    res["merge_empty_over_append"] = round(min(t_merge) / min(t_append), 3)

    ts = timed(lambda ix: ix.merge_records_device(keys.data_ptr(), taxa.data_ptr(), n), a.reps, prepare=filled)
    res.update(figures("merge_full", ts, n))
    res["merge_full_over_append"] = round(min(ts) / min(t_append), 3)

    src = table()
    src.append_device(keys.data_ptr(), taxa.data_ptr(), n)
    src.finalize()
    check(src)
    ts_mi = timed(lambda ix: ix.merge_index(src), a.reps, prepare=table)
    res.update(figures("merge_index", ts_mi, n))
    state = {}

    def run_respace(_):
        if state.get("out") is not None:
            state["out"].close()
        state["out"] = src.respace(s_new)
    ts_rs = timed(run_respace, a.reps)
    res["respace_result_records"] = int(state["out"].info().records)
    assert res["respace_result_records"] > 0.999 * n      # (random keys: the wider mask merges next to none)
    state["out"].close()
    res.update(figures("respace", ts_rs, n))
    res["merge_index_over_respace"] = round(min(ts_mi) / min(ts_rs), 3)

    S = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    S.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    buf = torch.zeros(info.table_bytes // 8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cus, ms = torch.cuda.get_device_properties(0).multi_processor_count, C.c_float(0)
    assert S.slk_stream_sum(buf.data_ptr(), info.table_bytes, cus * 4, a.reps, C.byref(ms), None) == 0
    del buf
    res.update(read_table_bytes_best_ms=round(ms.value, 3), merge_index_over_read=round(min(ts_mi) * 1e3 / ms.value, 1))

    if not a.no_host_route:
        # a second library: a quarter as many records, half of them under keys of the first with other taxa
        n2 = n // 4
        extra = torch.unique(torch.randint(-2**63, 2**63 - 1, (n2,), dtype=torch.int64, device=dev, generator=g) & mask7)[:n2 // 2]
        k2 = torch.cat([keys[:n2 - len(extra)], extra]).contiguous()
        other = table()
        other.append_device(k2.data_ptr(), taxa2.data_ptr(), len(k2))
        other.finalize()
        n_other = int(other.info().records)

        def device_route(ix):
            ix.merge_index(src)
            ix.merge_index(other)
            state["n_device"] = int(ix.info().records)
        ts_dev = timed(device_route, a.reps, prepare=table)
        hk, ht, got = np.zeros(n + n_other, np.int64), np.zeros(n + n_other, np.int32), C.c_uint64(0)
        t0 = time.perf_counter()
        capi._check(capi.lib().slk_index_export(src.h, hk.ctypes.data, ht.ctypes.data, n, C.byref(got)))   # (the call itself: Index.export sorts)
        capi._check(capi.lib().slk_index_export(other.h, hk[n:].ctypes.data, ht[n:].ctypes.data, n_other, C.byref(got)))
        t1 = time.perf_counter()
        hu, at = np.unique(hk, return_index=True)
        t2 = time.perf_counter()
        ix = table(taxonomy=False)
        ix.append(hu, ht[at])
        ix.finalize()
        t3 = time.perf_counter()
        assert ix.info().records == state["n_device"] == len(hu)
        ix.close()
        res.update(figures("two_libraries_merge_index", ts_dev, n + n_other))
        res.update(second_library_records=n_other, merged_records=len(hu), host_route_ms=round((t3 - t0) * 1e3, 1),
                   host_route_export_ms=round((t1 - t0) * 1e3, 1), host_route_unique_ms=round((t2 - t1) * 1e3, 1),
                   host_route_append_ms=round((t3 - t2) * 1e3, 1), host_route_over_merge_index=round((t3 - t0) / min(ts_dev), 1),
                   host_route_note="no LCA on the host: each shared key keeps its first taxon; a lower bound for that route")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
