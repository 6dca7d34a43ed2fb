#!/usr/bin/env python3
"""Time of slk_index_respace (respace.hip: one pass over a resident table, every record masked and inserted or LCA-merged into a
new table) on a library whose keys merge -- the generator of tests/respace_model.py at scale: classes of 1-64 records (geometric,
p = 1/4) that share their key at 12 spaces, taxa of a taxgen.taxonomy(400), for every other class from one clade -- beside three
yardsticks measured in the same run:
  stream     slk_index_taxon_counts on the source: the cells read once, coalesced (what the pass cannot beat)
  insert     slk_index_append_device of the already masked, already unique keys into a table of the size respace gives its own:
             the insertions without the stream, the decoding and the merges
  host       what there was before: slk_index_export, mask and numpy.unique on the host, slk_index_append -- WITHOUT the LCA of the
             groups (each keeps its first taxon), so a lower bound for that route
Best of --reps after a warm-up call (the host route: one run).  One JSON line on stdout.  Not part of bench.py; no test gates on it.

  python tools/bench_respace.py --records 2e8 > profiles/r08_respace.json"""
import argparse
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
    ap.add_argument("--records", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--from-spaces", type=int, default=7)
    ap.add_argument("--to-spaces", type=int, default=12)
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    import torch
    import respace_model as rm
    import slacken_amd
    import taxgen
    dev = "cuda"
    n_target, m, s_old, s_new = int(a.records), 31, a.from_spaces, a.to_spaces
    g = torch.Generator(device=dev).manual_seed(8)
    rng = np.random.default_rng(8)
    parents = taxgen.taxonomy(400, rng)

    def i64(x):   # a 64-bit mask as the signed number torch wants
        return x - (1 << 64) if x >> 63 else x

    # the generator of tests/respace_model.py, on the device
    bits = rm.free_bits(m, s_old, s_new)
    F = 1 << len(bits)
    n_classes = int(n_target / 3.98)
    base = torch.randint(-2**63, 2**63 - 1, (n_classes,), dtype=torch.int64, device=dev, generator=g) & i64(rm.mask(m, s_new))
    base = torch.unique(base)
    base = base[torch.randperm(len(base), device=dev, generator=g)]
    n_classes = len(base)
    u = torch.rand(n_classes, device=dev, generator=g, dtype=torch.float64)
    size = torch.clamp(torch.floor(torch.log1p(-u) / np.log(0.75)).long() + 1, max=min(64, F))   # geometric(1/4), capped
    first = torch.cumsum(size, 0) - size
    class_of = torch.repeat_interleave(torch.arange(n_classes, device=dev), size)
    n = len(class_of)
    j = torch.arange(n, device=dev) - first[class_of]
    aa = torch.randint(0, F, (n_classes,), device=dev, generator=g)
    bb = torch.randint(0, F // 2, (n_classes,), device=dev, generator=g) * 2 + 1
    fills = (aa[class_of] + bb[class_of] * j) % F
    del j, aa, bb
    keys = base[class_of]
    for jbit, b in enumerate(bits):
        keys |= ((fills >> jbit) & 1) << b
    del fills
    # taxa: uniform over the defined taxa; for every other class from the clade of one random node (of at least three taxa)
    defined = np.array(taxgen.defined_taxa(parents), np.int32)
    members = {int(t): [int(t)] for t in defined}
    for t in sorted(members, reverse=True):
        if parents[t] != 0:
            members[int(parents[t])].extend(members[t])
    big = [t for t in members if t != 1 and len(members[t]) >= 3]
    flat = torch.tensor(np.concatenate([members[t] for t in big]), device=dev, dtype=torch.int32)
    lens = torch.tensor([len(members[t]) for t in big], device=dev)
    offs = torch.cumsum(lens, 0) - lens
    taxa = torch.tensor(defined, device=dev)[torch.randint(0, len(defined), (n,), device=dev, generator=g)]
    node = torch.randint(0, len(big), (n_classes,), device=dev, generator=g)[class_of]
    pick = flat[offs[node] + torch.randint(0, 1 << 30, (n,), device=dev, generator=g) % lens[node]]
    taxa = torch.where(class_of % 2 == 0, pick, taxa).contiguous()
    del node, pick, class_of
    order = torch.randperm(n, device=dev, generator=g)
    keys, taxa = keys[order].contiguous(), taxa[order].contiguous()
    del order
    torch.cuda.synchronize()

    src = slacken_amd.Index(spaces=s_old, expected_records=n, max_taxon=len(parents) - 1, device=0)
    chunk = 50_000_000
    for o in range(0, n, chunk):
        c = min(chunk, n - o)
        src.append_device(keys[o:o + c].data_ptr(), taxa[o:o + c].data_ptr(), c)
    src.set_taxonomy(parents)
    src.finalize()
    info = src.info()
    assert info.records == n and info.duplicate_keys == 0
    res = {"records": n, "classes": n_classes, "from_spaces": s_old, "to_spaces": s_new, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "source_table_bytes": int(info.table_bytes), "source_load": round(n / (info.buckets * info.bucket_cells), 3)}

    # the masked, unique keys with one taxon each (the first of the group: no LCA), on the device -- the insertion yardstick's input
    masked = keys & i64(rm.mask(m, s_new))
    uk, inverse = torch.unique(masked, return_inverse=True)
    ut = torch.zeros(len(uk), dtype=torch.int32, device=dev)
    ut[inverse] = taxa
    del masked, inverse, keys, taxa
    torch.cuda.synchronize()
    assert len(uk) == n_classes

    state = {}

    def run_respace():
        if state.get("out") is not None:
            state["out"].close()
        state["out"] = src.respace(s_new)
    t_respace = best(run_respace, a.reps)
    out = state["out"]
    oi = out.info()
    assert oi.records == n_classes and oi.grown == 0, (oi.records, oi.grown)
    res.update(respace_ms=round(t_respace * 1e3, 2), respace_records_per_s=round(n / t_respace), result_records=int(oi.records),
               result_table_bytes=int(oi.table_bytes))

    t_stream = best(src.taxon_counts, a.reps)
    res.update(stream_taxon_counts_ms=round(t_stream * 1e3, 2), stream_records_per_s=round(n / t_stream))

    def run_insert():
        ix = slacken_amd.Index(spaces=s_new, expected_records=n, max_taxon=len(parents) - 1, device=0)
        t = time.perf_counter()
        ix.append_device(uk.data_ptr(), ut.data_ptr(), len(uk))
        state["t_insert"] = min(state.get("t_insert", 1e9), time.perf_counter() - t)
        assert ix.info().records == n_classes
        ix.close()
    for _ in range(a.reps + 1):
        run_insert()
    t_insert = state["t_insert"]
    res.update(insert_unique_ms=round(t_insert * 1e3, 2), insert_unique_keys=n_classes, insert_keys_per_s=round(n_classes / t_insert),
               respace_over_stream=round(t_respace / t_stream, 2), respace_over_insert=round(t_respace / t_insert, 2))

    if not a.no_host_route:
        import ctypes as C
        from slacken_amd import capi
        hk, ht, got = np.zeros(n, np.int64), np.zeros(n, np.int32), C.c_uint64(0)
        t0 = time.perf_counter()
        capi._check(capi.lib().slk_index_export(src.h, hk.ctypes.data, ht.ctypes.data, n, C.byref(got)))   # (the call itself: Index.export sorts)
        t1 = time.perf_counter()
        assert got.value == n
        hm = (hk.view(np.uint64) & np.uint64(rm.mask(m, s_new))).view(np.int64)
        hu, at = np.unique(hm, return_index=True)
        t2 = time.perf_counter()
        ix = slacken_amd.Index(spaces=s_new, expected_records=n, max_taxon=len(parents) - 1, device=0)
        ix.append(hu, ht[at])
        ix.finalize()
        t3 = time.perf_counter()
        assert ix.info().records == n_classes
        ix.close()
        res.update(host_route_ms=round((t3 - t0) * 1e3, 1), host_route_export_ms=round((t1 - t0) * 1e3, 1),
                   host_route_mask_unique_ms=round((t2 - t1) * 1e3, 1), host_route_append_ms=round((t3 - t2) * 1e3, 1),
                   host_route_over_respace=round((t3 - t0) / t_respace, 1))
        gk, _ = out.export()
        assert np.array_equal(gk, hu)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
