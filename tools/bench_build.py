#!/usr/bin/env python3
"""What `build` costs, piece by piece, on one MI355X.  Best of --reps after a warm-up; one JSON line on stdout.

On a resident table of --records random records (4 000 taxa), exported in pieces of --piece-buckets table buckets into pinned host
buffers, as the CLI does:
  grouped_200 / grouped_2000   slk_index_export_range with n_groups 200 (Spark's default partitions) and 2000: LDS histograms
  grouped_200_device_counters  the same with SLK_EXPORT_LDS_GROUPS=4: one device atomic per record
  ungrouped                    the same pieces with n_groups 0 (build.hip's compacting pass)
  export                       slk_index_export of the whole table (pageable host arrays, as its callers have them)
  read_and_sum                 tools/stream_sum.hip over as many bytes as the table has: the cells read once
  copy_to_host                 12 bytes per record from device to pinned host memory, by itself
The floor of the grouped export is two reads of the cells plus the 12 bytes per record that leave: 2 x read_and_sum + copy_to_host.
The writer alone: the first --writer-records records as a .slkrec library, rewritten as bucketed Parquet by `copy-records` with the
rows dealt out and written on one thread (SLK_WRITER_SERIAL=1, as it was) and with host dealing plus the grouped, pooled path.
Then `build` end to end on the synthetic library of tools/bench_bracken.py (--genomes x 1 Mbp), with the split of the wall clock it
prints, by both routes from table to files (SLK_EXPORT_GROUPED=0: ungrouped pieces dealt on the host).
Not part of bench.py; no test gates on these numbers.

  python tools/bench_build.py --work DIR > profiles/r09_build.json"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts)


def write_taxonomy(d, parents):
    import taxgen
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for t in taxgen.defined_taxa(parents):
            f.write(f"{t}\t|\t{1 if t == 1 else int(parents[t])}\t|\tno rank\t|\n")
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for t in taxgen.defined_taxa(parents):
            f.write(f"{t}\t|\tTaxon {t}\t|\t\t|\tscientific name\t|\n")


def say(what):
    print(f"[bench_build] {what}", file=sys.stderr, flush=True)


def timed_cli(args, env=None):
    t0 = time.perf_counter()
    r = subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(map(str, args))} failed:\n{r.stderr}")
    return dt, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--piece-buckets", type=int, default=1 << 23)
    ap.add_argument("--writer-records", type=float, default=5e7)
    ap.add_argument("--genomes", type=int, default=1024)
    ap.add_argument("--work", required=True, help="scratch directory for the libraries")
    a = ap.parse_args()
    import torch
    import slacken_amd
    import taxgen
    from slacken_amd import capi
    n, chunk = int(a.records), 50_000_000
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"records": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "compute_units": cus, "piece_buckets": a.piece_buckets}
    g = torch.Generator(device="cuda").manual_seed(9)
    ix = slacken_amd.Index(expected_records=n, max_taxon=4095, device=0)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        k = torch.randint(-2**63, 2**63 - 1, (m,), dtype=torch.int64, device="cuda", generator=g) & ~3
        t = torch.randint(1, 4001, (m,), dtype=torch.int32, device="cuda", generator=g)
        ix.append_device(k.data_ptr(), t.data_ptr(), m)
        del k, t
    ix.finalize()
    info = ix.info()
    stored, nb = int(info.records), int(info.buckets)
    res.update(stored_records=stored, table_bytes=int(info.table_bytes), buckets=nb, load=round(stored / (nb * info.bucket_cells), 3))
    piece = min(a.piece_buckets, nb)
    cap = piece * info.bucket_cells
    keys, taxa = capi.pinned_array((cap,), np.int64), capi.pinned_array((cap,), np.int32)
    L = capi.lib()

    def pieces(n_groups):
        offs = np.zeros(n_groups + 1, np.uint64)
        got, total = C.c_uint64(0), 0
        for b0 in range(0, nb, piece):
            capi._check(L.slk_index_export_range(ix.h, b0, min(nb, b0 + piece), n_groups, keys.ctypes.data, taxa.ctypes.data, cap,
                                                 offs.ctypes.data if n_groups else None, C.byref(got)))
            total += got.value
        assert total == stored
    say(f"table of {stored} records resident")
    for name, groups, env in (("grouped_200", 200, None), ("grouped_2000", 2000, None), ("grouped_200_device_counters", 200, "4"),
                              ("ungrouped", 0, None)):
        if env:
            os.environ["SLK_EXPORT_LDS_GROUPS"] = env
        dt = best(lambda: pieces(groups), a.reps)
        os.environ.pop("SLK_EXPORT_LDS_GROUPS", None)
        res[name + "_ms"] = round(dt * 1e3, 1)
        res[name + "_records_per_s"] = round(stored / dt)
        say(f"{name}: {res[name + '_ms']} ms")
    hk, ht, got = np.zeros(stored, np.int64), np.zeros(stored, np.int32), C.c_uint64(0)
    res["export_ms"] = round(best(lambda: capi._check(L.slk_index_export(ix.h, hk.ctypes.data, ht.ctypes.data, stored, C.byref(got))), a.reps) * 1e3, 1)
    S = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    S.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    buf = torch.empty(info.table_bytes // 8, dtype=torch.int64, device="cuda")
    ms = C.c_float(0)
    assert S.slk_stream_sum(buf.data_ptr(), info.table_bytes, cus * 4, a.reps, C.byref(ms), None) == 0
    del buf
    res["read_and_sum_ms"] = round(ms.value, 2)
    # 12 bytes per record to pinned host memory, piece by piece (torch's pinned tensors)
    per_piece = -(-stored // -(-nb // piece))
    dk, dt_ = torch.empty(per_piece, dtype=torch.int64, device="cuda"), torch.empty(per_piece, dtype=torch.int32, device="cuda")
    pk, pt = torch.empty(per_piece, dtype=torch.int64).pin_memory(), torch.empty(per_piece, dtype=torch.int32).pin_memory()

    def copy_out():
        for _ in range(-(-nb // piece)):
            pk.copy_(dk, non_blocking=True)
            pt.copy_(dt_, non_blocking=True)
        torch.cuda.synchronize()
    res["copy_to_host_ms"] = round(best(copy_out, a.reps) * 1e3, 1)
    del dk, dt_, pk, pt
    res["grouped_floor_ms"] = round(2 * res["read_and_sum_ms"] + res["copy_to_host_ms"], 1)
    res["grouped_200_over_floor"] = round(res["grouped_200_ms"] / res["grouped_floor_ms"], 2)

    say("export yardsticks done; the writer alone")
    # the writer alone
    import parquet_to_slkrec as conv
    rng = np.random.default_rng(9)
    parents = taxgen.taxonomy(8 * 512, rng)
    nw = min(int(a.writer_records), stored)
    src = os.path.join(a.work, "writer_src")
    conv.write_slkrec(src + ".slkrec", hk[:nw], ht[:nw])
    for buckets in (200,):
        with open(src + ".properties", "w") as f:
            f.write(f"k=35\nm=31\nbuckets={buckets}\nversion=1\nsplitter=randomXOR\nminimizerSpaces=7\ncanonical=true\n")
        write_taxonomy(src + "_taxonomy", parents)
        w = {"records": nw, "buckets": buckets}
        for name, env in (("serial_s", {"SLK_WRITER_SERIAL": "1"}), ("dealt_on_host_and_pooled_s", {})):
            w[name] = round(min(timed_cli(["copy-records", "-i", src, "-o", os.path.join(a.work, "writer_out"), "--format", "parquet"], env)[0]
                                for _ in range(2)), 2)
            say(f"writer {name}: {w[name]} s")
        res["writer_alone"] = w
    del hk, ht
    ix.close()
    torch.cuda.empty_cache()

    # build end to end
    from bench_bracken import genomes
    rng = np.random.default_rng(11)
    bases, offsets, taxa_of = genomes(a.genomes, 1 << 20, rng, parents)
    lib = os.path.join(a.work, "lib")
    os.makedirs(os.path.join(lib, "library"), exist_ok=True)
    with open(os.path.join(lib, "library", "genomes.fna"), "wb") as f:
        for i in range(len(taxa_of)):
            f.write(b">g%d\n" % i)
            f.write(bases[int(offsets[i]):int(offsets[i + 1])].tobytes())
            f.write(b"\n")
    with open(os.path.join(lib, "seqid2taxid.map"), "w") as f:
        for i, t in enumerate(taxa_of):
            f.write(f"g{i}\t{t}\n")
    tax = os.path.join(a.work, "taxonomy")
    write_taxonomy(tax, parents)
    say("library written")
    e2e = {"bases": int(len(bases)), "genomes": a.genomes}
    del bases
    for name, env in (("grouped_on_device", {}), ("dealt_on_host", {"SLK_EXPORT_GROUPED": "0"})):
        runs = []
        for _ in range(2):   # (the first run also warms the page cache with the genomes)
            dt, err = timed_cli(["build", "-i", os.path.join(a.work, "built", "lib"), "-t", tax, "-l", lib], env)
            line = next(l for l in err.split("\n") if l.startswith("build: "))
            num = lambda pat: float(re.search(pat, line).group(1))   # noqa: E731
            runs.append(dict(wall_s=round(dt, 2), records=int(num(r"(\d+) records")), read_and_parse_s=num(r"read and parse ([\d.e+-]+) s"),
                             add_sequences_s=num(r"add_sequences ([\d.e+-]+) s"), waited_for_add_s=num(r"waited for it ([\d.e+-]+) s\); export"),
                             export_s=num(r"export ([\d.e+-]+) s"), pieces=int(num(r"in (\d+) pieces")),
                             waited_for_writer_s=num(r"beside the writer \(waited for it ([\d.e+-]+) s\)"), export_and_write_s=num(r"\), ([\d.e+-]+) s in all")))
        e2e[name] = min(runs, key=lambda r: r["wall_s"])
        say(f"build {name}: {e2e[name]}")
    res["build_end_to_end"] = e2e
    shutil.rmtree(os.path.join(a.work, "built"), ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
