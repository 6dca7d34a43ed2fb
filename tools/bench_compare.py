#!/usr/bin/env python3
"""Times of the join of `compare` (compare.hip: slk_compare_*) on synthetic CAMI-like read ids: --rows reference rows (first mates
with /1, their /2 rows beside them for a fifth of the reads) and as many classified rows, nine in ten of which have a reference row.
  binding   add_reference / add_test of the whole text resident on the device (one call each: the line passes, the field pass, the
            table), and from host memory in chunks of 64 MiB (the upload included), in rows/s and GB/s of text
  floor     a plain coalesced read of the same bytes (tools/stream_sum.hip)
  command   `slacken-amd compare --test-files` end to end on the plain files and on their .gz, with and without --host; the command's
            own split (reference mapping / tests, from its last stderr line) beside the wall time -- for --host that is the join by a
            host hash map on the same box
Every figure: the best of --reps runs after a warm-up where one is cheap, with the slowest beside it.  One JSON line on stdout.  Not
part of bench.py; no test gates on these numbers.

  python tools/bench_compare.py --rows 1e7 > profiles/r18_compare.json"""
import argparse
import ctypes as C
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")


def spread(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts), max(ts)


def write_taxonomy(d, genera=200, species_per_genus=10):
    """root > superkingdom > genera > species; the ids are dense from 1"""
    os.makedirs(d)
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom")]
    species = []
    t = 3
    for _ in range(genera):
        g = t
        nodes.append((g, 2, "genus"))
        t += 1
        for _ in range(species_per_genus):
            nodes.append((t, g, "species"))
            species.append(t)
            t += 1
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        f.writelines(f"{a}\t|\t{b}\t|\t{r}\t|\n" for a, b, r in nodes)
    with open(os.path.join(d, "names.dmp"), "w") as f:
        f.writelines(f"{a}\t|\tNode {a}\t|\t\t|\tscientific name\t|\n" for a, _, _ in nodes)
    return np.array(species, np.int32), np.array([a for a, _, r in nodes if r == "genus"], np.int32)


def texts(n, species, genera, rng):
    """(reference mapping, classified rows): ids like S0R<number>-<salt>, the truth a species, the call mostly that species, its genus
    sometimes, another species or nothing now and then"""
    truth = species[rng.integers(0, len(species), n)]
    salt = rng.integers(0, 10**6, n)
    ids = [f"S0R{i}-{s}" for i, s in zip(range(n), salt)]
    paired = rng.random(n) < 0.2
    ref = "".join(f"a{i}\t{rid}/1\t{t}\ng{i}\t{rid}/2\t{t}\n" if p else f"a{i}\t{rid}/1\t{t}\n" for i, (rid, t, p) in enumerate(zip(ids, truth, paired)))
    roll = rng.random(n)
    other = species[rng.integers(0, len(species), n)]
    genus_of = {int(s): int(g) for g in genera for s in species if g < s <= g + 10}
    call = [int(t) if r < 0.7 else genus_of[int(t)] if r < 0.85 else int(o) if r < 0.92 else 0 for t, r, o in zip(truth, roll, other)]
    present = rng.random(n) < 0.9
    order = rng.permutation(n)
    test = "".join(f"{'C' if call[i] else 'U'}\t{ids[i] if present[i] else 'X' + ids[i]}\t{call[i]}\t150\t{call[i]}:90 0:26\n" for i in order)
    return ref.encode(), test.encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    import torch
    import slacken_amd
    n = int(a.rows)
    rng = np.random.default_rng(1)
    work = tempfile.mkdtemp(prefix="slk_bench_compare_")
    species, genera = write_taxonomy(os.path.join(work, "tax"))
    ref, test = texts(n, species, genera, rng)
    ref_rows, test_rows = ref.count(b"\n"), test.count(b"\n")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"rows": n, "reference_rows": ref_rows, "reference_bytes": len(ref), "test_rows": test_rows, "test_bytes": len(test), "reps": a.reps,
           "cli_reps": a.cli_reps, "device": torch.cuda.get_device_name(0), "compute_units": cus,
           "figures": "seconds as [best, slowest] of `reps` runs (the command: `cli_reps` runs, no warm-up)"}

    def rates(rows, nbytes, t):
        return {"s": [round(t[0], 4), round(t[1], 4)], "Mrows_per_s": round(rows / t[0] / 1e6, 1), "GB_per_s": round(nbytes / t[0] / 1e9, 2)}

    # ---- the binding: text resident on the device, one call each
    d_ref = torch.frombuffer(bytearray(ref), dtype=torch.uint8).cuda()
    d_test = torch.frombuffer(bytearray(test), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    handles = []

    def add_reference_device():
        c = slacken_amd.Compare()
        handles.append(c)
        assert c.add_reference_device(d_ref.data_ptr(), len(ref)) == len(ref)

    t_ref = spread(add_reference_device, a.reps)
    c = handles[-1]
    for h in handles[:-1]:
        h.close()
    kept = c.totals()[2]

    def add_test_device():
        c.begin_test()
        assert c.add_test_device(d_test.data_ptr(), len(test)) == len(test)

    t_test = spread(add_test_device, a.reps)
    totals = c.totals()
    res["device_text"] = {"add_reference": rates(ref_rows, len(ref), t_ref), "add_test": rates(test_rows, len(test), t_test),
                          "kept_ids": kept, "joined_rows": totals[4], "distinct_pairs": int(len(c.pairs()[0])),
                          "note": "add_test includes begin_test (the flags of the whole table are cleared); add_reference includes the table's growth from nothing"}
    c.close()
    # ---- the floor: the same bytes read and summed
    S = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    S.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    floor = {}
    for name, d, nbytes in (("reference", d_ref, len(ref)), ("test", d_test, len(test))):
        ms = C.c_float(0)
        assert S.slk_stream_sum(d.data_ptr(), nbytes, cus * 4, a.reps, C.byref(ms), None) == 0
        floor[name] = {"ms": round(ms.value, 3), "GB_per_s": round(nbytes / (ms.value * 1e-3) / 1e9, 1)}
    res["plain_read_of_the_same_bytes"] = floor
    res["device_text"]["add_reference_over_plain_read"] = round(t_ref[0] * 1e3 / floor["reference"]["ms"], 1)
    res["device_text"]["add_test_over_plain_read"] = round(t_test[0] * 1e3 / floor["test"]["ms"], 1)
    del d_ref, d_test
    torch.cuda.empty_cache()

    # ---- the binding: host text in chunks of 64 MiB (pageable memory; the upload is part of the call)
    def chunks(add, text):
        chunk, pos = 64 << 20, 0
        view = np.frombuffer(text, np.uint8)
        while pos < len(text):
            end = min(len(text), pos + chunk)
            used = add(view[pos:end], final=end == len(text))
            assert used > 0
            pos += used

    def add_reference_host():
        c = slacken_amd.Compare()
        handles.append(c)
        chunks(lambda t, final: c.add_reference(t, final=final), ref)

    del handles[:]
    t_ref = spread(add_reference_host, a.reps)
    c = handles[-1]
    for h in handles[:-1]:
        h.close()

    def add_test_host():
        c.begin_test()
        chunks(c.add_test, test)

    t_test = spread(add_test_host, a.reps)
    assert c.totals()[4] == totals[4]
    res["host_text_64MiB_chunks"] = {"add_reference": rates(ref_rows, len(ref), t_ref), "add_test": rates(test_rows, len(test), t_test)}
    c.close()

    # ---- the command, end to end
    if not a.no_cli:
        paths = {"plain": (os.path.join(work, "reads_mapping.tsv"), os.path.join(work, "part-00000.txt"))}
        for p, text in zip(paths["plain"], (ref, test)):
            with open(p, "wb") as f:
                f.write(text)
        paths["gz"] = tuple(p + ".gz" for p in paths["plain"])
        for p, text in zip(paths["gz"], (ref, test)):
            with gzip.open(p, "wb", compresslevel=1) as f:
                f.write(text)
        res["gz_bytes"] = [os.path.getsize(p) for p in paths["gz"]]
        cli, outputs = {}, {}
        for kind, (r, t) in paths.items():
            for mode in ("device", "host"):
                runs = []
                for _ in range(a.cli_reps):
                    t0 = time.perf_counter()
                    p = subprocess.run([CLI, "compare", "-t", os.path.join(work, "tax"), "-r", r, "-o", os.path.join(work, f"o_{kind}_{mode}"),
                                        "--test-files", t] + (["--host"] if mode == "host" else []), capture_output=True, text=True)
                    wall = time.perf_counter() - t0
                    assert p.returncode == 0, p.stderr
                    m = re.search(r"reference mappings \(([0-9.e+-]+) s\), tests ([0-9.e+-]+) s", p.stderr)
                    runs.append((wall, float(m.group(1)), float(m.group(2))))
                    outputs[(kind, mode)] = p.stdout.replace(t, "T")
                bestrun = min(runs)
                cli[f"{kind}_{mode}"] = {"wall_s": [round(bestrun[0], 2), round(max(runs)[0], 2)], "reference_s": round(bestrun[1], 2),
                                         "tests_s": round(bestrun[2], 2)}
        assert len(set(outputs.values())) == 1, "the four runs print different results"
        res["command"] = cli
        res["command_prints"] = outputs[("plain", "device")].split("\n")[1:12]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
