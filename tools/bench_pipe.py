#!/usr/bin/env python3
"""slk_pipe from pinned host memory: the world of tools/bench_packed_entry.py (2^22 reads of 150 bp from 1 Gbp of random genomes,
everything in slk_host_alloc memory) cut into calls of 2^17 / 2^20 / 2^22 reads, swept over the pipe's depth, the wire form
(dense validity + offsets, sparse validity + uniform_len), the number of caller threads (a pipe each; every thread classifies ALL
the reads, the rate is the aggregate) and the hit lists (none, merged lists).  Best of 5 after a warm-up, as the other tool; the
taxa of every configuration are compared with one synchronous call.  Prints one JSON object; run on the GPU box.

N_RATE (default 0.01): the share of reads that get one N, so that the exception list is not empty.
--sizes / --depths / --forms / --threads / --hits: comma-separated subsets of the sweep (with SLK_DEBUG_CALL_TIMING=1 for the
wall clocks of a call's phases on stderr)."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

READ_LEN = 150


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="17,20,22", help="log2 of the call sizes")
    ap.add_argument("--depths", default="1,2,3")
    ap.add_argument("--forms", default="dense,sparse")
    ap.add_argument("--threads", default="1,2,4")
    ap.add_argument("--hits", default="0,2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401
    import slacken_amd
    import taxgen
    from slacken_amd import capi
    L = slacken_amd.lib()
    rng = np.random.default_rng(5)
    parents = taxgen.taxonomy(8 * 1024, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    G, GL = 256, 4 << 20
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * GL, dtype=np.uint8)]
    ix = slacken_amd.Index(expected_records=int(G * GL * 0.4), max_taxon=len(parents) - 1)
    ix.set_taxonomy(parents)
    ix.add_sequences(bases, np.arange(G + 1, dtype=np.uint64) * np.uint64(GL), rng.choice(taxa[len(taxa) // 2:], G).astype(np.int32))
    ix.finalize()
    R = 1 << 22
    starts = rng.integers(0, G * GL - READ_LEN, R)
    rb = bases[(starts[:, None] + np.arange(READ_LEN)[None, :]).reshape(-1)]
    del bases
    n_rate = float(os.environ.get("N_RATE", 0.01))
    with_n = np.flatnonzero(rng.random(R) < n_rate)
    rb[with_n * READ_LEN + rng.integers(0, READ_LEN, with_n.size)] = ord("N")
    ro = np.arange(R + 1, dtype=np.uint64) * np.uint64(READ_LEN)
    st = ix.stream()
    want = st.classify_batch(rb, ro, with_hits=False)
    st.set_merged_hits(True)
    probe = st.classify_batch(rb[:(1 << 17) * READ_LEN], ro[:(1 << 17) + 1], with_hits=True)
    st.set_merged_hits(False)
    entries_per_read = float(probe["hit_offsets"][-1]) / (1 << 17)      # merged entries, for the capacity and the bytes that come down
    codes, valid = capi.pack_bases(rb, pinned=True)

    rows = []
    for lg in [int(v) for v in args.sizes.split(",")]:
        S = 1 << lg
        ncalls = R // S
        wpc = S * READ_LEN // 16                                        # words per call (S * 150 is a multiple of 16)
        offs = capi.pinned_array((S + 1,), np.uint64)
        offs[:] = ro[:S + 1]
        exc = []                                                        # per call: (exc_word, exc_bits) in pinned memory
        for c in range(ncalls):
            _, w, b = capi.pack_bases_sparse(rb[c * S * READ_LEN:(c + 1) * S * READ_LEN])
            pw, pb = capi.pinned_array((max(w.size, 1),), np.uint32), capi.pinned_array((max(w.size, 1),), np.uint16)
            pw[:w.size], pb[:w.size] = w, b
            exc.append((pw, pb, int(w.size)))
        n_exc = sum(e[2] for e in exc)
        cap = int(S * entries_per_read * 1.25) + 1024
        for form in args.forms.split(","):
            reads = []
            for c in range(ncalls):
                r = capi._Reads()
                r.codes = codes.ctypes.data + c * wpc * 4
                if form == "dense":
                    r.valid, r.offsets = valid.ctypes.data + c * wpc * 2, offs.ctypes.data
                else:
                    r.exc_word, r.exc_bits, r.n_exc, r.uniform_len = exc[c][0].ctypes.data, exc[c][1].ctypes.data, exc[c][2], READ_LEN
                reads.append(r)
            up = R * READ_LEN / 16 * 4 + (R * READ_LEN / 16 * 2 + (S + 1) * 8 * ncalls if form == "dense" else 6 * n_exc)
            for nthreads in [int(v) for v in args.threads.split(",")]:
                outs = [dict(taxon=capi.pinned_array((R,), np.int32), cls=capi.pinned_array((R,), np.uint8), nd=capi.pinned_array((R,), np.int32),
                             tk=capi.pinned_array((R,), np.int32), hoff=capi.pinned_array((S + 1,), np.uint64),
                             hits=capi.pinned_array((cap,), capi.HIT_DTYPE)) for _ in range(nthreads)]
                for depth in [int(v) for v in args.depths.split(",")]:
                    for hits in [int(v) for v in args.hits.split(",")]:
                        pipes = [slacken_amd.Pipe(ix, depth) for _ in range(nthreads)]
                        for p in pipes:
                            p.set_merged_hits(hits == 2)
                        thr = (C.c_double * 1)(0.0)
                        hit_entries = [0] * nthreads
                        errors = []

                        def work(t):
                            try:
                                p, o = pipes[t], outs[t]
                                flight, entries = [], 0

                                def collect(ticket, c):
                                    capi._check(L.slk_pipe_collect(p.h, ticket, o["taxon"].ctypes.data + c * S * 4, o["cls"].ctypes.data + c * S,
                                                                   o["nd"].ctypes.data + c * S * 4, o["tk"].ctypes.data + c * S * 4,
                                                                   o["hoff"].ctypes.data if hits else None, o["hits"].ctypes.data if hits else None,
                                                                   cap if hits else 0))
                                    return int(o["hoff"][S]) if hits else 0
                                for c in range(ncalls):
                                    if len(flight) == depth:
                                        entries += collect(*flight.pop(0))
                                    ticket = C.c_uint64(0)
                                    capi._check(L.slk_pipe_submit(p.h, S, C.byref(reads[c]), None, 2, thr, 1, hits, C.byref(ticket)))
                                    flight.append((ticket.value, c))
                                for f in flight:
                                    entries += collect(*f)
                                hit_entries[t] = entries
                            except BaseException as e:      # noqa: B036 (handed to the main thread)
                                errors.append(e)

                        def once():
                            ths = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
                            t0 = time.perf_counter()
                            for th in ths:
                                th.start()
                            for th in ths:
                                th.join()
                            dt = time.perf_counter() - t0
                            if errors:
                                raise errors[0]
                            return dt
                        once()                                                        # warm-up: the slots' buffers grow here
                        for o in outs:
                            assert np.array_equal(o["taxon"], want["taxon"][0]) and np.array_equal(o["cls"], want["classified"][0])
                            assert np.array_equal(o["nd"], want["num_distinct"]) and np.array_equal(o["tk"], want["total_kmers"])
                        dt = min(once() for _ in range(args.reps))
                        for p in pipes:
                            p.close()
                        down = R * 13 + (((S + 1) * 8 * ncalls + hit_entries[0] * 8) if hits else 0)
                        rows.append(dict(call_reads=S, depth=depth, form=form, threads=nthreads, hits=hits,
                                         M_reads_per_s=round(nthreads * R / dt / 1e6, 1), GB_per_s_up=round(nthreads * up / dt / 1e9, 2),
                                         GB_per_s_down=round(nthreads * down / dt / 1e9, 2), bytes_up_per_read=round(up / R, 2),
                                         bytes_down_per_read=round(down / R, 2)))
                        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps(dict(reads=R, read_len=READ_LEN, n_rate=n_rate, reps=args.reps, rows=rows)))


if __name__ == "__main__":
    main()
