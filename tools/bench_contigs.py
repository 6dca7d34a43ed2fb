#!/usr/bin/env python3
"""Contig-length fragments: the piece route against the library of the parent commit, on one MI355X, in one session.

  python tools/bench_contigs.py --parent-lib PATH/libslacken_amd.so --parent-label "parent commit SHA" > profiles/r16_contigs.json
  python tools/bench_contigs.py --parent-lib ... --taxa 131072 --rounds 1 > profiles/r16_contigs_18bit.json   (18-bit taxon ids: larger maps)

Every row also records the bytes of device scratch a FRESH stream held after one call of each variant (slk_stream_split_info).

Synthetic genomes (--genomes x --length random bases, one taxon each) and an index built from them on the device.  Batches of ONE
fragment length -- 100 kbp, 300 kbp, 1 Mbp, 4 Mbp, --batch-bases each -- cut from the genomes at random places, one base in a hundred
substituted.  slk_classify_batch_device without hit lists, timed by the engine's own stream events (slk_stream_last_stage_ms: from
before the first kernel to behind the last, both streams joined) and by the host clock around the call and its synchronisation; a
warm-up, then --reps runs, all listed, the best one quoted.

Every library runs in a process of its own (a process loads one libslacken_amd.so), the two alternating --rounds times: parent,
this tree, parent, this tree.  This tree's library runs every batch three times: with the route off (slk_stream_set_split_long(0): the
routes of the parent), forced on at 2 x 65 536 windows (131 072 bases; the 100 kbp batch is below it by construction), and as the
engine chooses (-1).  The results of all runs of a batch must be the same bytes (a digest of taxon, classified, distinct, total, spans is compared).

One more batch whose contigs each hit more than 128 taxa: a second index over the same genomes cut into 2 kbp chunks, every chunk
labelled with a random taxon, and --many contigs of 300 kbp -- about 150 chunks each.  On the parent that batch overflows the waves'
128-entry maps and is classified again by the staged kernels at the synchronisation, which the stream events do not see: the host
clock is what counts there.

--hits: the same batches WITH hit lists, through slk_classify_batch (host arrays in, lists out: the entry both libraries have), merged
(slk_stream_set_merged_hits, what the command line uses) and un-merged, timed by the host clock around the call -- uploads, the list
stages and the download of the lists are in it, on both sides alike.  This tree's library runs every batch with the threshold forced as
above and slk_stream_set_split_hits off (the parent's routes) and on; the parent's library as it is.

  python tools/bench_contigs.py --hits --parent-lib PATH/libslacken_amd.so --parent-label "parent commit SHA" > profiles/r17_contigs_hits.json

Not part of bench.py; no test gates on these numbers."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = (100_000, 300_000, 1_000_000, 4_000_000)
PIECE_WINDOWS = 65536
FORCED = 2 * PIECE_WINDOWS
ACGT = np.frombuffer(b"ACGT", np.uint8)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def tolerate_older_library():
    """the parent's library lacks the symbols this tree adds: the binding sets their argument types when it loads a library"""
    class Missing:
        argtypes = restype = None

    class Older(ctypes.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if name.startswith("slk_"):
                    return Missing()
                raise
    ctypes.CDLL = Older


def cut_batch(genomes, G, L, n, length, rng):
    starts = rng.integers(0, G, n) * L + rng.integers(0, L - length + 1, n)
    bases = np.concatenate([genomes[s:s + length] for s in starts])
    subs = rng.integers(0, len(bases), len(bases) // 100)
    bases[subs] = ACGT[rng.integers(0, 4, len(subs), dtype=np.uint8)]
    return bases, np.arange(n + 1, dtype=np.uint64) * np.uint64(length)


def child(a):
    has_route = a.lib is None
    if not has_route:
        os.environ["SLACKEN_AMD_LIB"] = a.lib
        tolerate_older_library()
    import torch
    import slacken_amd
    import taxgen
    rng = np.random.default_rng(16)
    G, L = a.genomes, int(a.length)
    parents = taxgen.taxonomy(a.taxa, rng)
    ls = (len(parents) - 2) // taxgen.N_RANKS
    leaves = np.arange(7 * ls + 2, 8 * ls + 2, dtype=np.int32)
    genomes = ACGT[rng.integers(0, 4, G * L, dtype=np.uint8)]

    def index_of(chunk, taxa):
        n = G * L // chunk
        ix = slacken_amd.Index(expected_records=int(G * L * 0.45), max_taxon=len(parents) - 1, device=0)
        ix.set_taxonomy(parents)
        ix.add_sequences(genomes[:n * chunk], np.arange(n + 1, dtype=np.uint64) * np.uint64(chunk), taxa)
        ix.finalize()
        return ix

    def run(st, d_b, d_o, n, total, outs, d_t, d_c):
        t0 = time.perf_counter()
        st.classify_batch_device(d_b.data_ptr(), d_o.data_ptr(), n, total, d_t.data_ptr(), d_c.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                 outs[2].data_ptr(), min_hit_groups=2, thresholds=(0.0, 0.1))
        ev = float(sum(st.last_stage_ms()))     # (synchronises on the call's last event)
        st.synchronize()                        # (... and here a batch whose maps overflowed is classified again)
        return ev, (time.perf_counter() - t0) * 1e3

    def fresh_scratch(min_len, d_b, d_o, n, total, outs, d_t, d_c):
        """the route's device scratch after this one call on a stream of its own (slk_stream_split_info: the buffers' sizes)"""
        s2 = ix_now[0].stream()
        s2.set_split_long(min_len)
        run(s2, d_b, d_o, n, total, outs, d_t, d_c)
        nbytes = s2.split_info()[1]
        s2.close()
        return nbytes

    def measure(st, name, bases, offsets, reps, variants):
        n, total = len(offsets) - 1, int(offsets[-1])
        d_b, d_o = torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()
        outs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        d_t, d_c = torch.zeros(2 * n, dtype=torch.int32, device="cuda"), torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = {}
        for vname, min_len in variants:
            if has_route:
                st.set_split_long(min_len)
            run(st, d_b, d_o, n, total, outs, d_t, d_c)   # warm-up
            times = [run(st, d_b, d_o, n, total, outs, d_t, d_c) for _ in range(reps)]
            h = hashlib.sha1()
            for t in (d_t, d_c, *outs):
                h.update(t.cpu().numpy().tobytes())
            ev, wall = min(t[0] for t in times), min(t[1] for t in times)
            r = dict(fragments=n, bases=total, event_ms=[round(t[0], 3) for t in times], wall_ms=[round(t[1], 3) for t in times],
                     gbp_per_s_events=round(total / ev / 1e6, 2), gbp_per_s_wall=round(total / wall / 1e6, 2), digest=h.hexdigest(),
                     distinct_hit_groups_mean=float(outs[0].float().mean()))
            if has_route:
                r["last_split"] = list(st.last_split())
                r["scratch_bytes_allocated"] = fresh_scratch(min_len, d_b, d_o, n, total, outs, d_t, d_c)
            res[vname] = r
            log(f"  {name} {vname}: {r['gbp_per_s_events']} Gbp/s by events, {r['gbp_per_s_wall']} by the host clock {r['wall_ms']}")
        return res

    variants = [("off", 0), ("forced", FORCED), ("default", -1)] if has_route else [("parent", None)]
    out = {"library": a.label, "device": torch.cuda.get_device_name(0), "batches": {}}
    ix = index_of(L, leaves[np.arange(G) % len(leaves)])
    ix_now = [ix]
    out["records"] = int(ix.info().records)
    out["taxon_bits"] = int(ix.info().taxon_bits)
    st = ix.stream()
    for length in LENGTHS:
        n = max(1, int(a.batch_bases) // length)
        bases, offsets = cut_batch(genomes, G, L, n, length, rng)
        out["batches"][str(length)] = measure(st, f"{length} bases x {n}", bases, offsets, a.reps, variants)
    st.close()
    del ix
    # the contigs that hit more than 128 taxa each
    chunk = 2000
    ix = index_of(chunk, rng.choice(leaves, G * L // chunk).astype(np.int32))
    ix_now[0] = ix
    st = ix.stream()
    bases, offsets = cut_batch(genomes, G, L, a.many, 300_000, rng)
    out["batches"]["many_taxa_300000"] = measure(st, f"more than 128 taxa: 300000 bases x {a.many}", bases, offsets, min(a.reps, 2), variants)
    st.close()
    print(json.dumps(out), flush=True)


def child_hits(a):
    """--hits: one library, every batch with hit lists (module docstring)"""
    has_route = a.lib is None
    if not has_route:
        os.environ["SLACKEN_AMD_LIB"] = a.lib
        tolerate_older_library()
    import torch
    import slacken_amd
    import taxgen
    rng = np.random.default_rng(16)
    G, L = a.genomes, int(a.length)
    parents = taxgen.taxonomy(a.taxa, rng)
    ls = (len(parents) - 2) // taxgen.N_RANKS
    leaves = np.arange(7 * ls + 2, 8 * ls + 2, dtype=np.int32)
    genomes = ACGT[rng.integers(0, 4, G * L, dtype=np.uint8)]
    ix = slacken_amd.Index(expected_records=int(G * L * 0.45), max_taxon=len(parents) - 1, device=0)
    ix.set_taxonomy(parents)
    ix.add_sequences(genomes, np.arange(G + 1, dtype=np.uint64) * np.uint64(L), leaves[np.arange(G) % len(leaves)])
    ix.finalize()
    st = ix.stream()
    if has_route:
        st.set_split_long(FORCED)
    out = {"library": a.label, "device": torch.cuda.get_device_name(0), "batches": {}}
    switches = [("off", False), ("on", True)] if has_route else [("parent", None)]
    for length in LENGTHS:
        n = max(1, int(a.batch_bases) // length)
        bases, offsets = cut_batch(genomes, G, L, n, length, rng)
        total = int(offsets[-1])
        res = {}
        for lists in ("merged", "unmerged"):
            st.set_merged_hits(lists == "merged")
            for vname, on in switches:
                if has_route:
                    st.set_split_hits(on)
                times, got = [], None
                for i in range(a.reps + 1):          # a warm-up, then the runs
                    t0 = time.perf_counter()
                    got = st.classify_batch(bases, offsets, thresholds=(0.0, 0.1), min_hit_groups=2, with_hits=True)
                    if i:
                        times.append((time.perf_counter() - t0) * 1e3)
                h = hashlib.sha1()
                for key in ("taxon", "classified", "num_distinct", "total_kmers", "hit_offsets", "hits"):
                    h.update(np.ascontiguousarray(got[key]).tobytes())
                r = dict(fragments=n, bases=total, wall_ms=[round(t, 3) for t in times], gbp_per_s_wall=round(total / min(times) / 1e6, 2),
                         digest=h.hexdigest(), entries=int(len(got["hits"])))
                if has_route:
                    r["last_split"] = list(st.last_split())
                res[f"{vname}_{lists}"] = r
                log(f"  {length} bases x {n}, {lists} lists, {vname}: {r['gbp_per_s_wall']} Gbp/s by the host clock {r['wall_ms']}, {r['entries']} entries")
                del got
        out["batches"][str(length)] = res
    st.close()
    print(json.dumps(out), flush=True)


def main_hits(a, common):
    runs = []
    for rnd in range(a.rounds):
        for lib in (os.path.abspath(a.parent_lib), None):
            log(f"round {rnd}: {'parent' if lib else 'this tree'}")
            p = subprocess.run(common + ["--hits"] + (["--lib", lib, "--label", a.parent_label] if lib else []), stdout=subprocess.PIPE,
                               timeout=a.child_timeout, check=True)
            runs.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    summary = {}
    for name in runs[0]["batches"]:
        row = {}
        for lists in ("merged", "unmerged"):
            per = {}
            for r in runs:
                for v, x in r["batches"][name].items():
                    if v.endswith("_" + lists):
                        per.setdefault(v[:-len(lists) - 1], []).append(x)
            cell = dict(same_results=len({x["digest"] for xs in per.values() for x in xs}) == 1, entries=per["parent"][0]["entries"])
            for v, xs in per.items():
                allms = [t for x in xs for t in x["wall_ms"]]
                cell[v] = dict(gbp_per_s=max(x["gbp_per_s_wall"] for x in xs), gbp_per_s_per_process=[x["gbp_per_s_wall"] for x in xs], ms_all_runs=allms,
                               spread=round((max(allms) - min(allms)) / min(allms), 4))
            cell["last_split"] = per["on"][0]["last_split"]
            cell["on_over_parent"] = round(cell["on"]["gbp_per_s"] / cell["parent"]["gbp_per_s"], 3)
            cell["off_over_parent"] = round(cell["off"]["gbp_per_s"] / cell["parent"]["gbp_per_s"], 3)
            cell["beats_parent_beyond_spread"] = bool(min(cell["parent"]["ms_all_runs"]) > max(cell["on"]["ms_all_runs"]))
            cell["slower_than_parent_beyond_spread"] = bool(max(cell["parent"]["ms_all_runs"]) < min(cell["on"]["ms_all_runs"]))
            row[lists] = cell
        row["fragments"], row["bases"] = runs[0]["batches"][name]["parent_merged"]["fragments"], runs[0]["batches"][name]["parent_merged"]["bases"]
        summary[name] = row
    print(json.dumps(dict(tool="tools/bench_contigs.py --hits", entry="slk_classify_batch, hit lists, host clock around the call", device=runs[0]["device"],
                          genomes=a.genomes, genome_bases=int(a.length), taxonomy_size=a.taxa, batch_bases=int(a.batch_bases), piece_windows=PIECE_WINDOWS,
                          forced_min_len=FORCED, reps=a.reps, rounds=a.rounds, batches=summary, processes=runs), indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libslacken_amd.so of the parent commit")
    ap.add_argument("--genomes", type=int, default=48)
    ap.add_argument("--taxa", type=int, default=4096, help="size of the synthetic taxonomy: its ids set the cells' taxon bits, which size the maps")
    ap.add_argument("--length", type=float, default=4.2e6)
    ap.add_argument("--batch-bases", type=float, default=1e9)
    ap.add_argument("--many", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--hits", action="store_true", help="the batches with hit lists, merged and un-merged, slk_stream_set_split_hits off and on")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-label", default="parent commit", help="how the file names the parent's library, e.g. its commit")
    ap.add_argument("--child-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        return child_hits(a) if a.hits else child(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's libslacken_amd.so (build the parent and copy its library aside)")
    common = [sys.executable, os.path.abspath(__file__), "--child", "--genomes", str(a.genomes), "--length", str(a.length), "--batch-bases",
              str(a.batch_bases), "--many", str(a.many), "--reps", str(a.reps), "--taxa", str(a.taxa)]
    if a.hits:
        return main_hits(a, common)
    runs = []
    for rnd in range(a.rounds):
        for lib in (os.path.abspath(a.parent_lib), None):
            log(f"round {rnd}: {'parent' if lib else 'this tree'}")
            # (a fresh process per library, each under its own time limit; a child that fails ends the measurement)
            p = subprocess.run(common + (["--lib", lib, "--label", a.parent_label] if lib else []), stdout=subprocess.PIPE, timeout=a.child_timeout, check=True)
            runs.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    summary, per_name = {}, {}
    for name in runs[0]["batches"]:
        per = {}
        for r in runs:
            for v, x in r["batches"][name].items():
                per.setdefault(v, []).append(x)
        digests = {x["digest"] for xs in per.values() for x in xs}
        row = dict(same_results=len(digests) == 1, fragments=per["parent"][0]["fragments"], bases=per["parent"][0]["bases"])
        clock = "wall" if name.startswith("many_taxa") else "events"
        for v, xs in per.items():
            rates = [x[f"gbp_per_s_{clock}"] for x in xs]       # the best of each process
            allms = [t for x in xs for t in x["wall_ms" if clock == "wall" else "event_ms"]]
            row[v] = dict(gbp_per_s=max(rates), gbp_per_s_per_process=rates, ms_all_runs=allms,
                          spread=round((max(allms) - min(allms)) / min(allms), 4))
        row["clock"] = clock
        row["last_split"] = per["forced"][0]["last_split"]
        row["forced_over_parent"] = round(row["forced"]["gbp_per_s"] / row["parent"]["gbp_per_s"], 3)
        row["off_over_parent"] = round(row["off"]["gbp_per_s"] / row["parent"]["gbp_per_s"], 3)
        row["default_over_parent"] = round(row["default"]["gbp_per_s"] / row["parent"]["gbp_per_s"], 3)
        row["last_split_default"] = per["default"][0]["last_split"]
        row["beats_parent_beyond_spread"] = bool(min(row["parent"]["ms_all_runs"]) > max(row["forced"]["ms_all_runs"]))
        summary[name] = row
        per_name[name] = per
    # scratch: what a fresh stream held after one call of each variant (slk_stream_split_info; this entry takes device arrays, so the
    # host sizes the scratch from total_bases alone -- DESIGN.md 21), and, computed here from the lengths, the bytes of the map ranges
    # the cut handed out: a power of two >= 2 (min(windows, 2^taxon_bits) + 1) entries of 8 bytes per split fragment
    tb = 1 << runs[-1]["taxon_bits"]
    for name, row in summary.items():
        for v in ("off", "forced", "default"):
            row[v]["scratch_bytes_allocated"] = per_name[name][v][0]["scratch_bytes_allocated"]
        frag_len = row["bases"] // row["fragments"]
        cap = 64
        while cap < 2 * (min(frag_len - 34, tb) + 1):
            cap <<= 1
        row["map_bytes_handed_out_computed"] = row["last_split"][0] * cap * 8
    qualifying = [int(n) for n, row in summary.items() if n.isdigit() and int(n) >= FORCED and row["beats_parent_beyond_spread"]]
    print(json.dumps(dict(tool="tools/bench_contigs.py", device=runs[0]["device"], genomes=a.genomes, genome_bases=int(a.length), taxonomy_size=a.taxa, records=runs[0]["records"],
                          taxon_bits=runs[-1]["taxon_bits"], piece_windows=PIECE_WINDOWS, forced_min_len=FORCED, reps=a.reps, rounds=a.rounds,
                          batches=summary, lengths_where_the_route_beats_the_parent_beyond_the_spread=sorted(qualifying),
                          smallest_qualifying_length=min(qualifying) if qualifying else None, processes=runs), indent=1))


if __name__ == "__main__":
    main()
