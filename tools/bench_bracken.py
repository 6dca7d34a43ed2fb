"""Bracken weights throughput (slk_bracken_*, bracken.hip): synthetic genomes of 1 Mbp with shared stretches and scattered N runs,
an index built from them on the device (slk_index_add_sequences), then every read of length 100 and 150 at every position.
Prints one JSON line per read length: device read positions per second (slk_bracken_add, host copies included) and the triples.
--cli DIR additionally writes the genomes as a library directory (DIR/library/*.fna, DIR/seqid2taxid.map) with an index of the
same records in the on-disk layout and times `slacken-amd bracken-build` end to end.
The time split by kernel: rocprofv3 --kernel-trace --stats -- python tools/bench_bracken.py --genomes 1024 --lengths 100"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import slacken_amd  # noqa: E402
import taxgen  # noqa: E402


def genomes(n, length, rng, parents):
    taxa = np.array(taxgen.defined_taxa(parents))
    leaves = np.setdiff1d(taxa, parents[taxa])
    src = rng.choice(leaves, size=n, replace=len(leaves) < n).astype(np.int32)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    bases = acgt[rng.integers(0, 4, n * length, dtype=np.uint8)]
    for g in range(1, n):   # a shared 20 kbp stretch with an earlier genome, and a few N runs
        a = int(rng.integers(0, length - 20_000))
        o = int(rng.integers(0, g))
        bases[g * length + a:g * length + a + 20_000] = bases[o * length + a:o * length + a + 20_000]
        for b in rng.integers(0, length - 100, 5):
            bases[g * length + b:g * length + b + int(rng.integers(1, 60))] = ord("N")
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    return bases, offsets, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=2048)
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--lengths", default="100,150")
    ap.add_argument("--cli", default=None, help="directory for the end-to-end bracken-build run")
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    parents = taxgen.taxonomy(8 * 512, rng)
    bases, offsets, src = genomes(a.genomes, a.length, rng, parents)
    ix = slacken_amd.Index(k=35, m=31, spaces=7, expected_records=int(len(bases) * 0.12), max_taxon=len(parents) - 1)
    ix.set_taxonomy(parents)
    t0 = time.perf_counter()
    ix.add_sequences(bases, offsets, src)
    ix.finalize()
    build_s = time.perf_counter() - t0
    st = ix.stream()
    for L in map(int, a.lengths.split(",")):
        bw = slacken_amd.BrackenWeights(ix, L, stream=st)
        t0 = time.perf_counter()
        bw.add(bases, offsets, src)
        dt = time.perf_counter() - t0
        d, s, c = bw.result()
        bw.close()
        reads = int(c.sum())
        print(json.dumps(dict(metric="bracken_read_positions_per_s", read_len=L, bases=int(len(bases)), reads=reads,
                              seconds=round(dt, 3), read_positions_per_s=round(reads / dt), triples=int(len(d)),
                              self_classified=round(float(c[d == s].sum()) / reads, 4), index_build_s=round(build_s, 2))),
              flush=True)
    if a.cli:
        import parquet_to_slkrec as conv
        keys, taxa = ix.export()
        st.close()
        ix.close()
        lib = os.path.join(a.cli, "lib")
        os.makedirs(os.path.join(lib, "library"), exist_ok=True)
        with open(os.path.join(lib, "library", "genomes.fna"), "wb") as f:
            for g in range(len(src)):
                f.write(b">g%d\n" % g)
                f.write(bases[int(offsets[g]):int(offsets[g + 1])].tobytes())
                f.write(b"\n")
        with open(os.path.join(lib, "seqid2taxid.map"), "w") as f:
            for g, t in enumerate(src):
                f.write(f"g{g}\t{t}\n")
        loc = os.path.join(a.cli, "base")
        conv.write_slkrec(loc + ".slkrec", keys, taxa)
        with open(loc + ".properties", "w") as f:
            f.write("k=35\nm=31\nbuckets=1\nversion=1\nsplitter=randomXOR\nminimizerSpaces=7\ncanonical=true\n")
        os.makedirs(loc + "_taxonomy", exist_ok=True)
        with open(os.path.join(loc + "_taxonomy", "nodes.dmp"), "w") as f:
            for t in taxgen.defined_taxa(parents):
                f.write(f"{t}\t|\t{1 if t == 1 else int(parents[t])}\t|\tno rank\t|\n")
        with open(os.path.join(loc + "_taxonomy", "names.dmp"), "w") as f:
            for t in taxgen.defined_taxa(parents):
                f.write(f"{t}\t|\tTaxon {t}\t|\t\t|\tscientific name\t|\n")
        cli = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")
        t0 = time.perf_counter()
        subprocess.run([cli, "bracken-build", "-i", loc, "--library", lib, "--read-len", "100"], check=True)
        dt = time.perf_counter() - t0
        print(json.dumps(dict(metric="bracken_build_cli_s", bases=int(len(bases)), read_len=100, seconds=round(dt, 2))), flush=True)


if __name__ == "__main__":
    main()
