#!/usr/bin/env python3
"""What low-complexity masking costs on one MI355X (profiles/r15_mask.json).  One JSON line on stdout; nothing gates on it.

  mask_device_random     slk_mask_device in Gbp/s on --bases (default 1e9) of uniform random ACGT as sequences of 1 Mbp: almost every
                         tile is clean and ends after the scores-only phase
  mask_device_repeats    the same text with 5 % of it replaced by microsatellites and homopolymers of 20..500 letters (planted into a block
                         of 2^27 letters on the host, the block repeated on the device)
  read_and_sum           tools/stream_sum.hip over the same bytes: the letters read once, the floor
  host_16_threads        mask_sequences_host (slacken_amd/host/mask.hpp, compiled here with -O3) on --host-bases of the second text, 16 threads
  build / build_mask     wall time of `slacken-amd build` and `build --mask` on the library of tools/bench_build.py (--genomes x 1 Mbp),
                         the better of two runs each

  python tools/bench_mask.py --work DIR > profiles/r15_mask.json"""
import argparse
import ctypes as C
import json
import os
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

HOST_MAIN = r"""
#include "mask.hpp"
#include <chrono>
#include <cstdlib>
// argv: file of letters, letters per sequence, threads -> seconds, letters changed
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  std::vector<uint8_t> bases;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint8_t buf[1 << 16];
  for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) bases.insert(bases.end(), buf, buf + got);
  fclose(f);
  const uint64_t per = strtoull(argv[2], nullptr, 10);
  std::vector<uint64_t> offsets;
  for (uint64_t o = 0; o < bases.size(); o += per) offsets.push_back(o);
  offsets.push_back(bases.size());
  const slk_mask_config cfg{64, 20, (uint8_t)'x'};
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t changed = slk_host::mask_sequences_host(bases.data(), offsets.data(), offsets.size() - 1, cfg, (size_t)atoi(argv[3]));
  printf("%f %llu\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), (unsigned long long)changed);
  return 0;
}
"""


def say(what):
    print(f"[bench_mask] {what}", file=sys.stderr, flush=True)


def plant_repeats(block, rng, share=0.05):
    """`share` of the block replaced by repeats of a 1..4-letter unit, 20..500 letters long"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    planted = 0
    while planted < share * block.size:
        n = int(rng.integers(20, 501))
        unit = acgt[rng.integers(0, 4, int(rng.integers(1, 5)))]
        at = int(rng.integers(0, block.size - n))
        block[at:at + n] = np.resize(unit, n)
        planted += n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=1e9)
    ap.add_argument("--host-bases", type=float, default=2 ** 26)
    ap.add_argument("--genomes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--work", required=True, help="scratch directory")
    a = ap.parse_args()
    import torch
    import slacken_amd
    import taxgen
    from slacken_amd import capi
    from bench_build import timed_cli, write_taxonomy
    os.makedirs(a.work, exist_ok=True)
    L = capi.lib()
    rng = np.random.default_rng(15)
    block_n, per = 1 << 27, 1 << 20
    reps_of_block = max(1, -(-int(a.bases) // block_n))   # (whole blocks: 1e9 becomes 2^30)
    n = block_n * reps_of_block
    res = {"date": time.strftime("%Y-%m-%d"), "runs": "one run", "device": torch.cuda.get_device_name(0), "bases": n, "sequence_bases": per,
           "tile_bases": capi.mask_tile_bases(), "reps": a.reps}
    acgt = np.frombuffer(b"ACGT", np.uint8)
    block = acgt[rng.integers(0, 4, block_n, dtype=np.uint8)]
    ix = slacken_amd.Index(expected_records=1024)
    st = ix.stream()
    d_offsets = torch.arange(0, n + 1, per, dtype=torch.int64, device="cuda")
    d_masked = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_work = torch.empty(n, dtype=torch.uint8, device="cuda")
    ss = C.CDLL(os.path.join(ROOT, "slacken_amd", "lib", "libslk_stream_sum.so"))
    ss.slk_stream_sum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg = capi.MaskConfig(64, 20, ord("x"))
    host_file = os.path.join(a.work, "host_letters.bin")
    for name in ("random", "repeats"):
        if name == "repeats":
            plant_repeats(block, rng)
            block[:int(a.host_bases)].tofile(host_file)
        d_block = torch.from_numpy(block).cuda()
        times = []
        for _ in range(a.reps + 1):   # (the first run sizes the stream's scratch and is not counted)
            d_work.view(reps_of_block, block_n).copy_(d_block.unsqueeze(0).expand(reps_of_block, block_n))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = L.slk_mask_device(st.h, d_work.data_ptr(), d_offsets.data_ptr(), d_offsets.numel() - 1, C.byref(cfg), d_masked.data_ptr())
            assert rc == 0, L.slk_last_error()
            st.synchronize()
            times.append(time.perf_counter() - t0)
        best = min(times[1:])
        masked = int(d_masked.cpu()[0])
        res["mask_device_" + name] = dict(seconds=round(best, 5), Gbp_per_s=round(n / best / 1e9, 2), letters_masked=masked,
                                          share_masked=round(masked / n, 5))
        say(f"{name}: {res['mask_device_' + name]}")
        del d_block
    ms = C.c_float(0)
    rc = ss.slk_stream_sum(d_work.data_ptr(), n, cus * 4, a.reps, C.byref(ms), None)
    assert rc == 0, rc
    res["read_and_sum"] = dict(ms=round(ms.value, 3), GB_per_s=round(n / (ms.value / 1e3) / 1e9, 1))
    del d_work
    st.close()
    ix.close()
    torch.cuda.empty_cache()

    # the host statement on 16 threads
    src = os.path.join(a.work, "host_main.cpp")
    with open(src, "w") as f:
        f.write(HOST_MAIN)
    exe = os.path.join(a.work, "host_mask")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-pthread", "-I", os.path.join(ROOT, "slacken_amd", "host"), "-o", exe, src])
    secs, changed = subprocess.run([exe, host_file, str(per), "16"], check=True, capture_output=True, text=True).stdout.split()
    res["host_16_threads"] = dict(bases=int(a.host_bases), seconds=round(float(secs), 3), Gbp_per_s=round(a.host_bases / float(secs) / 1e9, 4),
                                  letters_masked=int(changed))
    say(f"host: {res['host_16_threads']}")

    # build and build --mask on the library of bench_build.py
    from bench_bracken import genomes
    rng = np.random.default_rng(11)
    parents = taxgen.taxonomy(8 * 64, rng)
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
    res["build_library"] = {"bases": int(len(bases)), "genomes": a.genomes}
    del bases
    for name, extra in (("build", []), ("build_mask", ["--mask"])):
        runs = [timed_cli(["build", "-i", os.path.join(a.work, "built", "lib"), "-t", tax, "-l", lib, "--format", "slkrec", *extra])[0] for _ in range(2)]
        res[name] = dict(wall_s=round(min(runs), 2))
        say(f"{name}: {res[name]}")
    shutil.rmtree(a.work, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
