#!/usr/bin/env python3
"""Rate of slk_migration_add_device (migration.hip: table lookup + three-level pair count) against slk_lookup_device on the same
keys (the same random table read without the count), in two pair distributions:
  realistic  95 % of the records on t1 == t2 over 4096 taxa, the rest moved to one of 64 other ids
  uniform    t1 and t2 uniform over 300 ids each (90 000 pairs: the blocks' LDS maps cannot hold them)
One JSON line on stdout.  Not part of bench.py; no test gates on these numbers.

  python tools/bench_migration.py --reference-records 1e9 --subject-records 5e8 > profiles/migration_rate.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-records", type=float, default=1e9)
    ap.add_argument("--subject-records", type=float, default=5e8)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import slacken_amd
    from slacken_amd import capi
    n_ref, n_sub = int(a.reference_records), int(a.subject_records)
    L = slacken_amd.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    half = n_ref // 2
    ix = slacken_amd.Index(expected_records=n_ref, max_taxon=8192, device=0)
    keys = {}
    t0 = time.time()
    for name, ntax in (("realistic", 4096), ("uniform", 300)):
        k = torch.randint(-2**63, 2**63 - 1, (half,), dtype=torch.int64, device="cuda", generator=g) & ~3
        t = torch.randint(1, ntax + 1, (half,), dtype=torch.int32, device="cuda", generator=g)
        ix.append_device(k.data_ptr(), t.data_ptr(), half)
        pick = torch.randint(0, half, (n_sub,), device="cuda", generator=g)
        sk, t2 = k[pick].contiguous(), t[pick]
        if name == "realistic":
            moved = torch.rand(n_sub, device="cuda", generator=g) >= 0.95
            t1 = torch.where(moved, 5000 + (t2 % 64), t2).to(torch.int32).contiguous()
        else:
            t1 = torch.randint(1, 301, (n_sub,), dtype=torch.int32, device="cuda", generator=g)
        keys[name] = (sk, t1)
        del k, t, pick, t2
    ix.finalize()
    torch.cuda.synchronize()
    load_s = time.time() - t0
    st = ix.stream()
    out = torch.zeros(n_sub, dtype=torch.int32, device="cuda")
    res = {"reference_records": n_ref, "subject_records": n_sub, "table_bytes": int(ix.info().table_bytes), "load_s": round(load_s, 2),
           "device": torch.cuda.get_device_name(0)}

    def best(fn):
        fn()
        st.synchronize()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            st.synchronize()
            ts.append(time.perf_counter() - t)
        return min(ts)

    for name, (sk, t1) in keys.items():
        mig = capi.MinimizerMigration(ix, None, stream=st)
        t_lookup = best(lambda: capi._check(L.slk_lookup_device(ix.h, st.h, sk.data_ptr(), n_sub, out.data_ptr())))
        t_mig = best(lambda: mig.add_device(sk.data_ptr(), t1.data_ptr(), n_sub))
        r1, r2, _, cnt, matched, unmatched = mig.result()
        assert matched == n_sub * (a.reps + 1) and unmatched == 0 and int(cnt.sum()) == matched
        mig.close()
        res[name] = {"lookup_ms": round(t_lookup * 1e3, 3), "migration_ms": round(t_mig * 1e3, 3),
                     "lookup_records_per_s": round(n_sub / t_lookup), "migration_records_per_s": round(n_sub / t_mig),
                     "migration_over_lookup_time": round(t_mig / t_lookup, 3), "distinct_pairs": int(len(cnt))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
