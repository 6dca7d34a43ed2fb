// tablebuild.h -- what the kernels that write records into the table or read them back share (build.hip: library construction and
// export; respace.hip: a table derived from a resident one): the insert-or-merge of one record, and a cell back to its key.
#pragma once
#include "engine.h"
#include "wavetools.h"

namespace slk {

// Insert (key, taxon) or merge the taxon into the existing record.  Returns 1 if a new record was created, 0 if merged (or
// the key belongs to another rank's shard of the table), -1 if no cell could be found within the displacement limit.
__device__ inline int insert_merge(const TableBuild &t, const int32_t *parents, int32_t ntax, uint64_t key, int32_t taxon, int &max_d) {
  const uint64_t h = fmix64(key);
  if (!shard_keeps(t, h)) return 0;
  uint32_t home;
  uint64_t rem_hi;
  table_slot(t.g, h, home, rem_hi);
  const unsigned long long tmask = (1ULL << t.g.taxon_bits) - 1;
  for (int d = 0; d <= t.disp_limit; d++) {
    unsigned long long *bucket = (unsigned long long *)(t.cells + ((uint64_t)table_bucket(t.g, home, (uint32_t)d) * CELLS));
    const unsigned long long tag = rem_hi | (uint64_t)d;
    const unsigned long long val = (tag << t.g.taxon_bits) | (uint32_t)taxon;
    unsigned long long first = 0;
    for (int c = 0; c < CELLS; c++) {
      unsigned long long cur = __hip_atomic_load(&bucket[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == 0) {
        unsigned long long old = atomicCAS(&bucket[c], 0ULL, val);
        if (old == 0) {
          max_d = max(max_d, d);
          return 1;
        }
        cur = old;  // somebody else took this cell: it may be this very key
      }
      if (c == 0) first = cur;
      if (cell_tag(t.g, cur) == tag) {
        for (;;) {
          int32_t old_taxon = (int32_t)(cur & tmask);
          int32_t merged = tax_lca(parents, ntax, old_taxon, taxon);
          if (merged == old_taxon) return 0;
          unsigned long long want = (cur & ~tmask) | (uint32_t)merged;   // (the bucket flag in a first cell's top bit stays)
          unsigned long long prev = atomicCAS(&bucket[c], cur, want);
          if (prev == cur) return 0;
          cur = prev;    // (the taxon was merged by another lane, or the bucket flag was raised meanwhile: again)
        }
      }
    }
    // full, and the key is not here: the record goes on, and the bucket says so from now on (engine.h: TableGeom.flag)
    if (t.g.flag && !(first & t.g.flag)) atomicOr(&bucket[0], (unsigned long long)t.g.flag);
  }
  return -1;
}

// What a wave's lanes counted over their insert_merge calls, to the table's counters: one lane adds the wave's sums.
__device__ __forceinline__ void report_inserts(const TableBuild &t, uint32_t lane, int created, int failed, int max_d) {
  const uint32_t wc = wave_sum32((uint32_t)created), wf = wave_sum32((uint32_t)failed), wd = wave_max32((uint32_t)max_d);
  if (lane == 0) {
    if (wc) atomicAdd(t.n_inserted, (unsigned long long)wc);
    if (wf) atomicAdd(t.n_overflow, (unsigned long long)wf);
    if (wd) atomicMax(t.max_disp, (int)wd);
  }
}

__host__ __device__ inline uint64_t fmix64_inverse(uint64_t x) {
  x ^= x >> 33; x *= 0x9cb4b2f8129337dbULL;  // inverse of 0xc4ceb9fe1a85ec53 mod 2^64
  x ^= x >> 33; x *= 0x4f74430c22a54005ULL;  // inverse of 0xff51afd7ed558ccd mod 2^64
  x ^= x >> 33;
  return x;
}


// The key of the occupied cell at index i of the table: the cell holds the hash remainder and its displacement, the bucket index
// gives the home bucket, and both the range reduction (engine.h: table_hash_of) and fmix64 are invertible.
__device__ __forceinline__ uint64_t cell_key(const TableGeom &g, uint64_t i, uint64_t cell) {
  const uint64_t dmask = (1ULL << g.disp_bits) - 1;
  const uint64_t tag = cell_tag(g, cell);
  const uint64_t bucket = i / CELLS, d = tag & dmask;
  const uint32_t home = (uint32_t)(bucket >= d ? bucket - d : bucket + g.nbuckets - d);
  const uint64_t h = table_hash_of(g, home, tag >> g.disp_bits);
  return fmix64_inverse(h);
}

}  // namespace slk
