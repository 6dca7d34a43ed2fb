// merge.hip -- libraries united on the device.  A record's taxon is the LCA of the taxa of all sequences that hold its minimizer
// (KeyValueIndex.makeRecords, S/slacken/KeyValueIndex.scala:85-93: groupBy(id).agg(TaxonLCA); LowestCommonAncestor.scala:152-170), and
// LCA is associative, commutative and idempotent: under one taxonomy the records of build(A u B) are the records of build(A) and of
// build(B), merged per key by LCA.  The destination table is that group-by (tablebuild.h: insert_merge), as it is for the library
// builder (build.hip) and for respace.hip; here the records arrive as arrays (a library streamed from disk) or from the cells of
// another resident table (tablewalk.h: the walk respace.hip shares).
//
// Before a record is merged its taxon is translated into the destination's taxonomy (engine.h: MergeCheck -- the remap the host
// derived from the two taxonomies) and checked against it: insert_merge walks parents[] from the taxon, so a taxon that is no
// defined node of the destination must not reach it.  Such records are counted and the smallest offender kept for the message; the
// others are stored.  Both passes are idempotent and can be run again after the table has grown (index.hip: insert_growing).
#include <hip/hip_runtime.h>

#include "hostside.h"
#include "tablewalk.h"

namespace slk {

namespace {

constexpr int MG_BLOCK = 256;
constexpr int MG_UNROLL = 4;
constexpr int MG_BLOCKS_PER_CU = 8;   // as the walk: the inserts wait on HBM round trips

// per lane: what the records that failed the check leave
struct MergeBad {
  int count = 0;
  uint32_t smallest = 0xffffffffu;   // t ^ 0x80000000: unsigned order = signed order of t
};

// the source taxon t (the caller's id, not NONE) as the destination stores it; false: no such node there
__device__ __forceinline__ bool merge_taxon(const MergeCheck &C, int32_t field_max, int32_t t, int32_t &out, MergeBad &bad) {
  int32_t x = t;
  if (C.remap != nullptr && x > 0) x = x < C.n_remap ? C.remap[x] : 0;
  const bool ok = x >= 1 && x < C.T && x <= field_max && (x == 1 || C.parents[x] != 0);
  if (!ok) {
    bad.count++;
    bad.smallest = min(bad.smallest, (uint32_t)t ^ 0x80000000u);
    return false;
  }
  out = x;
  return true;
}

__device__ __forceinline__ void report_bad(const MergeCheck &C, uint32_t lane, const MergeBad &bad) {
  const uint32_t n = wave_sum32((uint32_t)bad.count);
  if (n == 0) return;   // (wave-uniform: wave_sum32 leaves the sum in every lane)
  const uint32_t smallest = ~wave_max32(~bad.smallest);
  if (lane == 0) {
    atomicAdd(C.bad, (unsigned long long)n);
    atomicMin((unsigned int *)(C.bad + 1), smallest);
  }
}

__global__ void __launch_bounds__(MG_BLOCK) merge_records_kernel(TableBuild D, MergeCheck C, const int64_t *__restrict__ keys,
                                                                 const int32_t *__restrict__ taxa, uint64_t n) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const int32_t field_max = (int32_t)((1LL << D.g.taxon_bits) - 1);
  int created = 0, failed = 0, max_d = 0;  // per lane
  MergeBad bad;
  const uint64_t tile = (uint64_t)MG_BLOCK * MG_UNROLL, stride = (uint64_t)gridDim.x * tile;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n; base += stride) {
    int64_t k[MG_UNROLL];
    int32_t t[MG_UNROLL];
#pragma unroll
    for (int u = 0; u < MG_UNROLL; u++) {   // the loads of a tile, all in flight before the first insert
      const uint64_t i = base + (uint64_t)u * MG_BLOCK + tid;
      k[u] = i < n ? keys[i] : 0;
      t[u] = i < n ? taxa[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < MG_UNROLL; u++) {
      int32_t x;
      if (t[u] == 0 || !merge_taxon(C, field_max, t[u], x, bad)) continue;   // (NONE: skipped, as slk_index_append skips it)
      const int r = insert_merge(D, C.parents, C.T, (uint64_t)k[u], x, max_d);
      created += (r == 1);
      failed += (r < 0);
    }
  }
  report_inserts(D, lane, created, failed, max_d);
  report_bad(C, lane, bad);
}

__global__ void __launch_bounds__(TW_BLOCK) merge_index_kernel(TableView S, TableBuild D, MergeCheck C, uint64_t n) {
  __shared__ TableWalkLds L;
  const int32_t field_max = (int32_t)((1LL << D.g.taxon_bits) - 1);
  MergeBad bad;
  walk_table_into(S, n, D, C.parents, C.T, L, [&](uint64_t key, int32_t taxon, uint64_t &out_key, int32_t &out_taxon) {
    out_key = key;
    return merge_taxon(C, field_max, ext_taxon(S, taxon), out_taxon, bad);   // (the caller's id where the source was renumbered)
  });
  report_bad(C, threadIdx.x & 63, bad);
}

}  // namespace

void launch_merge_records(const TableBuild &dst, const MergeCheck &c, const int64_t *keys, const int32_t *taxa, uint64_t n, hipStream_t s) {
  if (n == 0) return;
  const uint64_t tile = (uint64_t)MG_BLOCK * MG_UNROLL;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + tile - 1) / tile, (uint64_t)grid_for(-1, MG_BLOCKS_PER_CU, nullptr));
  hipLaunchKernelGGL(merge_records_kernel, dim3(grid), dim3(MG_BLOCK), 0, s, dst, c, keys, taxa, n);
}

void launch_merge_index(const TableView &src, const TableBuild &dst, const MergeCheck &c, hipStream_t s) {
  const uint64_t n = src.g.nbuckets * LPB;   // 16-byte elements of the source
  if (n == 0) return;
  hipLaunchKernelGGL(merge_index_kernel, dim3(table_walk_grid(n)), dim3(TW_BLOCK), 0, s, src, dst, c, n);
}

}  // namespace slk
