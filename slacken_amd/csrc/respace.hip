// respace.hip -- a library with more mask spaces, derived from a resident table: KeyValueIndex.respace
// (S/slacken/KeyValueIndex.scala:353-384) = every record's minimizer ANDed with the wider SpacedSeed mask, then
// groupBy(id columns).agg(TaxonLCA) (:370-379).  The reference shuffles the whole library for the group-by; here the source table
// gives its records back where they lie (the table is lossless: tablebuild.h, cell_key) and the destination table is the group-by
// (tablebuild.h, insert_merge), so the pass is one stream over the source's cells and one insert-or-merge per record.
//
// The stream: persistent blocks, a grid-stride loop over 16-byte elements (two cells) with RS_UNROLL loads in flight per lane, as
// taxon_counts_kernel reads them.  About half the cells of a table are empty and insert_merge diverges, so the occupied cells of a
// wave are compacted first: they go to a wave-shared LDS queue (wavetools.h: WaveQueue) and are inserted 64 at a time, one
// lane per record.  What bounds the pass is the random traffic to the destination -- one bucket read and one CAS per record, parent
// walks where the taxa of a group differ -- not the stream.  Records that share a masked key are scattered over the source by fmix64,
// so merging them inside a wave or a block first (wavetools.h: the three levels) would find next to nothing to merge.
//
// The taxon travels as the cell holds it (the dense id on an index that slk_index_finalize renumbered): the destination is given the
// same taxon field and the same id tables.  The source is only read; LCA is associative, commutative and idempotent, so the pass can
// be repeated into a fresh table from scratch (index.hip does when a record finds no cell within the displacement limit).
#include <hip/hip_runtime.h>

#include "hostside.h"
#include "tablebuild.h"

namespace slk {

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_WAVES = RS_BLOCK / 64;
constexpr int RS_UNROLL = 4;
constexpr int RS_BLOCKS_PER_CU = 8;   // 32 waves per CU: the inserts wait on HBM round trips, what they need is waves to switch to

struct RespaceLds {
  uint64_t q_key[RS_WAVES][128];
  int32_t q_tax[RS_WAVES][128];
};

__global__ void __launch_bounds__(RS_BLOCK) respace_kernel(TableView S, TableBuild D, uint64_t new_smask,
                                                           const int32_t *__restrict__ parents, int32_t ntax, uint64_t n) {
  __shared__ RespaceLds L;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ulonglong2 *__restrict__ cells = (const ulonglong2 *)S.cells;
  const uint64_t tmask = (1ULL << S.g.taxon_bits) - 1;
  WaveQueue<int32_t> Q(L.q_key[wib], L.q_tax[wib], lane);
  int created = 0, failed = 0, max_d = 0;  // per lane

  auto insert = [&](uint32_t e, bool active) {   // the queued records, one per lane
    if (!active) return;
    const int r = insert_merge(D, parents, ntax, L.q_key[wib][e], L.q_tax[wib][e], max_d);
    created += (r == 1);
    failed += (r < 0);
  };
  auto push = [&](uint64_t i, uint64_t cell) {   // cell i of the source, from every lane of the wave at once
    const bool has = (cell & tmask) != 0;
    Q.push(has, has ? cell_key(S.g, i, cell) & new_smask : 0, (int32_t)(cell & tmask), insert);
  };

  const uint64_t tile = (uint64_t)RS_BLOCK * RS_UNROLL, stride = (uint64_t)gridDim.x * tile;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n; base += stride) {   // block-uniform: the ballots see whole waves
    ulonglong2 v[RS_UNROLL];
#pragma unroll
    for (int u = 0; u < RS_UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * RS_BLOCK + tid;
      v[u] = i < n ? cells[i] : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < RS_UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * RS_BLOCK + tid;
      push(2 * i, v[u].x);
      push(2 * i + 1, v[u].y);
    }
  }
  Q.drain(insert);
  report_inserts(D, lane, created, failed, max_d);
}

}  // namespace

void launch_respace(const TableView &src, const TableBuild &dst, uint64_t new_smask, const int32_t *parents, int32_t ntax, hipStream_t s) {
  const uint64_t n = src.g.nbuckets * LPB;   // 16-byte elements of the source
  if (n == 0) return;
  const uint64_t tile = (uint64_t)RS_BLOCK * RS_UNROLL;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + tile - 1) / tile, (uint64_t)grid_for(-1, RS_BLOCKS_PER_CU, nullptr));
  hipLaunchKernelGGL(respace_kernel, dim3(grid), dim3(RS_BLOCK), 0, s, src, dst, new_smask, parents, ntax, n);
}

}  // namespace slk
