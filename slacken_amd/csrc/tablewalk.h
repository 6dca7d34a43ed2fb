// tablewalk.h -- the pass over the records of a resident table that ends in an insert-or-merge into another table (respace.hip: the
// keys masked; merge.hip: the taxa translated and checked).
//
// The stream: persistent blocks, a grid-stride loop over 16-byte elements (two cells) with TW_UNROLL loads in flight per lane, as
// taxon_counts_kernel reads them.  About half the cells of a table are empty and insert_merge diverges, so the occupied cells of a
// wave are compacted first: they go to a wave-shared LDS queue (wavetools.h: WaveQueue) and are inserted 64 at a time, one
// lane per record.  What bounds such a pass is the random traffic to the destination -- one bucket read and one CAS per record, parent
// walks where the taxa of a group differ -- not the stream.
#pragma once
#include "hostside.h"
#include "tablebuild.h"

namespace slk {

constexpr int TW_BLOCK = 256;
constexpr int TW_WAVES = TW_BLOCK / 64;
constexpr int TW_UNROLL = 4;
constexpr int TW_BLOCKS_PER_CU = 8;   // 32 waves per CU: the inserts wait on HBM round trips, what they need is waves to switch to

struct TableWalkLds {
  uint64_t q_key[TW_WAVES][128];
  int32_t q_tax[TW_WAVES][128];
};

// Every occupied cell of S (n 16-byte elements) as a record: record(key, taxon as the cell holds it, out_key, out_taxon) says whether
// the record goes on, and as what; those that do are inserted or LCA-merged into D (tablebuild.h: insert_merge) and the wave's counts
// reported (report_inserts).  By every thread of a block of TW_BLOCK threads, L in its LDS.
template <class Record>
__device__ __forceinline__ void walk_table_into(const TableView &S, uint64_t n, const TableBuild &D, const int32_t *__restrict__ parents,
                                                int32_t ntax, TableWalkLds &L, Record &&record) {
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
    bool has = (cell & tmask) != 0;
    uint64_t key = 0;
    int32_t taxon = 0;
    if (has) has = record(cell_key(S.g, i, cell), (int32_t)(cell & tmask), key, taxon);
    Q.push(has, key, taxon, insert);
  };

  const uint64_t tile = (uint64_t)TW_BLOCK * TW_UNROLL, stride = (uint64_t)gridDim.x * tile;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n; base += stride) {   // block-uniform: the ballots see whole waves
    ulonglong2 v[TW_UNROLL];
#pragma unroll
    for (int u = 0; u < TW_UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * TW_BLOCK + tid;
      v[u] = i < n ? cells[i] : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < TW_UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * TW_BLOCK + tid;
      push(2 * i, v[u].x);
      push(2 * i + 1, v[u].y);
    }
  }
  Q.drain(insert);
  report_inserts(D, lane, created, failed, max_d);
}

// the grid of such a pass over n 16-byte elements
inline unsigned table_walk_grid(uint64_t n) {
  const uint64_t tile = (uint64_t)TW_BLOCK * TW_UNROLL;
  return (unsigned)std::min<uint64_t>((n + tile - 1) / tile, (uint64_t)grid_for(-1, TW_BLOCKS_PER_CU, nullptr));
}

}  // namespace slk
