// respace.hip -- a library with more mask spaces, derived from a resident table: KeyValueIndex.respace
// (S/slacken/KeyValueIndex.scala:353-384) = every record's minimizer ANDed with the wider SpacedSeed mask, then
// groupBy(id columns).agg(TaxonLCA) (:370-379).  The reference shuffles the whole library for the group-by; here the source table
// gives its records back where they lie (the table is lossless: tablebuild.h, cell_key) and the destination table is the group-by
// (tablebuild.h, insert_merge), so the pass is one stream over the source's cells and one insert-or-merge per record.
//
// The pass over the source is tablewalk.h's (merge.hip shares it): a stream over the cells, the occupied ones compacted per wave.
// Records that share a masked key are scattered over the source by fmix64, so merging them inside a wave or a block first
// (wavetools.h: the three levels) would find next to nothing to merge.
//
// The taxon travels as the cell holds it (the dense id on an index that slk_index_finalize renumbered): the destination is given the
// same taxon field and the same id tables.  The source is only read; LCA is associative, commutative and idempotent, so the pass can
// be repeated into a fresh table from scratch (index.hip does when a record finds no cell within the displacement limit).
#include <hip/hip_runtime.h>

#include "hostside.h"
#include "tablewalk.h"

namespace slk {

namespace {

__global__ void __launch_bounds__(TW_BLOCK) respace_kernel(TableView S, TableBuild D, uint64_t new_smask,
                                                           const int32_t *__restrict__ parents, int32_t ntax, uint64_t n) {
  __shared__ TableWalkLds L;
  walk_table_into(S, n, D, parents, ntax, L, [&](uint64_t key, int32_t taxon, uint64_t &out_key, int32_t &out_taxon) {
    out_key = key & new_smask;
    out_taxon = taxon;
    return true;
  });
}

}  // namespace

void launch_respace(const TableView &src, const TableBuild &dst, uint64_t new_smask, const int32_t *parents, int32_t ntax, hipStream_t s) {
  const uint64_t n = src.g.nbuckets * LPB;   // 16-byte elements of the source
  if (n == 0) return;
  hipLaunchKernelGGL(respace_kernel, dim3(table_walk_grid(n)), dim3(TW_BLOCK), 0, s, src, dst, new_smask, parents, ntax, n);
}

}  // namespace slk
