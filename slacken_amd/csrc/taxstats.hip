// taxstats.hip -- records per taxon of a resident table: records.groupBy("taxon").agg(count("*")) (S/slacken/KeyValueIndex.scala:241,
// :278), the one number that `stats` (showIndexStats :240-251, the depth histograms :326-336) and `inspect` (report :274-306) are
// functions of.  The taxon sits in the low taxon_bits of every cell, so the count is one streaming pass over the cells: whole
// buckets are read coalesced, 16 B (two cells) per lane, as table_lookup reads them; a cell whose taxon field is 0 is empty (an
// occupied cell has taxon != 0, and the top bit of a bucket's first cell -- TableGeom.flag -- lies outside the field).
//
// The count has the three levels of wavetools.h, so that the few high LCAs that hold a large share of a real library's records do
// not serialise on a handful of HBM addresses: TS_LEADER_ROUNDS rounds in the wave, the lanes under the leader's taxon counted with
// a ballot; a map taxon -> uint32 in LDS (TS_SLOTS slots, at most TS_PROBES probes); the device-wide counters, one 64-bit atomic
// per occupied LDS slot at the end of the block.  A block's LDS counters are 32-bit; a launch covers at most TS_LAUNCH_MAX = 2^30
// 16-byte loads = 2^31 cells (the host cuts larger tables into several launches), so no block can see as many as 2^32 records
// between two flushes.
//
// The device-wide counters are an array of uint64 indexed by the taxon the cells hold (the dense internal id when the index has
// them: at most 2^22 entries, 32 MiB).  An index whose cells hold caller ids of more than 22 bits (not finalized yet, or no
// taxonomy to renumber by; the cell layout allows up to 28) would need up to 2 GiB that way for a few thousand counters; its
// counters are a pairmap.h map keyed by the taxon instead, doubled and the pass repeated when it fills (the pass changes nothing,
// so it can be repeated).
#include "hostside.h"
#include "pairmap.h"
#include "wavetools.h"

namespace {

// 512 lanes and 4096 slots (32 KiB of the CU's 160 KiB LDS): four blocks, 32 waves per CU -- the pass is a stream, what it needs is
// loads in flight (TS_UNROLL x 16 B per lane), and the ~4000 taxa that hold most records of a standard library fit a block's map.
constexpr int TS_BLOCK = 512;
constexpr uint32_t TS_SLOTS = 4096;
constexpr int TS_PROBES = 16;
constexpr int TS_LEADER_ROUNDS = 2;
constexpr int TS_BLOCKS_PER_CU = 4;
constexpr int TS_UNROLL = 4;
constexpr uint64_t TS_LAUNCH_MAX = 1ULL << 30;   // 16-byte loads of one launch
constexpr int TS_ARRAY_BITS = 22;                // counters as an array up to 2^22 taxa, as a map beyond

struct TsArgs {
  const ulonglong2 *cells;         // the table, two cells per element
  uint64_t n;                      // elements of this launch
  uint64_t tmask;                  // 2^taxon_bits - 1
  unsigned long long *counts;      // array route: [domain]
  uint64_t domain;
  unsigned long long *map_keys, *map_counts;   // map route (counts == nullptr)
  uint64_t map_mask;
  unsigned long long *totals;      // [0] distinct taxa, [1] records
  int32_t *status;                 // bit 1: the map is full; bit 2: a cell's taxon lies outside the array
};

__device__ __forceinline__ void ts_global_add(const TsArgs &A, uint32_t taxon, unsigned long long c) {
  if (A.counts != nullptr) {
    if (taxon >= A.domain) { atomicOr(A.status, 4); return; }
    if (atomicAdd(&A.counts[taxon], c) == 0) atomicAdd(A.totals + 0, 1ULL);   // (every addend is positive: 0 is seen once per taxon)
  } else if (!pair_map_add(A.map_keys, A.map_counts, A.map_mask, (unsigned long long)taxon, c, A.totals + 0)) {
    atomicOr(A.status, 2);
  }
}

using TsMap = LdsCountMap<unsigned int, 0u, TS_SLOTS, TS_PROBES, true>;   // by taxon; 0: free (no record has taxon 0)

__device__ __forceinline__ void ts_block_add(const TsArgs &A, TsMap &M, unsigned int *lcounts, uint32_t taxon, unsigned int c) {
  M.add(taxon, (taxon * 0x9E3779B1u) >> 20, [&](uint32_t h) { atomicAdd(&lcounts[h], c); }, [&] { ts_global_add(A, taxon, c); });
}

// the wave's lanes hand in one taxon each (0: none)
__device__ __forceinline__ void ts_wave_add(const TsArgs &A, TsMap &M, unsigned int *lcounts, int lane, uint32_t taxon) {
  bool have = taxon != 0;
  for (int round = 0; round < TS_LEADER_ROUNDS; round++) {
    const bool any = leader_round(have, taxon, [&](int leader, uint32_t lt, bool same) {
      const uint64_t group = __ballot(same);
      if (lane == leader) ts_block_add(A, M, lcounts, lt, (unsigned int)__popcll(group));
      have = have && !same;
    });
    if (!any) return;
  }
  if (have) ts_block_add(A, M, lcounts, taxon, 1u);
}

__global__ void __launch_bounds__(TS_BLOCK) taxon_counts_kernel(TsArgs A) {
  __shared__ TsMap M;
  __shared__ unsigned int lcounts[TS_SLOTS];
  M.clear(threadIdx.x, TS_BLOCK, [&](uint32_t s) { lcounts[s] = 0; });
  const int lane = threadIdx.x & 63;
  uint64_t n_records = 0;   // of this wave (every lane keeps the same number)
  const uint64_t tile = (uint64_t)TS_BLOCK * TS_UNROLL, stride = (uint64_t)gridDim.x * tile;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < A.n; base += stride) {   // block-uniform: the ballots see whole waves
    ulonglong2 v[TS_UNROLL];
#pragma unroll
    for (int u = 0; u < TS_UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * TS_BLOCK + threadIdx.x;
      v[u] = i < A.n ? A.cells[i] : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < TS_UNROLL; u++) {
      const uint32_t t0 = (uint32_t)(v[u].x & A.tmask), t1 = (uint32_t)(v[u].y & A.tmask);
      n_records += (uint64_t)__popcll(__ballot(t0 != 0)) + (uint64_t)__popcll(__ballot(t1 != 0));
      ts_wave_add(A, M, lcounts, lane, t0);
      ts_wave_add(A, M, lcounts, lane, t1);
    }
  }
  if (lane == 0 && n_records) atomicAdd(A.totals + 1, (unsigned long long)n_records);
  M.drain(threadIdx.x, TS_BLOCK, [&](uint32_t taxon, uint32_t s) { ts_global_add(A, taxon, (unsigned long long)lcounts[s]); });
}

// The non-zero counters as (taxon, count) pairs, the taxon in the caller's ids (ext_taxon).  The pairs leave in any order -- their
// number is known (totals[0]), a few thousand to a few hundred thousand, and the host sorts them.
__global__ void __launch_bounds__(256) taxon_pairs_kernel(TableView T, const unsigned long long *__restrict__ counts, uint64_t domain,
                                                          int32_t *__restrict__ taxa, unsigned long long *__restrict__ out,
                                                          uint64_t capacity, unsigned long long *__restrict__ cursor) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < domain; base += stride) {   // wave-uniform trip count
    const uint64_t t = base + threadIdx.x;
    const unsigned long long c = t < domain ? counts[t] : 0;
    const bool has = c != 0;
    const unsigned long long slot = wave_alloc_slots(has, cursor);   // one atomic per wave: the lanes' output slots are consecutive
    if (has && slot < capacity) {
      taxa[slot] = ext_taxon(T, (int32_t)t);
      out[slot] = c;
    }
  }
}

struct TsRun {
  DevBuf counts, small, d_taxa, d_out;   // small: totals[2], cursor, status
  PairMap map;
  unsigned long long totals[2] = {0, 0};
  int32_t status = 0;
};

// one pass over the table into R's (zeroed) counters; synchronises s
int32_t ts_pass(const slk_index *ix, hipStream_t s, TsRun &R, uint64_t domain, unsigned blocks) {
  TsArgs A{};
  A.tmask = (1ULL << ix->taxon_bits) - 1;
  A.counts = domain ? R.counts.as<unsigned long long>() : nullptr;
  A.domain = domain;
  A.map_keys = R.map.k(); A.map_counts = R.map.c(); A.map_mask = R.map.cap ? R.map.cap - 1 : 0;
  A.totals = R.small.as<unsigned long long>();
  A.status = (int32_t *)(R.small.as<unsigned long long>() + 3);
  const uint64_t n = ix->nbuckets * LPB;   // 16-byte elements of the table
  for (uint64_t o = 0; o < n; o += TS_LAUNCH_MAX) {
    A.cells = (const ulonglong2 *)ix->cells.get() + o;
    A.n = std::min(TS_LAUNCH_MAX, n - o);
    const uint64_t tile = (uint64_t)TS_BLOCK * TS_UNROLL;
    const unsigned grid = (unsigned)std::min<uint64_t>((A.n + tile - 1) / tile, blocks);
    hipLaunchKernelGGL(taxon_counts_kernel, dim3(grid), dim3(TS_BLOCK), 0, s, A);
    HIPCHK(hipGetLastError());
  }
  unsigned long long h[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, R.small.p, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  R.totals[0] = h[0]; R.totals[1] = h[1];
  R.status = (int32_t)(uint32_t)h[3];
  return SLK_OK;
}

}  // namespace

extern "C" int32_t slk_index_taxon_counts(const slk_index *ix, int32_t *taxa, uint64_t *counts, uint64_t capacity, uint64_t *n_taxa,
                                          uint64_t *n_records) {
  if (!ix || !n_taxa || (capacity && (!taxa || !counts))) return fail(SLK_E_INVALID, "null argument");
  *n_taxa = 0;
  if (n_records) *n_records = 0;
  int32_t rc = set_device(ix);   // (a spent index: SLK_E_STATE)
  if (rc) return rc;
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "taxon counts support minimizers of up to 32 nt (one id column)");
  hipStream_t s = ix->build_stream;   // the stream the records were inserted on: the pass sees them all
  // SLK_TAXSTATS_BLOCKS: the grid (tests: a grid whose stride does not divide the table; measurements: occupancy)
  const unsigned blocks = grid_for(ix->device, TS_BLOCKS_PER_CU, "SLK_TAXSTATS_BLOCKS");

  // the ids the cells hold: dense ranks 1 .. D, or the caller's ids below 2^taxon_bits
  const uint64_t ids = ix->D ? (uint64_t)ix->D + 1 : 1ULL << ix->taxon_bits;
  const bool as_array = ids <= (1ULL << TS_ARRAY_BITS);
  TsRun R;
  HIPCHK(R.small.ensure(32));
  std::vector<std::pair<int32_t, uint64_t>> pairs;
  if (as_array) {
    HIPCHK(R.counts.ensure(ids * 8));
    HIPCHK(hipMemsetAsync(R.counts.p, 0, ids * 8, s));
    HIPCHK(hipMemsetAsync(R.small.p, 0, 32, s));
    rc = ts_pass(ix, s, R, ids, blocks);
    if (rc) return rc;
    if (R.status & 4) return fail(SLK_E_STATE, "taxon counts: a cell holds a taxon beyond the index's %llu internal ids", (unsigned long long)ids);
    const uint64_t n = R.totals[0];
    if (n && capacity) {   // (all n pairs, also when fewer are asked for: the first `capacity` in ascending taxon are owed)
      HIPCHK(R.d_taxa.ensure(n * 4));
      HIPCHK(R.d_out.ensure(n * 8));
      hipLaunchKernelGGL(taxon_pairs_kernel, dim3((unsigned)std::min<uint64_t>((ids + 255) / 256, 4096)), dim3(256), 0, s, ix->view(),
                         R.counts.as<unsigned long long>(), ids, R.d_taxa.as<int32_t>(), R.d_out.as<unsigned long long>(), n,
                         R.small.as<unsigned long long>() + 2);
      HIPCHK(hipGetLastError());
      std::vector<int32_t> ht(n);
      std::vector<unsigned long long> hc(n);
      HIPCHK(hipMemcpyAsync(ht.data(), R.d_taxa.p, n * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(hc.data(), R.d_out.p, n * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      pairs.resize(n);
      for (uint64_t i = 0; i < n; i++) pairs[i] = {ht[i], (uint64_t)hc[i]};
    }
  } else {
    // 2^16 taxa to start with (1 MiB): more than a standard library stores
    int log2 = (int)std::min(31L, std::max(4L, env_long("SLK_TAXSTATS_MAP_LOG2", 16)));
    for (;; log2++) {
      rc = R.map.reset(s, 1ULL << log2);
      if (rc) return rc;
      HIPCHK(hipMemsetAsync(R.small.p, 0, 32, s));
      rc = ts_pass(ix, s, R, 0, blocks);
      if (rc) return rc;
      if (!(R.status & 2)) break;
      if (log2 >= 31) return fail(SLK_E_CAPACITY, "taxon counts: more distinct taxa than a map of 2^31 slots holds");
    }
    if (capacity) {
      std::vector<uint64_t> hk, hc;
      rc = R.map.read(s, hk, hc);
      if (rc) return rc;
      pairs.resize(hk.size());
      for (size_t i = 0; i < hk.size(); i++) pairs[i] = {(int32_t)(uint32_t)hk[i], hc[i]};   // (no dense ids here: ids as given)
    }
  }
  *n_taxa = R.totals[0];
  if (n_records) *n_records = R.totals[1];
  std::sort(pairs.begin(), pairs.end());
  for (size_t i = 0; i < pairs.size() && i < capacity; i++) { taxa[i] = pairs[i].first; counts[i] = pairs[i].second; }
  if (capacity && capacity < R.totals[0])
    return fail(SLK_E_CAPACITY, "%llu taxa, capacity %llu", (unsigned long long)R.totals[0], (unsigned long long)capacity);
  return SLK_OK;
}
