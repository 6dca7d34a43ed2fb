// coverage.hip -- genome coverage of a library against a resident index: IndexStatistics.showTaxonFullCoverageStats
// (S/slacken/IndexStatistics.scala:86-111) and the k-mers per source taxon of totalKmerCountReport (:38-52).  The reference finds every
// super-mer's minimizer of every labelled genome (SplitterMinimizers.find, S/slacken/Minimizers.scala:43-76: one (minimizer, source
// taxon) row per super-mer, with repetitions), groups the rows by (minimizer, source) into countAll and countDistinct = 1 (:91),
// inner-joins them with the records (:99-100) and groups again by (source, depth(record's LCA taxon)) into sumAll and sumDistinct
// (:101-102).  Here:
//   scan   coverage_scan_kernel, the lane-per-chunk scan of chunkscan.h with exact seams: one lane per chunk of BUILD_CHUNK_WINDOWS windows,
//          every super-mer's minimizer looked up in the table (the one random HBM request per super-mer); a hit adds 1 to a
//          device-wide pair map (pairmap.h) under (cell of the record << 28 | source ordinal) -- the first group-by and the join.
//          The record's position stands for the minimizer: a 32-nt minimizer fills all 64 bits, the cell index needs 36.
//   fold   coverage_fold_kernel, one streaming pass over the pair map's slots: the cell's taxon (one 8-byte random load), its depth,
//          and (all += count, distinct += 1) under (source ordinal, depth) in a second, small map -- the second group-by.  The slots
//          are emptied as they are read: after a fold the pair map is empty, the (source, depth) sums stay.
// Seams.  A super-mer found twice would be counted twice, so the chunks are cut with exact seams (chunkcut.h, chunkscan.h): the
// priming window of a chunk is neither emitted nor counted as a k-mer.
// The fold counts on the three levels of wavetools.h -- wave ballot, LDS map, device map -- since
// a genome's slots nearly all land on two or three (source, depth) pairs; the scan's per-source totals are combined by the wave
// before they reach the device arrays, since the chunks of a wave mostly belong to one sequence.
#include "chunkcut.h"
#include "chunkscan.h"
#include "hostside.h"
#include "pairmap.h"

#include <unordered_map>

namespace {

constexpr int CV_W = 4;                               // waves per block of the scan (as build.hip's)
constexpr uint32_t CV_PRIME = 1u << 31;               // chunk_src: the chunk starts one base early, its first window only primes
constexpr int CV_ORD_BITS = 28;
constexpr uint32_t CV_ORD_MASK = (1u << CV_ORD_BITS) - 1;
constexpr int CV_LEADER_ROUNDS = 2;
constexpr uint64_t CV_LAUNCH_WANT = 1ULL << 26;       // windows a launch should be able to take when the call has as many (cv_settle)
constexpr uint64_t CV_GROUP_BYTES = 1ULL << 30;       // bases of a host call on the device at a time
// the fold: 512 lanes, 2048 LDS slots of 20 bytes (40 KiB of the CU's 160 KiB: three blocks per CU)
constexpr int FD_BLOCK = 512;
constexpr uint32_t FD_SLOTS = 2048;
constexpr int FD_PROBES = 16;
constexpr int FD_BLOCKS_PER_CU = 3;
constexpr uint64_t FD_LAUNCH_MAX = 1ULL << 30;        // slots of one launch: a block's 32-bit `distinct` counters cannot wrap

struct CovLds {
  uint64_t q_key[CV_W][128];
  uint32_t q_ord[CV_W][128];
};

struct CovArgs {
  ScanParams P;
  TableView T;
  const uint8_t *bases;
  uint64_t total_bases;
  const uint64_t *chunk_start;
  const uint32_t *chunk_len;
  const uint32_t *chunk_src;       // source ordinal | CV_PRIME
  uint64_t nchunks;
  unsigned long long *map_keys, *map_counts;
  uint64_t map_mask;
  unsigned long long *kmers, *supermers;   // [sources], by ordinal
  unsigned long long *counters;    // [1] pairs in the pair map, [2] rows of the (source, depth) map
  int32_t *status;                 // bit 1: a map is full; bit 2: a pair names a cell outside the table
};

__global__ void __launch_bounds__(CV_W * 64) coverage_scan_kernel(CovArgs A) {
  extern __shared__ uint64_t ring[];  // [w][CV_W*64]: the last w keys of every lane
  __shared__ CovLds L;
  const ScanParams &P = A.P;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t stride = CV_W * 64;
  const uint64_t c = (uint64_t)blockIdx.x * stride + tid;
  const bool mine = c < A.nchunks;
  const uint32_t len = mine ? A.chunk_len[c] : 0;
  const uint64_t start = mine ? A.chunk_start[c] : 0;
  const uint32_t src = mine ? A.chunk_src[c] : 0;
  const bool prime = (src & CV_PRIME) != 0;
  const uint32_t ord = src & CV_ORD_MASK;
  const uint32_t maxlen = wave_max32(len);
  ChunkScan S(P.w);
  WaveQueue<uint32_t> Q(L.q_key[wib], L.q_ord[wib], lane);
  uint32_t n_kmers = 0, n_supermers = 0;   // of this lane's chunk: its own windows, matched or not

  auto lookup = [&](uint32_t e, bool active) {   // the queued minimizers, one per lane
    if (!active) return;
    uint64_t cell = 0;
    const bool hit = table_lookup_cell(A.T, L.q_key[wib][e], &cell) != 0;    // a miss leaves the join (:99-100)
    if (hit && !pair_map_add(A.map_keys, A.map_counts, A.map_mask, (cell << CV_ORD_BITS) | L.q_ord[wib][e], 1ULL, A.counters + 1))
      atomicOr(A.status, 2);
  };

  for (uint32_t step = 0; step < maxlen; step++) {
    const int window = S.step(P, ring, stride, tid, A.bases, start, A.total_bases, step, len, prime);
    const bool emit = window == ChunkScan::FRESH;
    if (window != ChunkScan::NO_WINDOW) { n_kmers++; if (emit) n_supermers++; }
    Q.push(emit, S.cur_val, ord, lookup);
  }
  Q.drain(lookup);

  // the chunks' totals: the lanes that share the leader's source hand theirs to it, the rest add their own
  bool have = mine;
  for (int round = 0; round < CV_LEADER_ROUNDS; round++) {
    const bool any = leader_round(have, ord, [&](int leader, uint32_t lo_ord, bool same) {
      const uint32_t ks = wave_sum32(same ? n_kmers : 0u), ss = wave_sum32(same ? n_supermers : 0u);
      if ((int)lane == leader) {
        if (ks) atomicAdd(&A.kmers[lo_ord], (unsigned long long)ks);
        if (ss) atomicAdd(&A.supermers[lo_ord], (unsigned long long)ss);
      }
      have = have && !same;
    });
    if (!any) break;
  }
  if (have) {
    if (n_kmers) atomicAdd(&A.kmers[ord], (unsigned long long)n_kmers);
    if (n_supermers) atomicAdd(&A.supermers[ord], (unsigned long long)n_supermers);
  }
}

struct FoldArgs {
  TableView T;
  uint64_t ncells, tmask;
  unsigned long long *map_keys, *map_counts;   // the pair map, slots [0, n) of this launch
  uint64_t n;
  const int32_t *depths;
  int32_t ndepths;
  unsigned long long *rkeys, *rall, *rdistinct;   // (source ordinal << 32 | depth) -> sumAll, sumDistinct
  uint64_t rmask;
  unsigned long long *counters;
  int32_t *status;
};

__device__ __forceinline__ void fd_global_add(const FoldArgs &A, unsigned long long pair, unsigned long long all, unsigned long long distinct) {
  if (!pair_map_add2(A.rkeys, A.rall, A.rdistinct, A.rmask, pair, all, distinct, A.counters + 2)) atomicOr(A.status, 2);
}

using FoldMap = LdsCountMap<unsigned long long, PAIR_EMPTY, FD_SLOTS, FD_PROBES, false>;

__global__ void __launch_bounds__(FD_BLOCK) coverage_fold_kernel(FoldArgs A) {
  __shared__ FoldMap M;
  __shared__ unsigned long long lall[FD_SLOTS];
  __shared__ unsigned int ldistinct[FD_SLOTS];
  M.clear(threadIdx.x, FD_BLOCK, [&](uint32_t s) { lall[s] = 0; ldistinct[s] = 0; });
  auto block_add = [&](unsigned long long pair, unsigned long long all, unsigned int distinct) {
    M.add(pair, (uint32_t)fmix64(pair), [&](uint32_t h) { atomicAdd(&lall[h], all); atomicAdd(&ldistinct[h], distinct); },
          [&] { fd_global_add(A, pair, all, (unsigned long long)distinct); });
  };
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * FD_BLOCK;
  for (uint64_t base = (uint64_t)blockIdx.x * FD_BLOCK; base < A.n; base += stride) {   // block-uniform: the ballots see whole waves
    const uint64_t i = base + threadIdx.x;
    const unsigned long long key = i < A.n ? A.map_keys[i] : PAIR_EMPTY;
    bool have = key != PAIR_EMPTY;
    unsigned long long count = 0, pair = 0;
    if (have) {
      count = A.map_counts[i];
      A.map_keys[i] = PAIR_EMPTY;    // every slot is read by one lane, and nobody adds during a fold: the map is empty afterwards
      A.map_counts[i] = 0;
      const uint64_t cell = key >> CV_ORD_BITS;
      if (cell >= A.ncells) { atomicOr(A.status, 4); have = false; }
      else {
        const int32_t t = ext_taxon(A.T, (int32_t)(A.T.cells[cell] & A.tmask));
        const int32_t depth = (t >= 0 && t < A.ndepths) ? A.depths[t] : -1;
        pair = ((unsigned long long)(key & CV_ORD_MASK) << 32) | (uint32_t)depth;
      }
    }
    for (int round = 0; round < CV_LEADER_ROUNDS; round++) {
      const bool any = leader_round(have, pair, [&](int leader, unsigned long long lp, bool same) {
        const uint64_t group = __ballot(same);
        const uint64_t all = wave_sum64(same ? count : 0ULL);
        if (lane == leader) block_add(lp, all, (unsigned int)__popcll(group));
        have = have && !same;
      });
      if (!any) break;
    }
    if (have) block_add(pair, count, 1u);
  }
  M.drain(threadIdx.x, FD_BLOCK, [&](unsigned long long pair, uint32_t s) { fd_global_add(A, pair, lall[s], (unsigned long long)ldistinct[s]); });
}

}  // namespace

struct slk_coverage {
  slk_index *ix = nullptr;
  int32_t device = 0;                 // copy: the handle may be destroyed after its index
  DevBuf d_depths;
  int32_t T = 0;
  uint64_t n_depths = 1;              // distinct values of depths[], and -1: the (source, depth) map holds at most sources x n_depths rows
  std::unordered_map<int32_t, uint32_t> ord_of;   // source taxon -> dense ordinal
  std::vector<int32_t> sources;       // ordinal -> source taxon
  DevBuf totals;                      // [2][totals_cap] uint64: k-mers, super-mers by ordinal
  uint64_t totals_cap = 0;
  PairMap map;                        // (cell << 28 | ordinal) -> super-mers, of the open group
  uint64_t max_pairs = 0, max_cap = 0;
  uint64_t n_pairs = 0;               // pairs in the map when it was last settled
  PairMap rows;                       // (ordinal << 32 | depth) -> sumAll
  DevBuf rows_distinct;               //                          -> sumDistinct
  DevBuf counters, status;            // CovArgs.counters (4 x uint64), CovArgs.status
  DevBuf d_bases, d_start, d_len, d_src;
  unsigned fold_blocks = 0;
  bool spent = false;
};

static unsigned long long *cv_kmers(const slk_coverage *c) { return c->totals.as<unsigned long long>(); }
static unsigned long long *cv_supermers(const slk_coverage *c) { return c->totals.as<unsigned long long>() + c->totals_cap; }

// Waits for what was queued on s, reports a full map or a spent budget, and moves the pair map to a larger one while it is more than
// half full -- or, within the budget, has less room than the launch that comes next would like (`want` windows, at most
// CV_LAUNCH_WANT: a launch covers no more windows than the map has free slots, and a map of 2^20 slots would cut a genome into
// launches of a few blocks).
static int32_t cv_settle(slk_coverage *c, hipStream_t s, uint64_t want) {
  unsigned long long n[4] = {0, 0, 0, 0};
  int32_t status = 0;
  HIPCHK(hipMemcpyAsync(n, c->counters.p, sizeof n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&status, c->status.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (status & 4) return fail(SLK_E_HIP, "coverage: a pair names a cell outside the table");
  if (status & 2) return fail(SLK_E_CAPACITY, "coverage: a map is full (%llu slots)", (unsigned long long)c->map.cap);
  c->n_pairs = n[1];
  if (c->n_pairs > c->max_pairs)
    return fail(SLK_E_CAPACITY, "coverage: %llu (minimizer, source) pairs in one group, the budget is %llu (max_pairs; fold between groups of sources)",
                (unsigned long long)c->n_pairs, (unsigned long long)c->max_pairs);
  uint64_t cap = c->map.cap;
  want = std::min(want, CV_LAUNCH_WANT);
  while (cap < c->max_cap && (c->n_pairs * 2 > cap || cap - c->n_pairs < want)) cap *= 2;
  if (cap == c->map.cap) return SLK_OK;
  PairMap old = std::move(c->map);
  c->map = PairMap();
  int32_t rc = c->map.reset(s, cap);
  if (rc) return rc;
  return c->n_pairs ? old.grow_into<false>(s, c->map, nullptr, nullptr, c->status.as<int32_t>()) : SLK_OK;
}

// room for every source's totals and every (source, depth) row
static int32_t cv_ensure_sources(slk_coverage *c, hipStream_t s) {
  const uint64_t ns = c->sources.size();
  if (ns > c->totals_cap) {
    uint64_t cap = std::max<uint64_t>(1024, c->totals_cap);
    while (cap < ns) cap *= 2;
    DevBuf now;
    HIPCHK(now.ensure(cap * 16));
    HIPCHK(hipMemsetAsync(now.p, 0, cap * 16, s));
    if (c->totals_cap) {
      HIPCHK(hipMemcpyAsync(now.p, cv_kmers(c), c->totals_cap * 8, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(now.as<unsigned long long>() + cap, cv_supermers(c), c->totals_cap * 8, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    c->totals = std::move(now);
    c->totals_cap = cap;
  }
  uint64_t cap = std::max<uint64_t>(1024, c->rows.cap);
  while (cap < 2 * ns * c->n_depths) cap *= 2;   // load at most 0.5
  if (cap == c->rows.cap) return SLK_OK;
  PairMap old = std::move(c->rows);
  DevBuf old_distinct = std::move(c->rows_distinct);
  c->rows = PairMap();
  c->rows_distinct = DevBuf();
  int32_t rc = c->rows.reset(s, cap);
  if (rc) return rc;
  HIPCHK(c->rows_distinct.ensure(cap * 8));
  HIPCHK(hipMemsetAsync(c->rows_distinct.p, 0, cap * 8, s));
  return old.cap ? old.grow_into<true>(s, c->rows, &old_distinct, &c->rows_distinct, c->status.as<int32_t>()) : SLK_OK;
}

// the pair map into the (source, depth) rows; synchronises s
static int32_t cv_fold(slk_coverage *c, hipStream_t s) {
  int32_t rc = cv_settle(c, s, 0);
  if (rc == SLK_OK) rc = cv_ensure_sources(c, s);
  if (rc || c->n_pairs == 0) return rc;
  FoldArgs A{};
  A.T = c->ix->view();
  A.ncells = c->ix->nbuckets * CELLS;
  A.tmask = (1ULL << c->ix->taxon_bits) - 1;
  A.depths = c->d_depths.as<int32_t>();
  A.ndepths = c->T;
  A.rkeys = c->rows.k(); A.rall = c->rows.c(); A.rdistinct = c->rows_distinct.as<unsigned long long>(); A.rmask = c->rows.cap - 1;
  A.counters = c->counters.as<unsigned long long>();
  A.status = c->status.as<int32_t>();
  for (uint64_t o = 0; o < c->map.cap; o += FD_LAUNCH_MAX) {
    A.map_keys = c->map.k() + o; A.map_counts = c->map.c() + o; A.n = std::min(FD_LAUNCH_MAX, c->map.cap - o);
    const unsigned blocks = (unsigned)std::min<uint64_t>((A.n + FD_BLOCK - 1) / FD_BLOCK, c->fold_blocks);
    hipLaunchKernelGGL(coverage_fold_kernel, dim3(blocks), dim3(FD_BLOCK), 0, s, A);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(c->counters.as<unsigned long long>() + 1, 0, 8, s));
  int32_t status = 0;
  HIPCHK(hipMemcpyAsync(&status, c->status.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->n_pairs = 0;
  if (status & 4) return fail(SLK_E_HIP, "coverage: a pair names a cell outside the table");
  if (status & 2) return fail(SLK_E_CAPACITY, "coverage: the (source, depth) map is full (%llu slots)", (unsigned long long)c->rows.cap);
  return SLK_OK;
}

static int32_t cv_add(slk_coverage *c, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *source_taxa, uint64_t R) {
  slk_index *ix = c->ix;
  hipStream_t s = st->s;
  const uint32_t k = (uint32_t)ix->sp.k, CW = BUILD_CHUNK_WINDOWS;
  // the sources' ordinals (the arguments were checked: from here on a failure spends the handle)
  for (uint64_t i = 0; i < R; i++) {
    if (source_taxa[i] == 0 || c->ord_of.count(source_taxa[i])) continue;
    c->ord_of.emplace(source_taxa[i], (uint32_t)c->sources.size());
    c->sources.push_back(source_taxa[i]);
  }
  int32_t rc = cv_ensure_sources(c, s);
  if (rc) return rc;
  std::vector<uint64_t> cstart;
  std::vector<uint32_t> clen, csrc;
  for (uint64_t i = 0, j; i < R; i = j) {   // groups of whole sequences of about 1 GiB, cut into chunks of CW windows
    j = group_end(offsets, i, R, CV_GROUP_BYTES);
    const uint64_t g0 = offsets[i], gbytes = offsets[j] - g0;
    cstart.clear(); clen.clear(); csrc.clear();
    uint32_t ord = 0;   // of the sequence whose chunks are coming: looked up at its first chunk, which is not early
    cut_chunks(offsets, i, j, k, CW, true, [&](uint64_t q) { return source_taxa[q] == 0; },
               [&](uint64_t q, uint64_t start, uint32_t len, uint32_t early) {
                 if (!early) ord = c->ord_of[source_taxa[q]];
                 cstart.push_back(start);
                 clen.push_back(len);
                 csrc.push_back(ord | (early ? CV_PRIME : 0u));
               });
    const uint64_t nc = cstart.size();
    if (nc == 0) continue;
    HIPCHK(c->d_bases.ensure(gbytes));
    HIPCHK(c->d_start.ensure(nc * 8));
    HIPCHK(c->d_len.ensure(nc * 4));
    HIPCHK(c->d_src.ensure(nc * 4));
    rc = copy_in(st, c->d_bases.p, bases + g0, gbytes);
    if (!rc) rc = copy_in(st, c->d_start.p, cstart.data(), nc * 8);
    if (!rc) rc = copy_in(st, c->d_len.p, clen.data(), nc * 4);
    if (!rc) rc = copy_in(st, c->d_src.p, csrc.data(), nc * 4);
    if (rc) return rc;
    CovArgs A{};
    A.P = ix->sp;
    A.T = ix->view();
    A.bases = c->d_bases.as<uint8_t>();
    A.total_bases = gbytes;
    A.counters = c->counters.as<unsigned long long>();
    A.status = c->status.as<int32_t>();
    uint64_t left = 0;   // windows of the chunks not launched yet
    for (uint64_t q = 0; q < nc; q++) left += clen[q] - (k - 1) - (csrc[q] >> 31);
    for (uint64_t c0 = 0; c0 < nc;) {
      rc = cv_settle(c, s, left);
      if (rc) return rc;
      // a launch covers no more super-mer candidates (windows) than the map has free slots: it cannot fill the map
      const uint64_t room = c->map.cap - c->n_pairs;
      uint64_t c1 = c0, windows = 0;
      while (c1 < nc) {
        const uint64_t nw = clen[c1] - (k - 1) - (csrc[c1] >> 31);
        if (windows + nw > room) break;
        windows += nw;
        c1++;
      }
      if (c1 == c0)
        return fail(SLK_E_CAPACITY, "coverage: the pair map (%llu slots, %llu pairs) has no room for another chunk within the budget of %llu pairs",
                    (unsigned long long)c->map.cap, (unsigned long long)c->n_pairs, (unsigned long long)c->max_pairs);
      A.chunk_start = c->d_start.as<uint64_t>() + c0;
      A.chunk_len = c->d_len.as<uint32_t>() + c0;
      A.chunk_src = c->d_src.as<uint32_t>() + c0;
      A.nchunks = c1 - c0;
      A.map_keys = c->map.k(); A.map_counts = c->map.c(); A.map_mask = c->map.cap - 1;
      A.kmers = cv_kmers(c); A.supermers = cv_supermers(c);
      const unsigned block = CV_W * 64;
      hipLaunchKernelGGL(coverage_scan_kernel, dim3((unsigned)((A.nchunks + block - 1) / block)), dim3(block), (size_t)block * ix->sp.w * 8, s, A);
      HIPCHK(hipGetLastError());
      left -= windows;
      c0 = c1;
    }
    rc = cv_settle(c, s, 0);   // (the group's bases are free to be overwritten; a failure of the last launch shows in this call)
    if (rc) return rc;
  }
  return SLK_OK;
}

static int32_t cv_enter(slk_coverage *c) {
  return enter_handle(c, "coverage: an earlier call on this handle failed, its counts are incomplete");
}
// SLK_E_CAPACITY and SLK_E_HIP leave the counts incomplete
static int32_t cv_leave(slk_coverage *c, int32_t rc) { return leave_handle(c, rc, rc == SLK_E_CAPACITY || rc == SLK_E_HIP); }

extern "C" {

int32_t slk_coverage_create(slk_index *ix, const int32_t *depths, int32_t T, uint64_t max_pairs, slk_coverage **out) {
  if (!out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (!ix) return fail(SLK_E_INVALID, "null handle");
  if (T < 0 || (T > 0 && !depths)) return fail(SLK_E_INVALID, "depths must hold T >= 0 entries");
  int32_t rc = check_whole_narrow_index(ix, "genome coverage", "table", true);
  if (rc) return rc;
  rc = set_device(ix);
  if (rc) return rc;
  std::unique_ptr<slk_coverage> c(new slk_coverage());   // (released into *out on success only)
  c->ix = ix;
  c->device = ix->device;
  c->T = T;
  std::vector<int32_t> distinct(depths, depths + T);
  distinct.push_back(-1);
  std::sort(distinct.begin(), distinct.end());
  c->n_depths = (uint64_t)(std::unique(distinct.begin(), distinct.end()) - distinct.begin());
  // SLK_COVERAGE_FOLD_BLOCKS: the fold's grid (tests: a few blocks; measurements: occupancy)
  c->fold_blocks = grid_for(ix->device, FD_BLOCKS_PER_CU, "SLK_COVERAGE_FOLD_BLOCKS");
  if (max_pairs == 0) {
    // half of the memory free now, at 16 bytes per slot and load 0.5 (a choice, not a measurement): the largest power of two within it
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t slots = std::max<uint64_t>((uint64_t)free_b / 2 / 16, 1024);
    c->max_cap = 1024;
    while (c->max_cap * 2 <= slots) c->max_cap *= 2;
    c->max_pairs = c->max_cap / 2;
  } else {
    c->max_pairs = max_pairs;
    c->max_cap = 1024;
    while (c->max_cap / 2 < max_pairs && c->max_cap < (1ULL << 40)) c->max_cap *= 2;
  }
  hipError_t e = c->counters.ensure(32);
  if (e == hipSuccess) e = c->status.ensure(8);
  if (e == hipSuccess) e = c->d_depths.ensure((size_t)std::max(T, 1) * 4);
  if (e == hipSuccess) e = hipMemset(c->counters.p, 0, 32);
  if (e == hipSuccess) e = hipMemset(c->status.p, 0, 8);
  if (e == hipSuccess && T) e = hipMemcpy(c->d_depths.p, depths, (size_t)T * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(SLK_E_HIP, "coverage: %s", hipGetErrorString(e)); }
  // 2^20 pairs (16 MiB) to start with; the map grows between launches (cv_settle)
  const int map_log2 = (int)std::min(40L, std::max(10L, env_long("SLK_COVERAGE_MAP_LOG2", 20)));
  rc = c->map.reset(nullptr, std::min(1ULL << map_log2, (unsigned long long)c->max_cap));
  if (rc == SLK_OK) rc = cv_ensure_sources(c.get(), nullptr);
  if (rc == SLK_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SLK_E_HIP, "coverage: map setup failed");
  if (rc) return rc;
  *out = c.release();
  return SLK_OK;
}

uint64_t slk_coverage_budget(const slk_coverage *c) { return c ? c->max_pairs : 0; }

int32_t slk_coverage_add(slk_coverage *c, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *source_taxa,
                         uint64_t R) {
  int32_t rc = cv_enter(c);
  if (rc) return rc;
  rc = check_ready(c->ix, st, false);
  if (rc) return rc;
  if (R && (!offsets || !source_taxa)) return fail(SLK_E_INVALID, "null argument");
  if (R && offsets[R] > offsets[0] && !bases) return fail(SLK_E_INVALID, "null argument");
  uint64_t fresh = 0;
  for (uint64_t i = 0; i < R; i++) {
    if (offsets[i + 1] < offsets[i]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)i);
    if (source_taxa[i] != 0 && !c->ord_of.count(source_taxa[i])) fresh++;   // (an upper bound: a new source may repeat)
  }
  // (2^28 - 1, not 2^28: the last ordinal with the last cell of a table of 2^36 cells would be the map's mark of a free slot)
  if (c->sources.size() + fresh > CV_ORD_MASK) {
    std::unordered_map<int32_t, int> seen;
    for (uint64_t i = 0; i < R; i++) if (source_taxa[i] != 0 && !c->ord_of.count(source_taxa[i])) seen[source_taxa[i]] = 1;
    if (c->sources.size() + seen.size() > CV_ORD_MASK) return cv_leave(c, fail(SLK_E_CAPACITY, "coverage: more than 2^28 source taxa"));
  }
  DrainOnExit drain(st);
  return cv_leave(c, cv_add(c, st, bases, offsets, source_taxa, R));
}

int32_t slk_coverage_fold(slk_coverage *c, slk_stream *st) {
  int32_t rc = cv_enter(c);
  if (rc) return rc;
  rc = check_ready(c->ix, st, false);
  if (rc) return rc;
  return cv_leave(c, cv_fold(c, st->s));
}

int32_t slk_coverage_result(slk_coverage *c, uint64_t *n_rows, int32_t *source, int32_t *depth, uint64_t *all, uint64_t *distinct,
                            uint64_t cap) {
  if (!c || !n_rows) return fail(SLK_E_INVALID, "null argument");
  if (cap && (!source || !depth || !all || !distinct)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = cv_enter(c);
  if (rc) return rc;
  std::vector<uint64_t> keys, sums, ones;
  auto read = [&]() -> int32_t {
    HIPCHK(hipDeviceSynchronize());   // whatever stream the adds ran on
    int32_t r = cv_fold(c, nullptr);  // what is pending
    if (r) return r;
    const uint64_t slots = c->rows.cap;
    std::vector<uint64_t> hd(slots);
    HIPCHK(hipMemcpy(hd.data(), c->rows_distinct.p, slots * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> hk(slots), ha(slots);
    HIPCHK(hipMemcpy(hk.data(), c->rows.keys.p, slots * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ha.data(), c->rows.counts.p, slots * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < slots; i++)
      if (hk[i] != PAIR_EMPTY) { keys.push_back(hk[i]); sums.push_back(ha[i]); ones.push_back(hd[i]); }
    return SLK_OK;
  };
  rc = read();
  if (rc) return cv_leave(c, rc);
  auto source_of = [&](size_t i) { return c->sources[(size_t)(keys[i] >> 32)]; };
  auto depth_of = [&](size_t i) { return (int32_t)(uint32_t)keys[i]; };
  std::vector<size_t> order(keys.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return source_of(a) != source_of(b) ? source_of(a) < source_of(b) : depth_of(a) < depth_of(b);
  });
  *n_rows = order.size();
  for (size_t i = 0; i < order.size() && i < cap; i++) {
    source[i] = source_of(order[i]);
    depth[i] = depth_of(order[i]);
    all[i] = sums[order[i]];
    distinct[i] = ones[order[i]];
  }
  if (cap && cap < order.size()) return fail(SLK_E_CAPACITY, "%llu rows, capacity %llu", (unsigned long long)order.size(), (unsigned long long)cap);
  return SLK_OK;
}

int32_t slk_coverage_totals(slk_coverage *c, uint64_t *n_sources, int32_t *source, uint64_t *kmers, uint64_t *supermers, uint64_t cap) {
  if (!c || !n_sources) return fail(SLK_E_INVALID, "null argument");
  if (cap && (!source || !kmers || !supermers)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = cv_enter(c);
  if (rc) return rc;
  const size_t ns = c->sources.size();
  std::vector<uint64_t> hk(ns), hs(ns);
  auto read = [&]() -> int32_t {
    HIPCHK(hipDeviceSynchronize());
    if (ns) {
      HIPCHK(hipMemcpy(hk.data(), cv_kmers(c), ns * 8, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hs.data(), cv_supermers(c), ns * 8, hipMemcpyDeviceToHost));
    }
    return SLK_OK;
  };
  rc = read();
  if (rc) return cv_leave(c, rc);
  std::vector<size_t> order(ns);
  for (size_t i = 0; i < ns; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return c->sources[a] < c->sources[b]; });
  *n_sources = ns;
  for (size_t i = 0; i < ns && i < cap; i++) {
    source[i] = c->sources[order[i]];
    kmers[i] = hk[order[i]];
    supermers[i] = hs[order[i]];
  }
  if (cap && cap < ns) return fail(SLK_E_CAPACITY, "%llu source taxa, capacity %llu", (unsigned long long)ns, (unsigned long long)cap);
  return SLK_OK;
}

void slk_coverage_destroy(slk_coverage *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

}  // extern "C"
