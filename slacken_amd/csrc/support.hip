// support.hip -- a sample's minimizers counted per taxon against a resident index: the arithmetic of Dynamic.minimizersInSubjects
// (S/slacken/Dynamic.scala:95-117: -C's count(minimizer) and -D's count_distinct(minimizer) per taxon) and Dynamic.multiStatsPerTaxon
// (:152-180: totalKmerCount, distinctMinimizerCount, totalMinimizerCount of the support reports).  The reference joins every SEQUENCE
// super-mer of every read with the records, keeps the hits whose taxon has depth(taxon) >= rank.depth and groups them by taxon.  Here:
//   scan    support_scan_kernel, the lane-per-chunk scan of chunkscan.h with exact seams: one lane per chunk of
//           BUILD_CHUNK_WINDOWS windows -- a 150-base read is one chunk, a long read several.  A super-mer is queued when it CLOSES
//           (at the next fresh minimizer -- an invalid base makes the next window fresh -- or at the end of the chunk), so that its
//           queue entry (key, k-mer windows, starts_here) holds its window count.  A super-mer that runs on from the chunk before
//           (the priming window had its minimizer) is queued by the later chunk with starts_here = 0: its windows go to `kmers`, it
//           adds nothing to `minimizers`.  A super-mer split by a seam is so counted once as a minimizer, with all its k-mers.
//   count   the wave looks 64 queued minimizers up at a time (table_lookup_cell: the one random HBM request per super-mer).  A hit
//           whose taxon passes the depth filter (`keep`, one byte per internal taxon id, made at create) adds
//             kmers[taxon] += windows, minimizers[taxon] += starts_here, distinct[taxon] += 1 the first time its CELL is seen.
//           A key names exactly one cell and one taxon, so count_distinct(minimizer) per taxon is the number of distinct cells hit:
//           one bit per table cell in a bitmap owned by the handle, no pair map, no budget, no sort.  The word is read first and
//           atomicOr is issued only where the bit is clear (a deep sample repeats most of its minimizers); the lane whose atomicOr
//           returns the bit clear owns the increment.
// The three sums go through the three levels of wavetools.h, because a sample's hits pile onto a handful of taxa: SP_LEADER_ROUNDS
// rounds in the wave, the lanes under the leader's taxon handing it their three numbers (wave sums); a map taxon -> 3 x uint32 in LDS
// (SP_SLOTS slots, at most SP_PROBES probes); three uint64 arrays indexed by the taxon the cells hold (the dense internal id of a
// finalized index).  A lane owns ONE chunk (the grid is not strided), so all that
// a block can add to its LDS counters are the windows of its own chunks: at most SP_W * 64 chunks of BUILD_CHUNK_WINDOWS windows
// = 2^17 per launch, whatever the launch's size -- no 32-bit LDS counter can wrap (static_assert below).
//
// Budget.  Blocks of SP_W = 4 waves (2 when the window has more than SP_WIDE_WINDOW m-mers).  LDS per block: the queue 6 KiB, the
// map 16 KiB (1024 slots x 16 B), the ring 8 w bytes per lane: 10 KiB at k = 35, m = 31 -- 32 KiB, five blocks = 20 waves per CU of
// the 160 KiB; 32 KiB of ring at w = 16 and 28 KiB at w = 28 with two waves, 54 KiB at most: two blocks per CU at the widest window,
// and no block asks for more dynamic LDS than the 64 KiB a launch gets without raising its limit.
// VGPRs: the scan's state and one 64-byte bucket per lane during the probe: the compiler reports 79 per lane and no scratch, which
// allows six waves per SIMD -- one more than the five (20 waves per CU) that the LDS admits at k = 35, m = 31 (coverage_scan_kernel has 75
// registers and 22 KiB less LDS).  The kernel waits for the random table requests; nothing here was tuned against a measurement.
#include "chunkcut.h"
#include "chunkscan.h"
#include "hostside.h"

namespace {

constexpr int SP_W = 4;                               // waves per block
constexpr int SP_W_WIDE = 2;                          // ... when the ring is wide
constexpr int SP_WIDE_WINDOW = 16;
constexpr uint32_t SP_SLOTS = 1024;
constexpr int SP_PROBES = 8;
constexpr int SP_LEADER_ROUNDS = 2;
constexpr uint32_t SP_FLAG = 1u << 31;                // chunk_len: the chunk starts one base early; queue meta: the super-mer starts here
constexpr uint64_t SP_GROUP_BYTES = 1ULL << 30;       // bases of a host call on the device at a time
static_assert((uint64_t)SP_W * 64 * BUILD_CHUNK_WINDOWS < (1ULL << 31), "a block's windows fit its 32-bit LDS counters and the queue's meta word");

enum { SP_ROWS = 0, SP_SUPERMERS = 1, SP_MATCHED = 2, SP_KEPT = 3, SP_CURSOR = 4, SP_STATUS = 5, SP_WORDS = 8 };   // slk_support::small

struct SupLds {
  uint64_t q_key[SP_W][128];
  uint32_t q_meta[SP_W][128];       // windows | SP_FLAG
  LdsCountMap<unsigned int, 0u, SP_SLOTS, SP_PROBES, true> map;   // by taxon; 0: free (no record has taxon 0)
  uint32_t kmers[SP_SLOTS], minimizers[SP_SLOTS], distinct[SP_SLOTS];
};

struct SupArgs {
  ScanParams P;
  TableView T;
  const uint8_t *bases;
  uint64_t total_bases;
  const uint64_t *chunk_start;
  const uint32_t *chunk_len;        // bases | SP_FLAG
  uint64_t nchunks;
  const uint8_t *keep;              // [domain] by the taxon the cells hold: depth >= min_depth
  uint64_t domain;
  uint32_t *bitmap;                 // one bit per cell, or nullptr (no distinct counts)
  unsigned long long *kmers, *minimizers, *distinct;   // [domain]
  unsigned long long *small;        // SP_ROWS .. SP_KEPT
  int32_t *status;                  // bit 2: a cell's taxon lies outside the arrays
};

__device__ __forceinline__ void sp_global_add(const SupArgs &A, uint32_t taxon, uint32_t k, uint32_t m, uint32_t d) {
  if (atomicAdd(&A.kmers[taxon], (unsigned long long)k) == 0) atomicAdd(A.small + SP_ROWS, 1ULL);   // (k > 0 always: 0 is seen once per taxon)
  if (m) atomicAdd(&A.minimizers[taxon], (unsigned long long)m);
  if (d) atomicAdd(&A.distinct[taxon], (unsigned long long)d);
}

__device__ __forceinline__ void sp_block_add(const SupArgs &A, SupLds &L, uint32_t taxon, uint32_t k, uint32_t m, uint32_t d) {
  L.map.add(taxon, (taxon * 0x9E3779B1u) >> 22,
            [&](uint32_t h) {
              atomicAdd(&L.kmers[h], k);
              if (m) atomicAdd(&L.minimizers[h], m);
              if (d) atomicAdd(&L.distinct[h], d);
            },
            [&] { sp_global_add(A, taxon, k, m, d); });
}

// the wave's lanes hand in one counted hit each (taxon 0: none); called by whole waves
__device__ __forceinline__ void sp_wave_add(const SupArgs &A, SupLds &L, uint32_t lane, uint32_t taxon, uint32_t k, uint32_t m, uint32_t d) {
  bool have = taxon != 0;
  for (int round = 0; round < SP_LEADER_ROUNDS; round++) {
    const bool any = leader_round(have, taxon, [&](int leader, uint32_t lt, bool same) {
      const uint32_t ks = wave_sum32(same ? k : 0u), ms = wave_sum32(same ? m : 0u), ds = wave_sum32(same ? d : 0u);
      if ((int)lane == leader) sp_block_add(A, L, lt, ks, ms, ds);
      have = have && !same;
    });
    if (!any) return;
  }
  if (have) sp_block_add(A, L, taxon, k, m, d);
}

__global__ void __launch_bounds__(SP_W * 64) support_scan_kernel(SupArgs A) {
  extern __shared__ uint64_t ring[];  // [w][blockDim.x]: the last w keys of every lane
  __shared__ SupLds L;
  const ScanParams &P = A.P;
  const uint32_t tid = threadIdx.x, lane = tid & 63, stride = blockDim.x;
  const uint32_t wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  L.map.clear(tid, stride, [&](uint32_t s) { L.kmers[s] = 0; L.minimizers[s] = 0; L.distinct[s] = 0; });
  const uint64_t c = (uint64_t)blockIdx.x * stride + tid;
  const bool mine = c < A.nchunks;
  const uint32_t packed = mine ? A.chunk_len[c] : 0;
  const uint32_t len = packed & ~SP_FLAG;
  const bool prime = (packed & SP_FLAG) != 0;
  const uint64_t start = mine ? A.chunk_start[c] : 0;
  const uint32_t maxlen = wave_max32(len);

  ChunkScan S(P.w);
  uint64_t open_key = 0;               // the super-mer that has not closed yet: its minimizer, its windows so far (0: none is open),
  uint32_t open_kmers = 0;             // and whether it started in this chunk
  bool open_starts = false;
  WaveQueue<uint32_t> Q(L.q_key[wib], L.q_meta[wib], lane);
  uint32_t n_supermers = 0, n_matched = 0, n_kept = 0;   // of the entries this lane looked up: those that start a super-mer

  auto count = [&](uint32_t e, bool active) {   // look the queued minimizers up, one per lane, and count them (whole waves)
    uint32_t taxon = 0, k = 0, m = 0, d = 0;
    if (active) {
      const uint32_t meta = L.q_meta[wib][e], starts = meta >> 31;
      uint64_t cell = 0;
      const uint32_t t = (uint32_t)table_lookup_cell(A.T, L.q_key[wib][e], &cell);   // a miss (NONE) is never counted
      n_supermers += starts;
      if (t != 0) {
        n_matched += starts;
        if (t >= A.domain) atomicOr(A.status, 4);
        else if (A.keep[t]) {
          taxon = t; k = meta & ~SP_FLAG; m = starts;
          n_kept += starts;
          if (A.bitmap != nullptr) {   // (cell < nbuckets * CELLS: the bitmap's size)
            const uint32_t bit = 1u << (cell & 31);
            uint32_t *word = A.bitmap + (cell >> 5);
            if ((__atomic_load_n(word, __ATOMIC_RELAXED) & bit) == 0 && (atomicOr(word, bit) & bit) == 0) d = 1;
          }
        }
      }
    }
    sp_wave_add(A, L, lane, taxon, k, m, d);
  };

  for (uint32_t step = 0; step < maxlen; step++) {
    const int window = S.step(P, ring, stride, tid, A.bases, start, A.total_bases, step, len, prime);
    bool emit = false;
    uint64_t key = 0;
    uint32_t meta = 0;
    if (window == ChunkScan::FRESH) {          // the open super-mer closes, this window opens the next
      emit = open_kmers != 0;
      key = open_key;
      meta = open_kmers | (open_starts ? SP_FLAG : 0u);
      open_key = S.cur_val; open_kmers = 1; open_starts = true;
    } else if (window == ChunkScan::SAME) {
      if (open_kmers == 0) { open_key = S.cur_val; open_starts = false; }   // (it runs on from the chunk before: the priming window had it)
      open_kmers++;
    }
    Q.push(emit, key, meta, count);
  }
  Q.push(open_kmers != 0, open_key, open_kmers | (open_starts ? SP_FLAG : 0u), count);   // the end of the chunk closes what is open
  Q.drain(count);

  const uint32_t ws = wave_sum32(n_supermers), wm = wave_sum32(n_matched), wk = wave_sum32(n_kept);
  if (lane == 0) {
    if (ws) atomicAdd(A.small + SP_SUPERMERS, (unsigned long long)ws);
    if (wm) atomicAdd(A.small + SP_MATCHED, (unsigned long long)wm);
    if (wk) atomicAdd(A.small + SP_KEPT, (unsigned long long)wk);
  }
  L.map.drain(tid, stride, [&](uint32_t taxon, uint32_t s) { sp_global_add(A, taxon, L.kmers[s], L.minimizers[s], L.distinct[s]); });
}

// keep[t] = the taxon that the cells hold as t has depth >= min_depth in the caller's depths (an id outside [0, n): depth -1)
__global__ void __launch_bounds__(256) support_keep_kernel(TableView T, const int32_t *__restrict__ depths, int32_t n, int32_t min_depth,
                                                           uint8_t *__restrict__ keep, uint64_t domain) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < domain; t += stride) {
    const int32_t e = ext_taxon(T, (int32_t)t);
    const int32_t depth = (e >= 0 && e < n) ? depths[e] : -1;
    keep[t] = (t != 0 && depth >= min_depth) ? 1 : 0;
  }
}

// The rows with k-mers (every counted hit has at least one) as (taxon in the caller's ids, kmers, minimizers, distinct), in any
// order: their number is known (SP_ROWS) and the host sorts them.  One atomic per wave (wavetools.h: wave_alloc_slots).
__global__ void __launch_bounds__(256) support_rows_kernel(TableView T, const unsigned long long *__restrict__ kmers,
                                                           const unsigned long long *__restrict__ minimizers,
                                                           const unsigned long long *__restrict__ distinct, uint64_t domain,
                                                           int32_t *__restrict__ taxa, unsigned long long *__restrict__ out, uint64_t capacity,
                                                           unsigned long long *__restrict__ cursor) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < domain; base += stride) {   // wave-uniform trip count
    const uint64_t t = base + threadIdx.x;
    const unsigned long long k = t < domain ? kmers[t] : 0;
    const bool has = k != 0;
    const unsigned long long slot = wave_alloc_slots(has, cursor);
    if (has && slot < capacity) {
      taxa[slot] = ext_taxon(T, (int32_t)t);
      out[slot] = k;
      out[capacity + slot] = minimizers[t];
      out[2 * capacity + slot] = distinct[t];
    }
  }
}

}  // namespace

struct slk_support {
  slk_index *ix = nullptr;
  int32_t device = 0;                 // copy: the handle may be destroyed after its index
  bool want_distinct = false;
  uint64_t domain = 0;                // ids the cells can hold: the arrays' length
  DevBuf keep;                        // [domain] uint8
  DevBuf sums;                        // [3][domain] uint64: kmers, minimizers, distinct
  DevBuf bitmap;                      // one bit per cell (want_distinct)
  DevBuf small;                       // SP_WORDS uint64
  DevBuf d_bases, d_start, d_len, d_taxa, d_rows;
  uint64_t sequences = 0;
  bool spent = false;
  unsigned long long *sum(int i) const { return sums.as<unsigned long long>() + (uint64_t)i * domain; }
};

static int32_t sp_enter(slk_support *s) {
  return enter_handle(s, "support: an earlier call on this handle failed, its counts are incomplete");
}
static int32_t sp_leave(slk_support *s, int32_t rc) { return leave_handle(s, rc, rc == SLK_E_HIP); }   // SLK_E_HIP leaves the counts incomplete

static int32_t sp_add(slk_support *sp, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, uint64_t R) {
  slk_index *ix = sp->ix;
  hipStream_t s = st->s;
  const uint32_t k = (uint32_t)ix->sp.k, CW = BUILD_CHUNK_WINDOWS;
  std::vector<uint64_t> cstart;
  std::vector<uint32_t> clen;
  for (uint64_t i = 0, j; i < R; i = j) {   // groups of whole sequences of about 1 GiB, cut into chunks of CW windows
    j = group_end(offsets, i, R, SP_GROUP_BYTES);
    const uint64_t g0 = offsets[i], gbytes = offsets[j] - g0;
    cstart.clear(); clen.clear();
    cstart.reserve((j - i) + gbytes / CW); clen.reserve((j - i) + gbytes / CW);   // (a chunk per sequence and one more per CW windows at most)
    cut_chunks(offsets, i, j, k, CW, true, [](uint64_t) { return false; }, [&](uint64_t, uint64_t start, uint32_t len, uint32_t early) {
      cstart.push_back(start);
      clen.push_back(len | (early ? SP_FLAG : 0u));
    });
    const uint64_t nc = cstart.size();
    if (nc == 0) continue;
    HIPCHK(sp->d_bases.ensure(gbytes));
    HIPCHK(sp->d_start.ensure(nc * 8));
    HIPCHK(sp->d_len.ensure(nc * 4));
    int32_t rc = copy_in(st, sp->d_bases.p, bases + g0, gbytes);
    if (!rc) rc = copy_in(st, sp->d_start.p, cstart.data(), nc * 8);
    if (!rc) rc = copy_in(st, sp->d_len.p, clen.data(), nc * 4);
    if (rc) return rc;
    SupArgs A{};
    A.P = ix->sp;
    A.T = ix->view();
    A.bases = sp->d_bases.as<uint8_t>();
    A.total_bases = gbytes;
    A.chunk_start = sp->d_start.as<uint64_t>();
    A.chunk_len = sp->d_len.as<uint32_t>();
    A.nchunks = nc;
    A.keep = sp->keep.as<uint8_t>();
    A.domain = sp->domain;
    A.bitmap = sp->want_distinct ? sp->bitmap.as<uint32_t>() : nullptr;
    A.kmers = sp->sum(0); A.minimizers = sp->sum(1); A.distinct = sp->sum(2);
    A.small = sp->small.as<unsigned long long>();
    A.status = (int32_t *)(sp->small.as<unsigned long long>() + SP_STATUS);
    const unsigned block = (ix->sp.w > SP_WIDE_WINDOW ? SP_W_WIDE : SP_W) * 64;
    hipLaunchKernelGGL(support_scan_kernel, dim3((unsigned)((nc + block - 1) / block)), dim3(block), (size_t)block * ix->sp.w * 8, s, A);
    HIPCHK(hipGetLastError());
    unsigned long long status = 0;   // (the group's buffers are free to be overwritten; a failure of the launch shows in this call)
    HIPCHK(hipMemcpyAsync(&status, sp->small.as<unsigned long long>() + SP_STATUS, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (status & 4) return fail(SLK_E_HIP, "support: a cell holds a taxon beyond the index's %llu internal ids", (unsigned long long)sp->domain);
  }
  sp->sequences += R;
  return SLK_OK;
}

extern "C" {

int32_t slk_support_create(slk_index *ix, const int32_t *depths, int32_t T, int32_t min_depth, int32_t want_distinct, slk_support **out) {
  if (!out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (!ix) return fail(SLK_E_INVALID, "null handle");
  if (T < 0 || (T > 0 && !depths)) return fail(SLK_E_INVALID, "depths must hold T >= 0 entries");
  if (min_depth < 0) return fail(SLK_E_INVALID, "min_depth must not be negative");
  int32_t rc = check_whole_narrow_index(ix, "sample support", "table", true);
  if (rc) return rc;
  rc = set_device(ix);
  if (rc) return rc;
  std::unique_ptr<slk_support> s(new slk_support());   // (released into *out on success only)
  s->ix = ix;
  s->device = ix->device;
  s->want_distinct = want_distinct != 0;
  // the ids the cells hold: dense ranks 1 .. D, or the caller's ids below 2^taxon_bits
  s->domain = ix->D ? (uint64_t)ix->D + 1 : 1ULL << ix->taxon_bits;
  const uint64_t ncells = ix->nbuckets * CELLS, words = (ncells + 31) / 32;
  DevBuf d_depths;
  hipError_t e = s->small.ensure(SP_WORDS * 8);
  if (e == hipSuccess) e = s->keep.ensure(s->domain);
  if (e == hipSuccess) e = s->sums.ensure(s->domain * 24);
  if (e == hipSuccess && s->want_distinct) e = s->bitmap.ensure(words * 4);
  if (e == hipSuccess) e = d_depths.ensure((size_t)std::max(T, 1) * 4);
  if (e == hipSuccess) e = hipMemset(s->small.p, 0, SP_WORDS * 8);
  if (e == hipSuccess) e = hipMemset(s->sums.p, 0, s->domain * 24);
  if (e == hipSuccess && s->want_distinct) e = hipMemset(s->bitmap.p, 0, words * 4);
  if (e == hipSuccess && T) e = hipMemcpy(d_depths.p, depths, (size_t)T * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(SLK_E_HIP, "support: %s", hipGetErrorString(e)); }
  hipLaunchKernelGGL(support_keep_kernel, dim3((unsigned)std::min<uint64_t>((s->domain + 255) / 256, 4096)), dim3(256), 0, nullptr, ix->view(),
                     d_depths.as<int32_t>(), T, min_depth, s->keep.as<uint8_t>(), s->domain);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));   // (d_depths dies here)
  *out = s.release();
  return SLK_OK;
}

int32_t slk_support_add(slk_support *s, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, uint64_t R) {
  int32_t rc = sp_enter(s);
  if (rc) return rc;
  rc = check_ready(s->ix, st, false);
  if (rc) return rc;
  if (R && !offsets) return fail(SLK_E_INVALID, "null argument");
  if (R && offsets[R] > offsets[0] && !bases) return fail(SLK_E_INVALID, "null argument");
  for (uint64_t i = 0; i < R; i++)
    if (offsets[i + 1] < offsets[i]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)i);
  DrainOnExit drain(st);
  return sp_leave(s, sp_add(s, st, bases, offsets, R));
}

int32_t slk_support_result(slk_support *s, uint64_t *n_taxa, int32_t *taxa, uint64_t *kmers, uint64_t *minimizers, uint64_t *distinct,
                           uint64_t cap) {
  if (!s || !n_taxa) return fail(SLK_E_INVALID, "null argument");
  if (cap && (!taxa || !kmers || !minimizers || !distinct)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = sp_enter(s);
  if (rc) return rc;
  struct Row { int32_t taxon; uint64_t k, m, d; };
  std::vector<Row> rows;
  auto read = [&]() -> int32_t {
    HIPCHK(hipDeviceSynchronize());   // whatever stream the adds ran on
    unsigned long long n = 0;
    HIPCHK(hipMemcpy(&n, s->small.as<unsigned long long>() + SP_ROWS, 8, hipMemcpyDeviceToHost));
    rows.resize(n);
    if (n == 0 || cap == 0) return SLK_OK;
    HIPCHK(s->d_taxa.ensure(n * 4));
    HIPCHK(s->d_rows.ensure(n * 24));
    HIPCHK(hipMemset(s->small.as<unsigned long long>() + SP_CURSOR, 0, 8));
    hipLaunchKernelGGL(support_rows_kernel, dim3((unsigned)std::min<uint64_t>((s->domain + 255) / 256, 4096)), dim3(256), 0, nullptr, s->ix->view(),
                       s->sum(0), s->sum(1), s->sum(2), s->domain, s->d_taxa.as<int32_t>(), s->d_rows.as<unsigned long long>(), (uint64_t)n,
                       s->small.as<unsigned long long>() + SP_CURSOR);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> ht(n);
    std::vector<unsigned long long> hr(3 * n);
    HIPCHK(hipMemcpy(ht.data(), s->d_taxa.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hr.data(), s->d_rows.p, n * 24, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; i++) rows[i] = {ht[i], hr[i], hr[n + i], hr[2 * n + i]};
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.taxon < b.taxon; });
    return SLK_OK;
  };
  rc = read();
  if (rc) return sp_leave(s, rc);
  *n_taxa = rows.size();
  for (size_t i = 0; i < rows.size() && i < cap; i++) {
    taxa[i] = rows[i].taxon;
    kmers[i] = rows[i].k;
    minimizers[i] = rows[i].m;
    distinct[i] = rows[i].d;
  }
  if (cap && cap < rows.size()) return fail(SLK_E_CAPACITY, "%llu taxa, capacity %llu", (unsigned long long)rows.size(), (unsigned long long)cap);
  return SLK_OK;
}

int32_t slk_support_totals(slk_support *s, uint64_t *sequences, uint64_t *supermers, uint64_t *matched, uint64_t *kept) {
  if (!s) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = sp_enter(s);
  if (rc) return rc;
  unsigned long long h[SP_WORDS] = {};
  auto read = [&]() -> int32_t {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h, s->small.p, sizeof h, hipMemcpyDeviceToHost));
    return SLK_OK;
  };
  rc = read();
  if (rc) return sp_leave(s, rc);
  if (sequences) *sequences = s->sequences;
  if (supermers) *supermers = h[SP_SUPERMERS];
  if (matched) *matched = h[SP_MATCHED];
  if (kept) *kept = h[SP_KEPT];
  return SLK_OK;
}

void slk_support_destroy(slk_support *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}

}  // extern "C"
