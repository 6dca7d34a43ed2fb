// migration.hip -- minimizer migration between two libraries: MinimizerMigration.taxaDistances (S/slacken/analysis/
// MinimizerMigration.scala:38-66).  The reference joins the records of a SUBJECT library with those of a REFERENCE library on the
// minimizer (joinWith, :47) and maps every matched row to (t1, t2, steps).  Here the reference's table is resident in HBM, the
// subject's records stream through one kernel that looks each key up (the only random access per record) and counts the (t1, t2)
// pairs; steps is a function of the pair, computed per distinct pair on the host (slk_migration_result).
//
// The count has the three levels of wavetools.h, so that the few hot pairs of a real library (t1 == t2 for a few thousand species)
// do not serialise on a handful of HBM addresses: MG_LEADER_ROUNDS rounds in the wave, the lanes under the leader's pair counted
// with a ballot; a map pair -> uint32 in LDS (MG_SLOTS slots, at most MG_PROBES probes); the device-wide map (pairmap.h), one
// 64-bit atomic per occupied LDS slot at the end of the block.  A block's LDS counters are 32-bit; a launch covers at most MG_LAUNCH_MAX = 2^30 records
// (the host cuts longer calls), so no block can see as many as 2^32 between two flushes.
#include "hostside.h"
#include "pairmap.h"
#include "wavetools.h"

namespace {

// 512 lanes and 4096 slots (48 KiB of the CU's 160 KiB LDS): three blocks, 24 waves per CU to hide the table's latency behind, and
// room for the ~4000 hot pairs of a standard library in every block's map at a load factor under one.
constexpr int MG_BLOCK = 512;
constexpr uint32_t MG_SLOTS = 4096;
constexpr int MG_PROBES = 16;
constexpr int MG_LEADER_ROUNDS = 2;
constexpr int MG_BLOCKS_PER_CU = 3;
constexpr uint64_t MG_LAUNCH_MAX = 1ULL << 30;
constexpr uint64_t MG_HOST_CHUNK = 1ULL << 22;   // records of a host call on the device at a time (48 MiB)

struct MgArgs {
  TableView T;
  const int64_t *keys;
  const int32_t *taxa;
  uint64_t n;
  unsigned long long *map_keys, *map_counts;
  uint64_t map_mask;
  unsigned long long *counters;   // [0] matched, [1] unmatched, [2] distinct pairs in the device-wide map
  int32_t *status;                // bit 1: the device-wide map is full
};

__device__ __forceinline__ void mg_global_add(const MgArgs &A, unsigned long long pair, unsigned long long c) {
  if (!pair_map_add(A.map_keys, A.map_counts, A.map_mask, pair, c, A.counters + 2)) atomicOr(A.status, 2);
}

using MgMap = LdsCountMap<unsigned long long, PAIR_EMPTY, MG_SLOTS, MG_PROBES, false>;

__global__ void __launch_bounds__(MG_BLOCK) migration_kernel(MgArgs A) {
  __shared__ MgMap M;
  __shared__ unsigned int lcounts[MG_SLOTS];
  M.clear(threadIdx.x, MG_BLOCK, [&](uint32_t s) { lcounts[s] = 0; });
  auto block_add = [&](unsigned long long pair, unsigned int c) {
    M.add(pair, (uint32_t)fmix64(pair), [&](uint32_t h) { atomicAdd(&lcounts[h], c); }, [&] { mg_global_add(A, pair, c); });
  };
  const int lane = threadIdx.x & 63;
  uint64_t n_matched = 0, n_unmatched = 0;   // of this wave (every lane keeps the same numbers)
  const uint64_t stride = (uint64_t)gridDim.x * MG_BLOCK;
  for (uint64_t base = (uint64_t)blockIdx.x * MG_BLOCK; base < A.n; base += stride) {   // block-uniform: the ballots see whole waves
    const uint64_t i = base + threadIdx.x;
    const bool in = i < A.n;
    const uint64_t key = in ? (uint64_t)A.keys[i] : 0;
    const int32_t t1 = in ? A.taxa[i] : 0;
    const bool act = in && t1 != 0;                                   // NONE records are skipped, as slk_index_append skips them
    const int32_t t2 = act ? ext_taxon(A.T, table_lookup(A.T, key)) : 0;
    bool have = act && t2 != 0;                                       // a miss leaves the join (:47)
    n_matched += (uint64_t)__popcll(__ballot(have));
    n_unmatched += (uint64_t)__popcll(__ballot(act && !have));
    const unsigned long long pair = ((unsigned long long)(uint32_t)t1 << 32) | (uint32_t)t2;
    for (int round = 0; round < MG_LEADER_ROUNDS; round++) {
      const bool any = leader_round(have, pair, [&](int leader, unsigned long long lp, bool same) {
        const uint64_t group = __ballot(same);
        if (lane == leader) block_add(lp, (unsigned int)__popcll(group));
        have = have && !same;
      });
      if (!any) break;
    }
    if (have) block_add(pair, 1u);
  }
  if (lane == 0) {
    if (n_matched) atomicAdd(A.counters + 0, (unsigned long long)n_matched);
    if (n_unmatched) atomicAdd(A.counters + 1, (unsigned long long)n_unmatched);
  }
  M.drain(threadIdx.x, MG_BLOCK, [&](unsigned long long pair, uint32_t s) { mg_global_add(A, pair, (unsigned long long)lcounts[s]); });
}

}  // namespace

struct slk_migration {
  slk_index *ix = nullptr;
  int32_t device = 0;            // copy: the handle may be destroyed after its index
  std::vector<int32_t> depths;   // Taxonomy.depth of the reference's taxonomy, by id
  bool have_depths = false;
  PairMap map;                   // (t1 << 32 | t2) -> records
  DevBuf counters, status;       // MgArgs.counters (3 x uint64), MgArgs.status
  DevBuf d_keys, d_taxa;         // a chunk of a host call
  int max_log2 = 32;
  unsigned blocks = 0;
  bool spent = false;            // an add failed: the map holds part of it
};

static int32_t mg_check_spent(const slk_migration *m) {
  if (m->spent) return fail(SLK_E_STATE, "migration: an earlier slk_migration_add failed, the counts of this handle are incomplete");
  return SLK_OK;
}

static MgArgs mg_args(const slk_migration *m) {
  MgArgs A{};
  A.T = m->ix->view();
  A.map_keys = m->map.k(); A.map_counts = m->map.c(); A.map_mask = m->map.cap - 1;
  A.counters = m->counters.as<unsigned long long>();
  A.status = m->status.as<int32_t>();
  return A;
}

// Waits for what was queued on s, reports a full map, and moves the map to a larger one when it is more than half full: the adds that
// follow find room.  Only an add that by itself brings more new pairs than the map has free slots can fill it.
static int32_t mg_settle(slk_migration *m, hipStream_t s) {
  unsigned long long c[3] = {0, 0, 0};
  int32_t status = 0;
  HIPCHK(hipMemcpyAsync(c, m->counters.p, sizeof c, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&status, m->status.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (status & 2)
    return fail(SLK_E_CAPACITY, "migration: one call brought more new (t1, t2) pairs than the map had room for (%llu slots; SLK_MIGRATION_MAP_LOG2)",
                (unsigned long long)m->map.cap);
  uint64_t cap = m->map.cap;
  while (c[2] * 2 > cap && cap < (1ULL << m->max_log2)) cap *= 2;
  if (cap == m->map.cap) return SLK_OK;
  PairMap old = std::move(m->map);
  m->map = PairMap();
  const int32_t rc = m->map.reset(s, cap);
  if (rc) return rc;
  return old.grow_into<false>(s, m->map, nullptr, nullptr, m->status.as<int32_t>());   // (old is freed on return)
}

static int32_t mg_launch(slk_migration *m, hipStream_t s, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n) {
  for (uint64_t o = 0; o < n; o += MG_LAUNCH_MAX) {
    MgArgs A = mg_args(m);
    A.keys = d_keys + o; A.taxa = d_taxa + o; A.n = std::min(MG_LAUNCH_MAX, n - o);
    const unsigned blocks = (unsigned)std::min<uint64_t>((A.n + MG_BLOCK - 1) / MG_BLOCK, m->blocks);
    hipLaunchKernelGGL(migration_kernel, dim3(blocks), dim3(MG_BLOCK), 0, s, A);
    HIPCHK(hipGetLastError());
  }
  return SLK_OK;
}

static int32_t mg_enter(slk_migration *m, slk_stream *st, const void *keys, const void *taxa, uint64_t n) {
  if (!m) return fail(SLK_E_INVALID, "null handle");
  int32_t rc = mg_check_spent(m);
  if (rc) return rc;
  rc = check_ready(m->ix, st, false);
  if (rc) return rc;
  if (n && (!keys || !taxa)) return fail(SLK_E_INVALID, "null argument");
  return set_device(m->ix);
}

extern "C" {

int32_t slk_migration_create(slk_index *reference, const int32_t *depths, int32_t T, slk_migration **out) {
  if (!out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (!reference) return fail(SLK_E_INVALID, "null handle");
  if (T < 0 || (T > 0 && !depths)) return fail(SLK_E_INVALID, "depths must hold T >= 0 entries");
  int32_t rc = check_whole_narrow_index(reference, "minimizer migration", "reference table", false);
  if (rc) return rc;
  rc = set_device(reference);
  if (rc) return rc;
  std::unique_ptr<slk_migration> m(new slk_migration());   // (released into *out on success only)
  m->ix = reference;
  m->device = reference->device;
  m->have_depths = depths != nullptr;
  if (depths) m->depths.assign(depths, depths + T);
  // SLK_MIGRATION_BLOCKS: the grid (tests: a few blocks see more pairs than their LDS maps hold; measurements: occupancy)
  m->blocks = grid_for(reference->device, MG_BLOCKS_PER_CU, "SLK_MIGRATION_BLOCKS");
  hipError_t e = m->counters.ensure(24);
  if (e == hipSuccess) e = m->status.ensure(8);
  if (e == hipSuccess) e = hipMemset(m->counters.p, 0, 24);
  if (e == hipSuccess) e = hipMemset(m->status.p, 0, 8);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(SLK_E_HIP, "migration: %s", hipGetErrorString(e)); }
  // 2^20 pairs (16 MiB) to start with: a standard library has a few hundred thousand, and the map grows (mg_settle)
  const int map_log2 = (int)std::min(32L, std::max(10L, env_long("SLK_MIGRATION_MAP_LOG2", 20)));
  rc = m->map.reset(nullptr, 1ULL << map_log2);
  if (rc == SLK_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SLK_E_HIP, "migration: map setup failed");
  if (rc) return rc;
  *out = m.release();
  return SLK_OK;
}

int32_t slk_migration_add_device(slk_migration *m, slk_stream *st, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n) {
  int32_t rc = mg_enter(m, st, d_keys, d_taxa, n);
  if (rc) return rc;
  rc = mg_settle(m, st->s);   // what earlier calls queued: its failure shows here, its new pairs are given room
  if (rc == SLK_OK) rc = mg_launch(m, st->s, d_keys, d_taxa, n);
  if (rc) m->spent = true;
  return rc;
}

int32_t slk_migration_add(slk_migration *m, slk_stream *st, const int64_t *keys, const int32_t *taxa, uint64_t n) {
  int32_t rc = mg_enter(m, st, keys, taxa, n);
  if (rc) return rc;
  DrainOnExit drain(st);
  auto run = [&]() -> int32_t {
    const uint64_t room = std::min<uint64_t>(std::max<uint64_t>(n, 1), MG_HOST_CHUNK);
    HIPCHK(m->d_keys.ensure(room * 8));
    HIPCHK(m->d_taxa.ensure(room * 4));
    int32_t r = mg_settle(m, st->s);
    for (uint64_t o = 0; r == SLK_OK && o < n; o += MG_HOST_CHUNK) {
      const uint64_t c = std::min(MG_HOST_CHUNK, n - o);
      r = copy_in(st, m->d_keys.p, keys + o, c * 8);
      if (r == SLK_OK) r = copy_in(st, m->d_taxa.p, taxa + o, c * 4);
      if (r == SLK_OK) r = mg_launch(m, st->s, m->d_keys.as<int64_t>(), m->d_taxa.as<int32_t>(), c);
      if (r == SLK_OK) r = mg_settle(m, st->s);   // chunk by chunk: the pairs of a long call are given room as they come
    }
    return r;
  };
  rc = run();
  if (rc) m->spent = true;
  return rc;
}

int32_t slk_migration_result(slk_migration *m, uint64_t *n_triples, int32_t *t1, int32_t *t2, int32_t *steps, uint64_t *count,
                             uint64_t cap, uint64_t *matched, uint64_t *unmatched) {
  if (!m || !n_triples) return fail(SLK_E_INVALID, "null argument");
  if (cap && (!t1 || !t2 || !steps || !count)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = mg_check_spent(m);
  if (rc) return rc;
  rc = set_device(m->ix);
  if (rc) return rc;
  auto read = [&](std::vector<uint64_t> &keys, std::vector<uint64_t> &counts, unsigned long long *c) -> int32_t {
    HIPCHK(hipDeviceSynchronize());   // whatever stream the adds were queued on
    int32_t status = 0;
    HIPCHK(hipMemcpy(&status, m->status.p, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(c, m->counters.p, 24, hipMemcpyDeviceToHost));
    if (status & 2)
      return fail(SLK_E_CAPACITY, "migration: one call brought more new (t1, t2) pairs than the map had room for (%llu slots; SLK_MIGRATION_MAP_LOG2)",
                  (unsigned long long)m->map.cap);
    return m->map.read(nullptr, keys, counts);
  };
  std::vector<uint64_t> keys, counts;
  unsigned long long c[3] = {0, 0, 0};
  rc = read(keys, counts, c);
  if (rc) { m->spent = true; return rc; }
  std::vector<size_t> order(keys.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  auto t1_of = [&](size_t i) { return (int32_t)(uint32_t)(keys[i] >> 32); };
  auto t2_of = [&](size_t i) { return (int32_t)(uint32_t)keys[i]; };
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return t1_of(a) != t1_of(b) ? t1_of(a) < t1_of(b) : t2_of(a) < t2_of(b); });
  auto depth = [&](int32_t t) { return (t >= 0 && (size_t)t < m->depths.size()) ? m->depths[t] : -1; };
  *n_triples = order.size();
  if (matched) *matched = c[0];
  if (unmatched) *unmatched = c[1];
  for (size_t i = 0; i < order.size() && i < cap; i++) {
    const int32_t a = t1_of(order[i]), b = t2_of(order[i]);
    t1[i] = a;
    t2[i] = b;
    count[i] = counts[order[i]];
    // MinimizerMigration.scala:51-64
    steps[i] = !m->have_depths ? 0 : depth(a) == -1 ? -100 : depth(b) == -1 ? -200 : depth(a) - depth(b);
  }
  if (cap && cap < order.size()) return fail(SLK_E_CAPACITY, "%llu triples, capacity %llu", (unsigned long long)order.size(), (unsigned long long)cap);
  return SLK_OK;
}

void slk_migration_destroy(slk_migration *m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

}  // extern "C"
