// hostside.h -- what the host-side translation units of the library share (index.hip / stream.hip / classify.hip / hostcalls.hip /
// capi.hip: the C ABI of one index / one stream; shardset.hip: the table-sharded set of indices): the handles' structures, error reporting, the staged copies
// between caller memory and HBM.  Internal: not part of the C ABI.
#pragma once
#include "../../include/slacken_amd.h"
#include "engine.h"
#include "laneplan.h"   // PlanSwitches: what a classify call reads of the environment, once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace slk;

inline thread_local std::string g_err;

inline int32_t fail(int32_t code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// A failed HIP call leaves its code behind as the thread's "last error"; it is read back (cleared) here so that it cannot
// be mistaken for the result of a later kernel launch that is checked with hipGetLastError().
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      (void)hipGetLastError();                                                                         \
      return fail(SLK_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    }                                                                                                  \
  } while (0)


// ---- owners -------------------------------------------------------------------------------------------------------------------
// Whatever the host side allocates on or for a device is held by one of these: released when the owner dies, movable, not copyable.
// Two rules follow from the destructors.  No owner has static storage duration (the HIP runtime is gone by the time statics die),
// and whoever deletes a handle selects its device first.
template <class H, hipError_t (*Free)(H)>
class Owner {
  H h_{};

 public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h_(o.h_) { o.h_ = H{}; }
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) { reset(o.h_); o.h_ = H{}; }
    return *this;
  }
  ~Owner() { reset(); }
  H get() const { return h_; }
  operator H() const { return h_; }
  void reset(H h = H{}) { if (h_) (void)Free(h_); h_ = h; }
  H *put() { reset(); return &h_; }   // for the call that makes one: hipStreamCreate(s.put()), hipMalloc((void **)p.put(), n)
};
template <class T> hipError_t free_device(T *p) { return hipFree((void *)p); }
template <class T> hipError_t free_pinned(T *p) { return hipHostFree((void *)p); }
template <class T> using DevPtr = Owner<T *, free_device<T>>;
template <class T> using PinnedPtr = Owner<T *, free_pinned<T>>;
using Stream = Owner<hipStream_t, hipStreamDestroy>;
using Event = Owner<hipEvent_t, hipEventDestroy>;

struct DevBuf {   // device scratch that grows on demand
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T *as() const { return (T *)p; }
};

// ---- host side of the copies ----------------------------------------------------------------------------------------------
// A few threads that move bytes between the caller's (pageable) memory and the pinned staging buffers: one thread copies
// at 10-12 GB/s, PCIe Gen5 x16 takes ~55.  Started on first use; SLK_COPY_THREADS (default 6, 1 = the calling thread only).
class HostPool {
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  const std::function<void(size_t)> *fn_ = nullptr;
  size_t next_ = 0, n_ = 0, active_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
  std::mutex call_mu_;  // one parallel_for at a time (others wait: the pool is for memory-bound copies)

  void worker() {
    uint64_t seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || (gen_ != seen && fn_); });
      if (stop_) return;
      seen = gen_;
      while (fn_ && next_ < n_) {
        size_t i = next_++;
        active_++;
        const std::function<void(size_t)> *f = fn_;
        lk.unlock();
        (*f)(i);
        lk.lock();
        active_--;
      }
      done_.notify_all();
    }
  }

 public:
  explicit HostPool(size_t n) { for (size_t i = 0; i + 1 < n; i++) th_.emplace_back([this] { worker(); }); }
  ~HostPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto &t : th_) t.join();
  }
  size_t size() const { return th_.size() + 1; }
  void parallel_for(size_t n, const std::function<void(size_t)> &f) {  // f(0) .. f(n-1), the caller takes part
    if (n == 0) return;
    if (th_.empty() || n == 1) { for (size_t i = 0; i < n; i++) f(i); return; }
    std::lock_guard<std::mutex> call(call_mu_);
    std::unique_lock<std::mutex> lk(mu_);
    fn_ = &f; next_ = 0; n_ = n; gen_++;
    cv_.notify_all();
    while (next_ < n_) {
      size_t i = next_++;
      active_++;
      lk.unlock();
      f(i);
      lk.lock();
      active_--;
    }
    done_.wait(lk, [&] { return active_ == 0; });
    fn_ = nullptr;
  }
};
inline HostPool &host_pool() {
  static HostPool *pool = [] {
    long n = env_long("SLK_COPY_THREADS", 6);
    unsigned hc = std::thread::hardware_concurrency();
    if (hc && n > (long)hc) n = hc;
    return new HostPool((size_t)std::max<long>(1, n));  // (never destroyed: worker threads must not be joined at process exit)
  }();
  return *pool;
}
inline void parallel_memcpy(void *dst, const void *src, size_t n) {
  const size_t SLICE = (size_t)1 << 20;
  if (n <= 2 * SLICE) { memcpy(dst, src, n); return; }
  const size_t parts = std::min(host_pool().size(), (n + SLICE - 1) / SLICE);
  const size_t per = ((n + parts - 1) / parts + 63) & ~(size_t)63;
  host_pool().parallel_for(parts, [&](size_t i) {
    const size_t a = i * per, b = std::min(n, a + per);
    if (a < b) memcpy((char *)dst + a, (const char *)src + a, b - a);
  });
}

// Host memory the library has pinned (slk_host_alloc / slk_host_register): copies from and to it are DMA'd directly.
struct PinnedRanges {
  std::mutex mu;
  std::map<uintptr_t, std::pair<size_t, bool>> ranges;  // start -> (bytes, allocated by us)
  void add(void *p, size_t n, bool owned) { std::lock_guard<std::mutex> lk(mu); ranges[(uintptr_t)p] = {n, owned}; }
  bool remove(void *p, bool *owned) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = ranges.find((uintptr_t)p);
    if (it == ranges.end()) return false;
    *owned = it->second.second;
    ranges.erase(it);
    return true;
  }
  bool covers(const void *p, size_t n) {
    std::lock_guard<std::mutex> lk(mu);
    if (ranges.empty()) return false;
    auto it = ranges.upper_bound((uintptr_t)p);
    if (it == ranges.begin()) return false;
    --it;
    return (uintptr_t)p + n <= it->first + it->second.first;
  }
};
inline PinnedRanges &pinned() { static PinnedRanges *r = new PinnedRanges(); return *r; }

// Pinned staging buffers: every copy between PAGEABLE caller memory and HBM goes through them (copy_in / copy_out), so the
// runtime never has to pin the caller's pages for DMA -- that path took tens of ms per call once an application with many
// threads was mapping and unmapping memory around it.  Memory from slk_host_alloc / slk_host_register skips them.
constexpr int N_STAGE = 3;
struct Staging {
  PinnedPtr<void> buf[N_STAGE];
  Event ev[N_STAGE];
  bool busy[N_STAGE] = {};
  int next = 0;
  void release() {
    for (int i = 0; i < N_STAGE; i++) { buf[i].reset(); ev[i].reset(); busy[i] = false; }
  }
};

struct slk_index {
  int32_t device = 0;
  slk_params params{};
  ScanParams sp{};
  DevPtr<uint64_t> cells;
  uint64_t nbuckets = 0;
  int32_t bucket_bits = 0, taxon_bits = 0, disp_bits = 0;   // bucket_bits = ceil(log2(nbuckets)): the hash bits that choose the bucket
  bool bucket_flag = false;        // the cells keep their top bit for the buckets' "a record went past" flag (engine.h: TableGeom.flag)
  uint32_t shard = 0, n_shards = 0;  // slk_index_set_shard: keep only the records of this shard
  DevPtr<int32_t> d_max_disp;
  DevPtr<unsigned long long> d_counters;  // inserted, duplicate, overflow, negative taxa skipped (several id columns)
  DevPtr<int32_t> d_parents;      // the taxonomy as given (ids of the caller)
  int32_t T = 0;
  std::vector<int32_t> h_parents;  // host copy, for the dense renumbering at finalize
  // dense taxon ids (engine.h: TableView.to_orig): set up by slk_index_finalize when the caller's ids need more than 22 bits
  DevPtr<int32_t> d_parents_dense, d_to_orig, d_to_dense;
  // Euler tours (index.hip: build_tax_nodes).  The two owners: of the taxonomy as given (the staged classify kernel works in the
  // caller's ids; null: more than 2^26 ids) and of the dense renumbering.  d_nodes is a VIEW of one of them: kernel_parents() with
  // its tour (engine.h: FusedArgs.nodes); null: more than 2^22 ids, no lane kernel.
  DevPtr<uint4> d_nodes_orig, d_nodes_dense;
  const uint4 *d_nodes = nullptr;
  int32_t D = 0;                   // nodes of the taxonomy = largest dense id (0: ids are stored as given)
  bool finalized = false;
  int32_t max_disp = 0;
  uint64_t records = 0, dups = 0;
  uint64_t unplaced = 0;           // records of the last insert that found no cell within reach of the displacement field (index.hip: insert_growing)
  uint32_t grown = 0;              // times the table was moved to a larger one because of that
  float load_target = 0;           // the load factor the table was sized for (given, or chosen by the free memory: slk_index_create)
  bool spent = false;              // the table was lost while it was growing (index.hip: grow_table): only slk_index_destroy takes the index
  // slk_index_merge_*: the translation of source taxa (slk_index_set_merge_remap; null: none) and what a pass leaves of the records
  // it refused (engine.h: MergeCheck.bad)
  DevPtr<int32_t> d_merge_remap;
  int32_t n_merge_remap = 0;
  DevPtr<unsigned long long> d_merge_bad;
  Stream build_stream;
  DevBuf stage_keys, stage_taxa;
  Staging staging;    // host -> HBM copies of the build calls
  int W = 1;          // id columns; > 1: the wide path (wide.hip) with its own table
  WideParams wp{};
  WideTable wt{};    // (a view: the two arrays are owned by wide_keys / wide_taxa)
  DevPtr<uint64_t> wide_keys;
  DevPtr<int32_t> wide_taxa;

  static TableGeom geom_of(uint64_t nbuckets, int32_t bucket_bits, bool bucket_flag, int32_t taxon_bits, int32_t disp_bits) {
    TableGeom g{};
    g.nbuckets = nbuckets;
    g.q = bucket_bits;
    g.rem_mask = (1ULL << (64 - bucket_bits)) - 1;
    g.flag = bucket_flag ? (1ULL << 63) : 0;
    g.taxon_bits = taxon_bits;
    g.disp_bits = disp_bits;
    return g;
  }
  TableGeom geom() const { return geom_of(nbuckets, bucket_bits, bucket_flag, taxon_bits, disp_bits); }
  TableView view() const {
    TableView v;
    v.cells = cells;
    v.g = geom();
    v.max_disp = max_disp;
    v.to_orig = d_to_orig;
    return v;
  }
  // what the fused kernels walk: the parents array in the ids the cells hold
  const int32_t *kernel_parents() const { return D ? d_parents_dense : d_parents; }
  const uint4 *kernel_nodes() const { return d_nodes; }
  int32_t kernel_ntax() const { return D ? D + 1 : T; }
  int internal_taxon_bits() const {
    if (!D) return taxon_bits;
    int b = 1;
    while ((1LL << b) <= (long long)D) b++;
    return b;
  }
};

struct slk_stream {
  slk_index *ix = nullptr;
  int32_t device = 0;  // copy: the stream may be destroyed after its index
  Stream s;
  DevBuf span_keys, span_meta, span_taxon, span_count;  // per-batch scratch (sparse per-read regions)
  DevBuf bases, offsets, mate_bases, mate_offsets;      // staging for the host-pointer entry points
  DevBuf out_taxon, out_cls, out_nd, out_tk, out_nh, out_offsets, out_items, defer_list, scan_tmp;
  bool merged_hits = false;                 // slk_stream_set_merged_hits: hit lists as TaxonCounts.fromHits merges them
  DevBuf pk_codes, pk_valid, pk_mate_codes, pk_mate_valid;   // slk_classify_batch_packed: the reads as they arrive (3 bits per base)
  Event ev_unpack;
  DevBuf parse_text, parse_scratch, parse_title_pos, parse_title_len, parse_counts;   // textparse.hip: the raw text, the passes' scratch, what comes back beside bases / offsets
  DevBuf parse_text2, parse_title_pos2, parse_title_len2, parse_pair;   // paired text: the mates' text and titles (their bases / offsets are mate_bases / mate_offsets), the pair record
  DevBuf mask_scratch, mask_count;         // mask.hip: the two bitmaps (sequence starts, masked letters), the host entries' counter
  Stream s2;                               // the segment pass and the wave pass run here, beside the long-lane pass on s
  Event ev_fork, ev_join;
  DevPtr<int32_t> d_status;        // device error bits of the fused kernels
  PinnedPtr<int32_t> h_status;     // pinned copy, refreshed after every classify launch
  Event ev[4];
  Staging staging;
  // large host-pointer calls: the reads go up on a second stream, sub-batch by sub-batch, while the kernels of the
  // sub-batches before run on s (slk_classify_batch)
  Stream cs;
  Staging staging_c;
  std::vector<Event> up_ev;
  // ... and the results of sub-batch i come down on a third stream while sub-batch i + 1 runs (pinned result buffers only)
  Stream ds;
  std::vector<Event> dn_ev;
  bool reran = false;           // check_status classified queued calls again (a taxon map had overflowed): results on the host are stale
  bool timed = false;
  uint32_t last_route = 0;      // SLK_ROUTE_* of the kernels the last classify call launched (slk_stream_last_route), set where they are issued
  bool last_used_lane = false;  // the last classify call ran the lane kernel (defer_list[0] is its deferral count)
  // the piece route (engine.h: PieceArgs): slk_stream_set_split_long, its scratch (header, slots, units, records | the HBM maps), and
  // whether the last classify call ran it (piece_scratch then starts with its header: slk_stream_last_split)
  int64_t split_long = -1;
  bool split_hits = false;       // slk_stream_set_split_hits: calls with hit lists take the route too (piece_hits: their side array)
  DevBuf piece_scratch, piece_maps, piece_hits;
  bool last_used_pieces = false;
  bool split_reported = false;   // SLK_DEBUG_SPLIT: the last call's numbers have been printed (check_status)
  // The arguments of every classify call queued since the stream was last synchronised, for the unbounded re-run
  // (check_status): a taxon-map overflow is only seen at the next synchronisation, and by then several calls may have gone by.
  struct Queued {
    ClassifyCall call;
    bool valid = false;   // the call can be run again (it was a fused classify call)
  };
  std::vector<Queued> queued;
};

constexpr size_t STAGE_BYTES = (size_t)8 << 20;

inline int32_t stage_ready(Staging *g) {
  if (g->ev[N_STAGE - 1]) return SLK_OK;
  for (int i = 0; i < N_STAGE; i++) {
    HIPCHK(hipHostMalloc(g->buf[i].put(), STAGE_BYTES, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(g->ev[i].put(), hipEventDisableTiming));
  }
  return SLK_OK;
}

// caller memory -> HBM, ordered on s.  The caller's buffer is free on return unless it is pinned memory of the library
// (then the DMA reads it directly and is complete when s has been synchronised -- every host entry point does before it
// returns); the last DMA may still be in flight.
inline int32_t copy_in(Staging *g, hipStream_t s, void *d_dst, const void *h_src, size_t n) {
  if (n == 0) return SLK_OK;
  if (pinned().covers(h_src, n)) {
    HIPCHK(hipMemcpyAsync(d_dst, h_src, n, hipMemcpyHostToDevice, s));
    return SLK_OK;
  }
  int32_t rc = stage_ready(g);
  if (rc) return rc;
  for (size_t o = 0; o < n; o += STAGE_BYTES) {
    const size_t len = std::min(STAGE_BYTES, n - o);
    const int b = g->next;
    g->next = (g->next + 1) % N_STAGE;
    if (g->busy[b]) HIPCHK(hipEventSynchronize(g->ev[b]));  // the DMA that last used this buffer
    parallel_memcpy(g->buf[b], (const char *)h_src + o, len);
    HIPCHK(hipMemcpyAsync((char *)d_dst + o, g->buf[b], len, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(g->ev[b], s));
    g->busy[b] = true;
  }
  return SLK_OK;
}

// HBM -> caller memory, after everything queued on s; complete on return.  The DMA of one piece overlaps the copy of the
// piece before it into the caller's buffer.
inline int32_t copy_out(Staging *g, hipStream_t s, void *h_dst, const void *d_src, size_t n) {
  if (n == 0) return SLK_OK;
  if (pinned().covers(h_dst, n)) {
    HIPCHK(hipMemcpyAsync(h_dst, d_src, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SLK_OK;
  }
  int32_t rc = stage_ready(g);
  if (rc) return rc;
  size_t prev_o = 0, prev_len = 0;
  int prev_b = -1;
  for (size_t o = 0; o < n; o += STAGE_BYTES) {
    const size_t len = std::min(STAGE_BYTES, n - o);
    const int b = prev_b < 0 ? 0 : (prev_b + 1) % N_STAGE;
    // (stream order protects the buffer: an earlier copy_in DMA out of it is queued before this write into it)
    HIPCHK(hipMemcpyAsync(g->buf[b], (const char *)d_src + o, len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(g->ev[b], s));
    g->busy[b] = true;
    if (prev_b >= 0) {
      HIPCHK(hipEventSynchronize(g->ev[prev_b]));
      parallel_memcpy((char *)h_dst + prev_o, g->buf[prev_b], prev_len);
    }
    prev_b = b; prev_o = o; prev_len = len;
  }
  if (prev_b >= 0) {
    HIPCHK(hipEventSynchronize(g->ev[prev_b]));
    parallel_memcpy((char *)h_dst + prev_o, g->buf[prev_b], prev_len);
  }
  return SLK_OK;
}
inline int32_t copy_in(slk_stream *st, void *d_dst, const void *h_src, size_t n) { return copy_in(&st->staging, st->s, d_dst, h_src, n); }
inline int32_t copy_out(slk_stream *st, void *h_dst, const void *d_src, size_t n) { return copy_out(&st->staging, st->s, h_dst, d_src, n); }

// Every entry point that takes an index starts here: select the index's device and drop whatever error code an earlier,
// unrelated HIP call of this thread (this library's or the application's) left behind, so that the hipGetLastError()
// after a launch reports that launch.  An index that lost its table (index.hip: grow_table) is refused.
inline int32_t check_spent(const slk_index *ix) {
  if (ix->spent)
    return fail(SLK_E_STATE, "this index lost its records when its table could not grow: destroy it and repeat the load (with a larger "
                             "slk_table_config.expected_records)");
  return SLK_OK;
}
inline int32_t set_device(const slk_index *ix) {
  int32_t rc = check_spent(ix);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ix->device));
  (void)hipGetLastError();
  return SLK_OK;
}

// The grid of a persistent-block pass: blocks_per_cu blocks for every CU of `device` (< 0: the current one; 256 CUs where the
// runtime does not say), or what the environment variable `env_name` (may be null) gives: the tests' way to a few blocks.
inline unsigned grid_for(int device, int blocks_per_cu, const char *env_name) {
  int cus = 0;
  if ((device < 0 && hipGetDevice(&device) != hipSuccess) ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    cus = 256;
  }
  const long env_blocks = env_name ? env_long(env_name, 0) : 0;
  return env_blocks > 0 ? (unsigned)std::min(env_blocks, 65535L) : (unsigned)cus * (unsigned)blocks_per_cu;
}

// What the analyses that look a library's or a sample's minimizers up in a resident table refuse at create: `what` names the
// analysis, `table` the table in its words; need_scan: it scans sequences with the lane-per-chunk scan (chunkscan.h).
inline int32_t check_whole_narrow_index(const slk_index *ix, const char *what, const char *table, bool need_scan) {
  if (!ix->finalized) return fail(SLK_E_STATE, "index is not finalized");
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "%s supports minimizers of up to 32 nt (one id column)", what);
  if (ix->n_shards > 1) return fail(SLK_E_UNSUPPORTED, "%s needs the whole %s on one GPU (the index is a shard)", what, table);
  if (need_scan && ix->sp.w > BUILD_MAX_W)
    return fail(SLK_E_UNSUPPORTED, "%s supports windows of up to %d m-mers (k - m + 1 = %d)", what, BUILD_MAX_W, ix->sp.w);
  return SLK_OK;
}

// A handle whose counts an earlier failure left incomplete (`spent`) takes no further call.  Every entry of such a handle starts
// with enter_handle and returns through leave_handle; which codes spend the handle is the handle's choice.
template <class H> inline int32_t enter_handle(const H *h, const char *spent_text) {
  if (!h) return fail(SLK_E_INVALID, "null handle");
  if (h->spent) return fail(SLK_E_STATE, "%s", spent_text);
  return set_device(h->ix);
}
template <class H> inline int32_t leave_handle(H *h, int32_t rc, bool spends) {
  if (spends) h->spent = true;
  return rc;
}

// A synchronous host entry leaves with nothing queued that reads or writes the caller's memory: from the first copy it queues, every
// return -- the failing ones too, after which the caller may free its buffers -- passes through this.
struct DrainOnExit {
  slk_stream *st;
  explicit DrainOnExit(slk_stream *st_) : st(st_) {}
  DrainOnExit(const DrainOnExit &) = delete;
  ~DrainOnExit() {
    for (hipStream_t s : {st->cs.get(), st->s.get(), st->ds.get()})
      if (s && hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
  }
};

// What the host-side translation units share, by the file that defines it; not exported (the library exports its extern "C" names only)
namespace slk {
// stream.hip
int32_t check_ready(const slk_index *ix, const slk_stream *st, bool need_tax);
int32_t check_status(slk_stream *st);   // call after the stream has been synchronised
int32_t fork_ready(slk_stream *st);     // st->s2 and the events that fork it from st->s and join it again
// classify.hip: the dispatch
bool use_fused(const slk_index *ix, bool force_v1);      // with SLK_FORCE_V1 as a classify call read it (PlanSwitches.force_v1)
bool lane_path_ok(const slk_index *ix, bool force_v1);
bool use_fused(const slk_index *ix);                      // ... and as the environment has it now: decisions per index, outside a classify call
bool lane_path_ok(const slk_index *ix);
uint64_t span_slots(uint64_t total_bases, uint64_t total_mate_bases, uint64_t R, bool paired);
int32_t ensure_scratch(slk_stream *st, uint64_t slots, uint64_t R);
Thresholds thresholds_of(const double *v, int32_t C);
FusedArgs fused_args(const slk_index *ix, const slk_stream *st, const Reads &in);
void launch_spans(const slk_index *ix, slk_stream *st, const Reads &in, uint64_t *keys, int32_t *meta, int32_t *count);
int32_t run_classify(slk_index *ix, slk_stream *st, const ClassifyCall &call, const PlanSwitches &sw);   // (the switches as the caller read them)
int32_t run_classify(slk_index *ix, slk_stream *st, const ClassifyCall &call);   // the kernels of a batch and the status word's copy, queued on st->s
int32_t run_unbounded(slk_stream *st, const ClassifyCall &c);   // the batch again by the staged kernels (check_status); synchronises st->s
// hostcalls.hip: the pieces of the host entries, which pipe.hip queues per slot and shardset.hip and bracken.hip use too
int32_t validate_reads(const uint64_t *offsets, const uint64_t *mate_offsets, uint64_t R);
int32_t upload_reads(slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const uint8_t *mate_bases,
                     const uint64_t *mate_offsets, uint64_t R, uint64_t *total, uint64_t *mate_total);
int32_t size_host_buffers(slk_stream *st, uint64_t R, int32_t C, uint64_t total, uint64_t mate_total, bool paired, bool pk);
int32_t upload_range(slk_stream *st, Staging *g, hipStream_t up, hipStream_t run, hipEvent_t ev, bool packed, const uint8_t *bases,
                     const uint32_t *codes, const uint16_t *valid, DevBuf &d_codes, DevBuf &d_valid, uint8_t *dst, uint64_t p0, uint64_t p1);
ClassifyCall host_call(slk_stream *st, uint64_t R, uint64_t total, uint64_t mate_total, bool paired, const double *thresholds, int32_t C,
                       int32_t min_hit_groups, bool want_hits, const uint64_t *h_offsets);
int32_t ensure_outputs(slk_stream *st, uint64_t R, int32_t C);   // the stream's result rows (out_taxon .. out_nh) for R fragments
struct HostRows { int32_t *taxon; uint8_t *classified; int32_t *nd, *tk; };   // a host call's results in the caller's memory (nullable from nd on)
int32_t download_rows(slk_stream *st, const HostRows &out, uint64_t R, int32_t C);   // complete on return
int32_t counts_to_offsets(slk_stream *st, const int32_t *d_counts, uint64_t R, uint64_t *out_offsets, uint64_t capacity);
int32_t assemble_hits(slk_stream *st, const Reads &in, bool want_hits, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity,
                      bool call_timing, double th[3]);
// textparse.hip: FASTA / FASTQ text parsed on the device (used by hostcalls.hip: slk_classify_text)
int32_t check_parse_args(uint64_t n, int32_t format);
int32_t parse_uploaded(slk_stream *st, const uint8_t *text, uint64_t n, int32_t format, bool final, uint64_t bases_capacity,
                       uint64_t records_capacity, uint64_t counts[4]);
// two texts parsed (text 1 into bases / offsets, text 2 into mate_bases / mate_offsets) and paired in lockstep; pair: the pair record
// (slk_pair_record as eight words).  Synchronises st->s.  SLK_E_CAPACITY: pair holds the sizes both sides need.
struct PairText { const uint8_t *text; uint64_t n; int32_t format; bool final; uint64_t bases_capacity, records_capacity; };
int32_t parse_pair_uploaded(slk_stream *st, const PairText &t1, const PairText &t2, uint64_t pair[8]);

inline int ceil_log2_u64(uint64_t x) {
  int b = 0;
  while (b < 63 && (1ULL << b) < x) b++;
  return b;
}

// argument checks the entry points repeat
inline int32_t check_thresholds(const double *thresholds, int32_t C) {
  return C < 1 || C > MAX_THRESHOLDS || !thresholds ? fail(SLK_E_INVALID, "need 1..%d thresholds", MAX_THRESHOLDS) : SLK_OK;
}
inline int32_t check_mates(const void *mate_bases, const void *mate_offsets) {
  return (mate_bases == nullptr) != (mate_offsets == nullptr) ? fail(SLK_E_INVALID, "mate_bases and mate_offsets must be given together") : SLK_OK;
}
inline int32_t check_one_id_column(const slk_index *ix) {
  return ix->W > 1 ? fail(SLK_E_UNSUPPORTED, "the staged and sharded entry points support minimizers of up to 32 nt (one id column)") : SLK_OK;
}
}  // namespace slk
