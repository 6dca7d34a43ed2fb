// classify.hip -- the classify side of the C ABI (include/slacken_amd.h): streams and their scratch, the dispatch of a batch to
// the kernels of lane.hip / fused.hip / kernels.hip / wide.hip, the status word and the unbounded re-run, one step of the
// table-sharded pipeline, hit lists, spans, and the host batch entry with its sub-batch pipeline.  Host-side only.
#include "hostside.h"

int32_t slk_stream_create(slk_index *ix, slk_stream **out) {
  if (!ix || !out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  int32_t rc = set_device(ix);
  if (rc) return rc;
  std::unique_ptr<slk_stream> st(new slk_stream());   // (released into *out on success only)
  st->ix = ix;
  st->device = ix->device;
  HIPCHK(hipStreamCreate(st->s.put()));
  for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(st->ev[i].put()));
  HIPCHK(hipMalloc((void **)st->d_status.put(), sizeof(int32_t)));
  HIPCHK(hipMemset(st->d_status, 0, sizeof(int32_t)));
  HIPCHK(hipHostMalloc((void **)st->h_status.put(), sizeof(int32_t), hipHostMallocDefault));
  *st->h_status = 0;
  *out = st.release();
  return SLK_OK;
}

int32_t slk_stream_synchronize(slk_stream *st) {
  if (!st) return fail(SLK_E_INVALID, "null argument");
  { int32_t rc_ = set_device(st->ix); if (rc_) return rc_; }
  HIPCHK(hipStreamSynchronize(st->s));
  return check_status(st);
}

int32_t slk_stream_set_merged_hits(slk_stream *st, int32_t on) {
  if (!st) return fail(SLK_E_INVALID, "null handle");
  st->merged_hits = on != 0;
  return SLK_OK;
}

void *slk_stream_hip_stream(slk_stream *st) { return st ? (void *)st->s : nullptr; }

void slk_stream_destroy(slk_stream *st) {
  if (!st) return;
  (void)hipSetDevice(st->device);
  for (hipStream_t s : {st->s.get(), st->ds.get(), st->s2.get()})
    if (s) (void)hipStreamSynchronize(s);
  delete st;
}

// span slots needed by a batch (see span_region in engine.h)
uint64_t slk::span_slots(uint64_t total_bases, uint64_t total_mate_bases, uint64_t R, bool paired) {
  return total_bases + (paired ? total_mate_bases + R : 0) + 1;
}

int32_t slk::ensure_scratch(slk_stream *st, uint64_t slots, uint64_t R) {
  HIPCHK(st->span_keys.ensure(slots * 8 * st->ix->W));
  HIPCHK(st->span_meta.ensure(slots * 4));
  HIPCHK(st->span_taxon.ensure(slots * 4));
  HIPCHK(st->span_count.ensure((R + 1) * 4));
  return SLK_OK;
}

int32_t slk::check_ready(const slk_index *ix, const slk_stream *st, bool need_tax) {
  if (!ix || !st) return fail(SLK_E_INVALID, "null handle");
  if (st->ix != ix) return fail(SLK_E_INVALID, "stream belongs to a different index");
  if (!ix->finalized) return fail(SLK_E_STATE, "index is not finalized");
  if (need_tax && !ix->d_parents) return fail(SLK_E_STATE, "taxonomy not set");
  return SLK_OK;
}

// The fused wave-per-read kernels (fused.hip) cover windows of up to 32 m-mers; wider windows (and SLK_FORCE_V1=1, an
// A/B switch for tests) run the three separate lane-per-read kernels of kernels.hip.  Both are HIP: no CPU path.
static bool use_fused(const slk_index *ix) {
  static const bool force_v1 = env_on("SLK_FORCE_V1");
  return !force_v1 && ix->W == 1 && ix->sp.w <= 32;
}

// The fused kernels keep a fragment's taxon -> count map in LDS (12 slots per lane, 128 per wave).  A fragment that hits more
// distinct taxa than that (long reads across conserved regions can) raises status bit 1; the batch is then classified again
// by the staged kernels, whose per-fragment map lives in HBM scratch and is unbounded -- the same three kernels that serve
// windows wider than 32 m-mers.  Slower (HBM intermediates), rare, and bit-identical for every other fragment.
static int32_t run_unbounded(slk_stream *st, const ClassifyCall &c) {
  slk_index *ix = st->ix;
  const Reads &in = c.in;
  int32_t rc = ensure_scratch(st, span_slots(in.total, in.mate_total, in.R, in.paired()) + c.span_shift, in.R);
  if (rc) return rc;
  uint64_t *const keys = st->span_keys.as<uint64_t>() + c.span_shift;   // (fused path only: one key word per span)
  int32_t *const meta = st->span_meta.as<int32_t>() + c.span_shift, *const taxa = st->span_taxon.as<int32_t>() + c.span_shift;
  launch_scan(ix->sp, in.bases, in.offsets, in.mate_bases, in.mate_offsets, in.R, keys, meta, st->span_count.as<int32_t>(), st->s);
  launch_probe(ix->view(), in.offsets, in.mate_offsets, in.R, keys, meta, st->span_count.as<int32_t>(), taxa, st->s);
  launch_classify(ix->d_parents, ix->d_nodes_orig, ix->T, c, meta, taxa, st->span_count.as<int32_t>(), keys, st->s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st->s));
  return SLK_OK;
}

int32_t slk::check_status(slk_stream *st) {
  int32_t v = *st->h_status;
  // SLK_DEBUG_SPLIT (tuning and test aid, like SLK_DEBUG_CALL_TIMING): what the piece route did in the call that is through, once per
  // call, for the callers whose streams nobody else can ask (a slk_pipe's slots, the command line's workers)
  if (st->last_used_pieces && !st->split_reported && getenv("SLK_DEBUG_SPLIT") != nullptr) {
    uint64_t hdr[PieceHdr::WORDS];
    if (hipMemcpy(hdr, st->piece_scratch.p, sizeof(hdr), hipMemcpyDeviceToHost) == hipSuccess)
      fprintf(stderr, "slk split: %llu fragments, %llu pieces, %llu spills\n", (unsigned long long)hdr[PieceHdr::N_FRAG],
              (unsigned long long)hdr[PieceHdr::N_UNIT], (unsigned long long)hdr[PieceHdr::SPILLS]);
    st->split_reported = true;
  }
  std::vector<slk_stream::Queued> queued;
  queued.swap(st->queued);
  if (v != 0) {
    *st->h_status = 0;
    HIPCHK(hipMemsetAsync(st->d_status, 0, sizeof(int32_t), st->s));
    if (v == 1 && !queued.empty()) {
      // Some queued batch held a fragment with more distinct taxa than the LDS maps take.  The status word does not say
      // which, so every batch queued since the last synchronisation is classified again by the unbounded kernels, in
      // order (callers that reuse their output buffers from call to call end up with the last call's results, as before).
      for (const slk_stream::Queued &q : queued) {
        if (!q.valid) return fail(SLK_E_CAPACITY, "a fragment hit more than %d distinct taxa; the per-read taxon map overflowed", 128);
        int32_t rc = run_unbounded(st, q.call);
        if (rc) return rc;
      }
      st->reran = true;
      return SLK_OK;
    }
    if (v & PIECE_STATUS_TOO_LONG) return fail(SLK_E_INVALID, "a fragment of 2^31 bases or more cannot be split into pieces (slk_stream_set_split_long)");
    if (v & PIECE_STATUS_SCRATCH) return fail(SLK_E_INVALID, "the piece route's scratch, sized from total_bases, did not hold the batch's fragments: total_bases smaller than the batch?");
    if (v & PIECE_STATUS_MAP) return fail(SLK_E_HIP, "internal: a split fragment named more taxa than its map was sized for (device status %d)", v);
    if (v & 2) return fail(SLK_E_CAPACITY, "a send region of slk_shard_step_device's EMIT job overflowed its capacity_per_owner");
    if (v & 1) return fail(SLK_E_CAPACITY, "a fragment hit more than %d distinct taxa; the per-read taxon map overflowed", 128);
    return fail(SLK_E_HIP, "device status %d", v);
  }
  return SLK_OK;
}

bool slk::lane_path_ok(const slk_index *ix) {
  return use_fused(ix) && ix->sp.w <= 32 && ix->internal_taxon_bits() <= 22 && ix->d_nodes != nullptr;
}

// the second stream of a classify call or a sharded step, and the two events that fork it from s and join it again
static int32_t fork_ready(slk_stream *st) {
  if (st->ev_join) return SLK_OK;
  HIPCHK(hipStreamCreateWithFlags(st->s2.put(), hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(st->ev_fork.put(), hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(st->ev_join.put(), hipEventDisableTiming));
  return SLK_OK;
}

// the part of FusedArgs every job shares: the splitter, the table, the taxonomy in the table's ids, the reads, the status word
static FusedArgs fused_args(const slk_index *ix, const slk_stream *st, const Reads &in) {
  FusedArgs A{};
  A.P = ix->sp; A.T = ix->view(); A.parents = ix->kernel_parents(); A.ntax = ix->kernel_ntax(); A.nodes = ix->kernel_nodes();
  A.bases = in.bases; A.offsets = in.offsets; A.mate_bases = in.mate_bases; A.mate_offsets = in.mate_offsets; A.R = in.R;
  A.status = st->d_status;
  return A;
}
Thresholds slk::thresholds_of(const double *v, int32_t C) {
  Thresholds thr{};
  memcpy(thr.v, v, C * sizeof(double));
  return thr;
}

// the spans of a batch, by the kernel that scans for this index
static void launch_spans(const slk_index *ix, slk_stream *st, const Reads &in, uint64_t *keys, int32_t *meta, int32_t *count) {
  if (ix->W > 1) {
    launch_wide_scan(ix->wp, in.bases, in.offsets, in.mate_bases, in.mate_offsets, in.R, keys, meta, count, st->s);
  } else if (use_fused(ix)) {
    FusedArgs A = fused_args(ix, st, in);
    A.span_keys = keys; A.span_meta = meta; A.span_count = count;
    launch_fused(MODE_SPANS, A, st->s);
  } else {
    launch_scan(ix->sp, in.bases, in.offsets, in.mate_bases, in.mate_offsets, in.R, keys, meta, count, st->s);
  }
}

// The routing of a batch on the hot path, one lane per fragment (window of at most 32 m-mers, taxon ids of at most 22 bits:
// lane_path_ok).  What that kernel does not take -- fragments over 1000 bases, taxon maps that overflow -- it appends to the hand-on
// list of the kernel that does (engine.h: FusedArgs.hand_*): four length classes for its own long variant (1001 .. 4999 bases), the
// lane-per-segment kernel (unpaired, w = 5, the fragments that are long for their batch), the wave-per-fragment kernel (the rest, and
// what the long variant hands on in turn).  Everything here follows from the batch's numbers and five switches, read per call so
// that tests can move them (SLK_FORCE_WAVE alone is read once per process).
struct LanePlan {
  bool lane = false;                             // the lane path runs at all (else: the wave-per-fragment kernel alone)
  bool route_first = false, seg_on = false;      // a routing kernel stands for the first pass; the lane-per-segment kernel takes its share
  uint32_t long_max = 0, long_bound[3] = {0, 0, 0};   // the long variant's limit (0: no such pass) and the borders of its classes
  uint32_t seg_min_len = 0, wave_min = 0, wave_ratio_q10 = 0;
  uint64_t long_cap = 0;      // entries of a list of fragments over 1000 bases
  size_t hand_bytes = 0;      // the hand-on buffer: header and lists
  // the piece route (engine.h: PieceArgs): on when piece_min_len != 0; then seg_min_len is at most piece_min_len, so that the
  // routing hands every fragment the cut may take to the segment pass's list
  uint32_t piece_min_len = 0, piece_windows = 0;
  uint64_t piece_frags = 0, piece_units = 0, piece_map = 0;   // entries the batch can need at most
  bool piece_hits = false;    // the route writes hit lists (slk_stream_set_split_hits): a side array of PieceHitRecords, the move kernel
};
// The engine's own threshold of the piece route (slk_stream_set_split_long(-1)): the smallest length at which the route measured
// faster than the routes before it by more than the spread of the runs (profiles/r16_contigs.json: 100 against 82 Gbp/s at 300 kbp,
// 105 / 41 at 1 Mbp, 108 / 10 at 4 Mbp), never under two pieces.  Unasked, the route runs only where the host can tell
// that it costs nothing: in batches whose fragments average over 1000 bases (the batches of reads -- the headline -- see no launch,
// memset or allocation of it), and while its map scratch stays under PIECE_DEFAULT_MAP_BYTES (a caller who names a threshold gets
// the scratch the batch needs, whatever it is).
// What the batch needs: with the offsets on the host (h_offsets: slk_classify_batch[_packed], slk_classify_text) the fragments at or
// above the threshold are counted and their pieces and map ranges summed exactly -- a batch without such a fragment runs nothing of
// the route.  The device entries know total_bases alone: the sums are bounds then (a cut fragment has at least min_len bases, makes at
// most n / windows + 1 pieces of its n windows, and its map has at most 4 min(n, taxa) + 64 entries), and a batch that holds
// min_len bases in all gets the header's memset, the four launches and the scratch of those bounds whether it has a long fragment or not.
constexpr int64_t PIECE_DEFAULT_MIN_LEN = 300000;
constexpr uint64_t PIECE_DEFAULT_MAP_BYTES = 2ull << 30;
// ... and under PIECE_DEFAULT_MAP_PER_BASE bytes per base of the batch: the ranges are cleared before the pieces run and read whole by
// the merge, and where they outweigh the bases the route loses what it gains (18 taxon bits, profiles/r16_contigs_18bit.json: 28 bytes
// of map per base at 300 kbp, 34 against the parent's 79 Gbp/s; 8.4 at 1 Mbp, 54 against 40; 2.1 at 4 Mbp, 59 against 10)
constexpr uint64_t PIECE_DEFAULT_MAP_PER_BASE = 8;
static LanePlan plan_lane(uint64_t R, uint64_t all_bases, bool paired, bool want_hits, int w, int64_t split_long, bool split_hits,
                          uint32_t taxa_bound, const uint64_t *h_offsets, int k) {
  LanePlan p;
  static const bool force_wave = env_on("SLK_FORCE_WAVE");   // A/B switch: classify with the wave-per-read kernel only
  p.lane = !force_wave && R < 0xFFFFFFFFull;
  if (!p.lane) return p;
  p.long_cap = std::min<uint64_t>(R, all_bases / 1001 + 1);
  // SLK_LANE_LONG_MAX moves the long variant's limit (at most 8191: queue entries carry 13-bit k-mer counts; 0: no such pass)
  const int long_max = (int)std::min(env_long("SLK_LANE_LONG_MAX", 4999), 8191L);
  // A batch whose fragments average more than 1000 bases gets a routing kernel instead of a first pass (engine.h:
  // FusedArgs.hand_short; SLK_ROUTE_FIRST=0 / 1 says so either way)
  const char *route_env = getenv("SLK_ROUTE_FIRST");
  p.route_first = long_max > 1000 && (route_env ? route_env[0] == '1' : all_bases / 1000 > R);
  p.hand_bytes = HandOn::WORDS * sizeof(uint64_t) + HandOn::entries(R, p.long_cap, p.route_first) * sizeof(uint32_t);
  // SLK_SEG_MIN_LEN moves the segment kernel's limit (0: wave kernel only).
  // Wave or segment kernel: on batches of ONE length the wave kernel is the faster one up to ~250 000 bases since round 4's diet
  // (115 against 101 Gbp/s at 15 kbp, 111 / 100 at 30 kbp, 91 / 92 at 100 kbp, 90 / 74 at 200 kbp, 70 / 75 at 300 kbp,
  // profiles/r04_long_routes.txt) -- but it takes a fragment per wave at ~15 Mbp/s, so a fragment that is long for its batch is
  // what the batch then waits for.  So the default follows the batch: the segment kernel takes what a single wave would need
  // about half the batch's time for -- fragments of more than 1/16384 of the batch's bases --, never under 16 000 bases (below
  // that its lanes have too little each) and always from 250 000; and the wave kernel starts its long fragments longest first
  // (engine.h: hand_hdr).  Nanopore-like mix, 200 .. 50 000 bases, 1 Gbp: 90-94 Gbp/s with the threshold at 12-16 000, 93-99 at
  // 30 000, 97-101 at 64 000 (none on the segment kernel).
  const uint64_t seg_auto = std::min<uint64_t>(250000, std::max<uint64_t>(16000, all_bases >> 14));
  const int seg_min = (int)env_long("SLK_SEG_MIN_LEN", (long)seg_auto);
  // (hit lists: the segment kernel can put them together -- SLK_SEG_HITS=1 --, but the queues that take its spans to memory
  //  in order cost it half its resident waves, and it measured 51-53 Gbp/s against the wave kernel's 68-79 on the same reads:
  //  profiles/r03_long_hits_*.json; so per-read lines of long reads keep the wave kernel unless asked otherwise)
  const bool seg_ok = !paired && w == 5 && seg_min > 0;
  p.seg_on = (!want_hits || env_on("SLK_SEG_HITS")) && seg_ok;
  p.long_max = long_max > 1000 ? (uint32_t)long_max : 0;
  if (p.long_max) {  // class borders: a geometric ladder from 1000 to the limit (a tile's lanes then differ by at most ~1.5x)
    const double ratio = pow((double)p.long_max / 1000.0, 0.25);
    for (int i = 0; i < 3; i++) p.long_bound[i] = (uint32_t)(1000.0 * pow(ratio, i + 1));
  }
  p.seg_min_len = p.seg_on ? (uint32_t)std::max(seg_min, (int)std::max<uint32_t>(p.long_max, 1000) + 1) : 0;
  p.wave_min = std::max<uint32_t>(p.long_max, 1000) + 1;   // (the wave kernel's eight length classes: 1.75^7 = 50 times the shortest)
  p.wave_ratio_q10 = 1792;
  // The piece route takes what the segment kernel would, cut up: same scope (unpaired, w = 5, no hit lists).  SLK_PIECE_MIN_LEN
  // overrides the stream's setting (0: off), SLK_PIECE_WINDOWS sets the piece size (a multiple of 64, at least 64 x 64).
  // A call that wants hit lists takes it only where the caller asked for both: a threshold (never the engine's own choice) and
  // slk_stream_set_split_hits, which SLK_PIECE_HITS=0|1 overrides; the segment pass is then on for the cut's sake, and unless
  // SLK_SEG_HITS says otherwise its list holds nothing but what the cut takes.
  const char *piece_env = getenv("SLK_PIECE_MIN_LEN");
  int64_t piece_min = piece_env ? atoll(piece_env) : split_long;
  const bool unasked = piece_min < 0;
  const char *hits_env = getenv("SLK_PIECE_HITS");
  const bool hits_on = hits_env ? hits_env[0] == '1' : split_hits;
  if (want_hits ? (seg_ok && hits_on && piece_min > 0) : (p.seg_on && (unasked ? p.route_first : piece_min > 0))) {
    const uint64_t win = (uint64_t)std::max(1L, env_long("SLK_PIECE_WINDOWS", (long)PIECE_DEFAULT_WINDOWS));
    p.piece_windows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((win + 63) / 64 * 64, PIECE_MIN_WINDOWS), 1u << 30);
    if (unasked) piece_min = std::max<int64_t>(PIECE_DEFAULT_MIN_LEN, 2 * (int64_t)p.piece_windows);
    const uint64_t min_len = std::min<uint64_t>(std::max<uint64_t>((uint64_t)piece_min, (uint64_t)std::max<uint32_t>(p.long_max, 1000) + 1), 0x7FFFFFFFull);
    uint64_t units = 0;
    if (h_offsets) {
      for (uint64_t r = 0; r < R; r++) {
        const uint64_t len = h_offsets[r + 1] - h_offsets[r];
        if (len < min_len || len > 0x7FFFFFFFull) continue;   // (host entries hold no longer fragment: validate_reads)
        const uint32_t nwin = (uint32_t)len - (uint32_t)k + 1;
        p.piece_frags++;
        units += (nwin + p.piece_windows - 1) / p.piece_windows;
        p.piece_map += piece_map_cap(nwin, taxa_bound);
      }
    } else {
      p.piece_frags = std::min<uint64_t>(R, all_bases / min_len);
      units = all_bases / p.piece_windows + p.piece_frags;
      p.piece_map = 4 * std::min<uint64_t>(all_bases, p.piece_frags * (uint64_t)taxa_bound) + 64 * p.piece_frags;
    }
    // (no fragment of the batch is that long, or the engine's own choice would take too much scratch: nothing of the route runs)
    const uint64_t map_bytes = p.piece_map * 2 * sizeof(int32_t);
    if (p.piece_frags != 0 && !(unasked && (map_bytes > PIECE_DEFAULT_MAP_BYTES || map_bytes > PIECE_DEFAULT_MAP_PER_BASE * all_bases))) {
      p.piece_min_len = (uint32_t)min_len;
      p.piece_units = units;
      p.piece_hits = want_hits;
      p.seg_min_len = p.seg_on ? std::min(p.seg_min_len, p.piece_min_len) : p.piece_min_len;
      p.seg_on = true;
    }
  }
  return p;
}

int32_t slk::run_classify(slk_index *ix, slk_stream *st, const ClassifyCall &call) {
  ClassifyCall c = call;
  if (c.out.stride == 0) c.out.stride = c.in.R;
  const Reads &in = c.in;
  const uint64_t R = in.R, span_shift = c.span_shift;
  const bool paired = in.paired(), want_hits = c.want_hits;
  bool fused = use_fused(ix);
  int32_t rc;
  st->last_used_lane = false;
  if (!fused || want_hits) {
    rc = ensure_scratch(st, span_slots(in.total, in.mate_total, R, paired) + span_shift, R);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(st->ev[0], st->s));
  if (st->queued.size() >= 4096) {  // (a caller that never synchronises: settle what is queued before taking more)
    HIPCHK(hipStreamSynchronize(st->s));
    rc = check_status(st);
    if (rc) return rc;
  }
  st->queued.push_back({c, fused});
  if (fused) {
    FusedArgs A = fused_args(ix, st, in);
    A.out_stride = c.out.stride;
    A.min_hit_groups = c.min_hit_groups; A.thr = c.thr; A.C = c.C;
    A.out_taxon = c.out.taxon; A.out_classified = c.out.classified;
    A.out_nd = c.out.nd; A.out_tk = c.out.tk; A.out_nh = c.out.nh; A.out_np = c.out.np;
    A.span_meta = want_hits ? st->span_meta.as<int32_t>() + span_shift : nullptr;
    A.span_taxon = want_hits ? st->span_taxon.as<int32_t>() + span_shift : nullptr;
    A.span_count = want_hits ? st->span_count.as<int32_t>() : nullptr;
    const uint32_t taxa_bound = 1u << std::min(ix->internal_taxon_bits(), 22);   // (lane_path_ok: at most 22 bits)
    const LanePlan plan = lane_path_ok(ix) ? plan_lane(R, in.total + in.mate_total, paired, want_hits, ix->sp.w, st->split_long, st->split_hits, taxa_bound, c.h_offsets, ix->sp.k) : LanePlan{};
    st->last_used_pieces = false;
    st->split_reported = false;
    if (plan.lane) {
      st->last_used_lane = true;
      const size_t hdr_bytes = HandOn::WORDS * sizeof(uint64_t);
      HIPCHK(st->defer_list.ensure(plan.hand_bytes));
      HIPCHK(hipMemsetAsync(st->defer_list.p, 0, hdr_bytes, st->s));
      A.hand_hdr = (unsigned long long *)st->defer_list.p;
      A.hand_lists = (uint32_t *)((char *)st->defer_list.p + hdr_bytes);
      A.hand_stride = R; A.hand_long_cap = plan.long_cap; A.route_first = plan.route_first ? 1 : 0;
      A.long_max = plan.long_max; memcpy(A.long_bound, plan.long_bound, sizeof(A.long_bound));
      A.seg_min_len = plan.seg_min_len; A.wave_min = plan.wave_min; A.wave_ratio_q10 = plan.wave_ratio_q10;
      if (plan.route_first) launch_route(A, st->s);
      else launch_lane(A, nullptr, 1000, st->s);  // (the one-word map entries carry 10-bit k-mer counts)
      // The passes over the hand-on lists depend on the first pass only, and the long variant runs BESIDE the other two (which
      // follow each other on a second stream): with a few hundred thousand long fragments in a batch the long variant is a handful
      // of waves per CU working through 5 000 lockstep steps, the segment pass not much more, and the wave kernel behind them on one
      // stream waited for both (nanopore-like mix: 1.1 + 4.9 + 5.8 ms one after the other, 77-84 Gbp/s; 95-101 this way;
      // profiles/r04_long_mixed_trace.txt).  Segment pass before wave pass: the wave kernel is bound by instruction issue and holds
      // every wave slot until it is through, the other two are chains of dependent steps that share a CU well.  What the long
      // variant hands on in turn (map overflows) goes to a list of its own that a second launch of the wave kernel takes when
      // both streams are through.
      rc = fork_ready(st);
      if (rc) return rc;
      HIPCHK(hipEventRecord(st->ev_fork, st->s));
      if (A.long_max) launch_lane_long(A, A.long_max, st->s);   // (first: its chain of steps is the longest, whoever comes first gets the CUs)
      HIPCHK(hipStreamWaitEvent(st->s2, st->ev_fork, 0));
      if (plan.piece_min_len) {
        // the piece route's scratch: header, fragment slots, unit list, piece records; and the maps
        const size_t hdr_b = PieceHdr::WORDS * sizeof(uint64_t), frag_b = plan.piece_frags * sizeof(PieceFrag), unit_b = plan.piece_units * sizeof(uint64_t);
        HIPCHK(st->piece_scratch.ensure(hdr_b + frag_b + unit_b + plan.piece_units * sizeof(PieceRecord)));
        HIPCHK(st->piece_maps.ensure(plan.piece_map * 2 * sizeof(int32_t)));
        if (plan.piece_hits) HIPCHK(st->piece_hits.ensure(plan.piece_units * sizeof(PieceHitRecord)));
        PieceArgs X{};
        char *const base = (char *)st->piece_scratch.p;
        X.hdr = (unsigned long long *)base; X.frags = (PieceFrag *)(base + hdr_b); X.units = (uint64_t *)(base + hdr_b + frag_b);
        X.records = (PieceRecord *)(base + hdr_b + frag_b + unit_b);
        X.map_key = st->piece_maps.as<int32_t>(); X.map_cnt = X.map_key + plan.piece_map;
        X.frag_cap = plan.piece_frags; X.unit_cap = plan.piece_units; X.map_cap = plan.piece_map;
        X.seg_list = A.hand_lists + HandOn::list_at(HandOn::SEG, R, plan.long_cap); X.seg_count = A.hand_hdr + HandOn::SEG;
        X.min_len = plan.piece_min_len; X.windows = plan.piece_windows; X.taxa_bound = taxa_bound;
        HIPCHK(hipMemsetAsync(X.hdr, 0, hdr_b, st->s2));
        FusedArgs P = A;
        if (plan.piece_hits) {
          X.hits = st->piece_hits.as<PieceHitRecord>();
          P.span_keys = st->span_keys.as<uint64_t>() + span_shift;   // (the provisional region, as the segment pass below has it)
        }
        launch_pieces(P, X, st->s2);   // (before the segment pass: the cut takes its fragments out of that pass's list)
        st->last_used_pieces = true;
      }
      if (plan.seg_on) {
        FusedArgs B = A;
        if (want_hits) B.span_keys = st->span_keys.as<uint64_t>() + span_shift;   // (scratch of the hit lists: the spans' places before the borders are settled)
        B.work_list = A.hand_lists + HandOn::list_at(HandOn::SEG, R, plan.long_cap); B.work_count = A.hand_hdr + HandOn::SEG; B.work_draw = A.hand_hdr + HandOn::SEG_DRAW;
        launch_segments(B, st->s2);
      }
      {
        FusedArgs W = A;
        launch_order_wave_list(W, st->s2);
        W.work_list = A.hand_lists + HandOn::ordered_at(R, plan.long_cap); W.work_count = A.hand_hdr + HandOn::ORDERED; W.work_draw = A.hand_hdr + HandOn::WAVE_DRAW;
        launch_fused(want_hits ? MODE_HITS : MODE_CLASSIFY, W, st->s2);
      }
      HIPCHK(hipEventRecord(st->ev_join, st->s2));
      HIPCHK(hipStreamWaitEvent(st->s, st->ev_join, 0));
      if (A.long_max) {
        A.work_list = A.hand_lists + HandOn::list_at(HandOn::LATE, R, plan.long_cap); A.work_count = A.hand_hdr + HandOn::N_LATE; A.work_draw = A.hand_hdr + HandOn::LATE_DRAW;
        launch_fused(want_hits ? MODE_HITS : MODE_CLASSIFY, A, st->s);
      }
    } else {
      launch_fused(want_hits ? MODE_HITS : MODE_CLASSIFY, A, st->s);
    }
    HIPCHK(hipEventRecord(st->ev[1], st->s));
    HIPCHK(hipEventRecord(st->ev[2], st->s));
  } else {
    uint64_t *const keys = st->span_keys.as<uint64_t>();
    int32_t *const meta = st->span_meta.as<int32_t>(), *const taxa = st->span_taxon.as<int32_t>(), *const count = st->span_count.as<int32_t>();
    launch_spans(ix, st, in, keys, meta, count);   // (not the fused kernel here)
    HIPCHK(hipEventRecord(st->ev[1], st->s));
    if (ix->W > 1) launch_wide_probe(ix->wt, ix->W, in.offsets, in.mate_offsets, R, keys, meta, count, taxa, st->s);
    else launch_probe(ix->view(), in.offsets, in.mate_offsets, R, keys, meta, count, taxa, st->s);
    HIPCHK(hipEventRecord(st->ev[2], st->s));
    // the key slots are dead after the probe: the per-read taxon->count map reuses them
    launch_classify(ix->d_parents, ix->d_nodes_orig, ix->T, c, meta, taxa, count, keys, st->s);
  }
  HIPCHK(hipEventRecord(st->ev[3], st->s));
  HIPCHK(hipMemcpyAsync(st->h_status, st->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st->s));
  HIPCHK(hipGetLastError());
  st->timed = true;
  return SLK_OK;
}

int32_t slk_classify_batch_device(slk_index *ix, slk_stream *st, const uint8_t *d_bases, const uint64_t *d_offsets,
                                  const uint8_t *d_mate_bases, const uint64_t *d_mate_offsets, uint64_t R,
                                  uint64_t total_bases, uint64_t total_mate_bases, int32_t min_hit_groups,
                                  const double *thresholds, int32_t C, int32_t *d_out_taxon,
                                  uint8_t *d_out_classified, int32_t *d_out_num_distinct,
                                  int32_t *d_out_total_kmers, int32_t *d_out_num_hits,
                                  int32_t *d_out_num_probes) {
  int32_t rc = check_ready(ix, st, true);
  if (rc) return rc;
  if ((rc = check_thresholds(thresholds, C))) return rc;
  if (R && (!d_bases || !d_offsets || !d_out_taxon || !d_out_classified)) return fail(SLK_E_INVALID, "null argument");
  if ((rc = check_mates(d_mate_bases, d_mate_offsets))) return rc;
  rc = set_device(ix);
  if (rc) return rc;
  ClassifyCall c;
  c.in = {d_bases, d_offsets, d_mate_bases, d_mate_offsets, R, total_bases, total_mate_bases};
  c.out = {d_out_taxon, d_out_classified, d_out_num_distinct, d_out_total_kmers, d_out_num_hits, d_out_num_probes, R};
  c.thr = thresholds_of(thresholds, C); c.C = C; c.min_hit_groups = min_hit_groups;
  return run_classify(ix, st, c);
}

int32_t slk_scan_device(slk_index *ix, slk_stream *st, const uint8_t *d_bases, const uint64_t *d_offsets,
                        const uint8_t *d_mate_bases, const uint64_t *d_mate_offsets, uint64_t R,
                        uint64_t *d_span_keys, int32_t *d_span_meta, int32_t *d_span_count) {
  int32_t rc = check_ready(ix, st, false);
  if (rc) return rc;
  if ((rc = check_one_id_column(ix))) return rc;
  if (R && (!d_bases || !d_offsets || !d_span_keys || !d_span_meta || !d_span_count)) return fail(SLK_E_INVALID, "null argument");
  if ((rc = check_mates(d_mate_bases, d_mate_offsets))) return rc;
  rc = set_device(ix);
  if (rc) return rc;
  launch_spans(ix, st, {d_bases, d_offsets, d_mate_bases, d_mate_offsets, R}, d_span_keys, d_span_meta, d_span_count);
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

int32_t slk_lookup_device(slk_index *ix, slk_stream *st, const int64_t *d_keys, uint64_t n, int32_t *d_out_taxa) {
  int32_t rc = check_ready(ix, st, false);
  if (rc) return rc;
  if ((rc = check_one_id_column(ix))) return rc;
  if (n && (!d_keys || !d_out_taxa)) return fail(SLK_E_INVALID, "null argument");
  rc = set_device(ix);
  if (rc) return rc;
  launch_lookup_coop(ix->view(), d_keys, n, d_out_taxa, st->s);
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

// FusedArgs / ShardIO of a batch's EMIT job from its lists
static void fill_emit(const slk_index *ix, slk_stream *st, const slk_shard_lists &E, FusedArgs &A, ShardIO &S) {
  A = fused_args(ix, st, {E.d_bases, E.d_offsets, E.d_mate_bases, E.d_mate_offsets, E.R});
  A.span_meta = E.d_span_meta; A.span_taxon = E.d_span_taxon; A.span_count = E.d_span_count;
  S.n_shards = (int32_t)E.n_shards; S.chunk = slk_shard_chunk(E.n_shards); S.cap = E.capacity_per_owner;
  S.send_keys = E.d_send_keys; S.cursors = (unsigned long long *)E.d_cursors; S.send_meta = E.d_send_meta;
  S.batch_log = (uint4 *)E.d_batch_log; S.tile_rows = (uint2 *)E.d_tile_rows; S.read_info = (int2 *)E.d_read_info;
}
static int32_t check_lists(const slk_shard_lists &E, const char *what) {
  if (E.n_shards < 1 || E.n_shards > 64) return fail(SLK_E_INVALID, "%s: n_shards %u outside 1..64", what, E.n_shards);
  const uint32_t chunk = slk_shard_chunk(E.n_shards);
  if (E.capacity_per_owner < chunk || E.capacity_per_owner % chunk != 0 || E.capacity_per_owner >= (1ull << 32))
    return fail(SLK_E_INVALID, "%s: capacity_per_owner must be a multiple of slk_shard_chunk(n_shards) = %u below 2^32", what, chunk);
  if (!E.d_cursors || !E.d_defer || (E.R && (!E.d_offsets || !E.d_send_keys || !E.d_send_meta || !E.d_batch_log || !E.d_tile_rows || !E.d_read_info)))
    return fail(SLK_E_INVALID, "%s: null argument", what);
  if ((E.d_mate_bases == nullptr) != (E.d_mate_offsets == nullptr)) return fail(SLK_E_INVALID, "%s: mate_bases and mate_offsets must be given together", what);
  if ((E.d_span_meta == nullptr) != (E.d_span_taxon == nullptr) || (E.d_span_meta == nullptr) != (E.d_span_count == nullptr))
    return fail(SLK_E_INVALID, "%s: the span arrays of the hit lists must be given together", what);
  if (E.R >= 0xFFFFFFFFull) return fail(SLK_E_INVALID, "%s: a batch holds fewer than 2^32 fragments", what);
  return SLK_OK;
}

// One pipeline step of the table-sharded mode (engine.h: ShardIO): up to three jobs of three different batches in ONE kernel.
int32_t slk_shard_step_device(slk_index *ix, slk_stream *st, const slk_shard_lists *emit, const slk_shard_lookup *lookup,
                              const slk_shard_lists *apply_lists, const slk_shard_results *apply) {
  int32_t rc = check_ready(ix, st, apply != nullptr);
  if (rc) return rc;
  if ((rc = check_one_id_column(ix))) return rc;
  if (!lane_path_ok(ix)) return fail(SLK_E_UNSUPPORTED, "splitter outside the fused kernel's range: use the staged calls");
  if ((apply_lists == nullptr) != (apply == nullptr)) return fail(SLK_E_INVALID, "apply_lists and apply must be given together");
  if (emit && (rc = check_lists(*emit, "emit"))) return rc;
  if (emit && emit->R && !emit->d_bases) return fail(SLK_E_INVALID, "emit: null argument");
  if (apply_lists && (rc = check_lists(*apply_lists, "apply"))) return rc;
  if (lookup && lookup->n && (!lookup->d_keys || !lookup->d_out_taxa)) return fail(SLK_E_INVALID, "lookup: null argument");
  if (apply) {
    if ((rc = check_thresholds(apply->thresholds, apply->C))) return rc;
    if (apply_lists->R && (!apply->d_taxa || !apply->d_out_taxon || !apply->d_out_classified)) return fail(SLK_E_INVALID, "apply: null argument");
    if (emit && emit->R && (apply_lists->d_span_meta == nullptr) != (emit->d_span_meta == nullptr))
      return fail(SLK_E_INVALID, "the batches of one step write hit lists or none does");
  }
  rc = set_device(ix);
  if (rc) return rc;
  const bool scans = emit && emit->R != 0;
  FusedArgs A{};
  ShardIO S{};
  A.P = ix->sp; A.status = st->d_status;
  if (emit) HIPCHK(hipMemsetAsync(emit->d_cursors, 0, ((size_t)emit->n_shards + 3) * sizeof(uint64_t), st->s));
  if (scans) {
    fill_emit(ix, st, *emit, A, S);
    HIPCHK(hipMemsetAsync(emit->d_defer, 0, emit->R * sizeof(int32_t), st->s));
  }
  uint64_t *draw = scans ? emit->d_cursors + emit->n_shards : nullptr;
  bool lookup_beside = false;
  if (lookup && lookup->n) {
    // The lookups ride in the scan, their 64-key batches dealt out to its tiles -- unless the scan is far too short for them (a
    // tile sends off about 2 / (w + 1) keys per base; a tile handed several times as many lookups as that would finish them alone,
    // at its end, with the rest of the part idle): then they run as a kernel of their own, like those of a step without a scan.
    const uint64_t tiles = scans ? (emit->R + 63) / 64 : 0, batches = (lookup->n + 63) / 64;
    const double own = scans ? 2.0 / (ix->sp.w + 1) * (double)(emit->total_bases + emit->total_mate_bases) / 64.0 / (double)tiles : 0;
    const uint64_t per_tile = scans ? (batches + tiles - 1) / tiles : 0;
    if (scans && (double)per_tile <= 3.0 * own + 8.0) {
      S.side_keys = lookup->d_keys; S.side_n = lookup->n; S.side_out = lookup->d_out_taxa;
      S.side_per_tile = (uint32_t)per_tile;
    } else {
      // (beside the step's kernel when there is one -- the replay of a step without a scan, the pipeline's drain: the replay waits
      //  for two dependent loads per row, the lookups for the table; on one stream they took 2.1 + 9.6 ms, side by side ~10)
      const bool beside = scans || (apply && apply_lists->R != 0);
      if (beside) {
        rc = fork_ready(st);
        if (rc) return rc;
        HIPCHK(hipEventRecord(st->ev_fork, st->s));
        HIPCHK(hipStreamWaitEvent(st->s2, st->ev_fork, 0));
      }
      launch_lookup_coop(ix->view(), lookup->d_keys, lookup->n, lookup->d_out_taxa, beside ? st->s2 : st->s);
      HIPCHK(hipGetLastError());
      if (beside) { HIPCHK(hipEventRecord(st->ev_join, st->s2)); lookup_beside = true; }
    }
  }
  ApplyJob J{};
  const bool applies = apply && apply_lists->R != 0;
  if (applies) {
    const Thresholds thr = thresholds_of(apply->thresholds, apply->C);
    FusedArgs &B = J.A;
    B = fused_args(ix, st, {nullptr, apply_lists->d_offsets, nullptr, apply_lists->d_mate_offsets, apply_lists->R});
    B.out_stride = apply_lists->R;
    B.min_hit_groups = apply->min_hit_groups; B.thr = thr; B.C = apply->C;
    B.out_taxon = apply->d_out_taxon; B.out_classified = apply->d_out_classified; B.out_nd = apply->d_out_num_distinct;
    B.out_tk = apply->d_out_total_kmers; B.out_nh = apply->d_out_num_hits;
    B.span_meta = apply_lists->d_span_meta; B.span_taxon = apply_lists->d_span_taxon; B.span_count = apply_lists->d_span_count;
    J.n_shards = (int32_t)apply_lists->n_shards; J.cap = apply_lists->capacity_per_owner;
    J.send_meta = apply_lists->d_send_meta; J.batch_log = (const uint4 *)apply_lists->d_batch_log;
    J.tile_rows = (const uint2 *)apply_lists->d_tile_rows; J.read_info = (const int2 *)apply_lists->d_read_info;
    J.taxa = apply->d_taxa; J.to_dense = ix->d_to_dense; J.n_to_dense = ix->T; J.defer = apply_lists->d_defer;
    J.n_deferred = (unsigned long long *)(apply_lists->d_cursors + apply_lists->n_shards + 2);
    if (!scans) {   // a step without a scan: the replay's waves draw their tiles from a counter of its own (the batch's spare word)
      draw = apply_lists->d_cursors + apply_lists->n_shards + 1;
      HIPCHK(hipMemsetAsync(draw, 0, sizeof(uint64_t), st->s));
      S.n_shards = 0;
    }
  }
  if (scans || applies) {
    // (S.cursors[S.n_shards] is the tile draw: with a scan the batch's own word behind its cursors, else the word chosen above)
    if (!scans) S.cursors = (unsigned long long *)draw;
    st->queued.emplace_back();   // (not re-runnable: a map overflow of the replay defers the fragment, a full region is an error)
    launch_lane_step(A, S, J, scans ? emit->d_defer : nullptr, 1000, st->s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_status, st->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st->s));
  }
  if (lookup_beside) HIPCHK(hipStreamWaitEvent(st->s, st->ev_join, 0));
  return SLK_OK;
}

int32_t slk_classify_hits_device(slk_index *ix, slk_stream *st, const uint64_t *d_offsets,
                                 const uint64_t *d_mate_offsets, uint64_t R, const int32_t *d_span_meta,
                                 const int32_t *d_span_taxon, const int32_t *d_span_count, uint64_t *d_scratch,
                                 int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *d_out_taxon,
                                 uint8_t *d_out_classified, int32_t *d_out_num_distinct, int32_t *d_out_total_kmers,
                                 int32_t *d_out_num_hits) {
  int32_t rc = check_ready(ix, st, true);
  if (rc) return rc;
  if ((rc = check_one_id_column(ix))) return rc;
  if ((rc = check_thresholds(thresholds, C))) return rc;
  if (R && (!d_offsets || !d_span_meta || !d_span_taxon || !d_span_count || !d_scratch || !d_out_taxon || !d_out_classified))
    return fail(SLK_E_INVALID, "null argument");
  rc = set_device(ix);
  if (rc) return rc;
  ClassifyCall c;
  c.in.offsets = d_offsets; c.in.mate_offsets = d_mate_offsets; c.in.R = R;
  c.out = {d_out_taxon, d_out_classified, d_out_num_distinct, d_out_total_kmers, d_out_num_hits, nullptr, R};
  c.thr = thresholds_of(thresholds, C); c.C = C; c.min_hit_groups = min_hit_groups;
  launch_classify(ix->d_parents, ix->d_nodes_orig, ix->T, c, d_span_meta, d_span_taxon, d_span_count, d_scratch, st->s);
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

int32_t slk::ensure_outputs(slk_stream *st, uint64_t R, int32_t C) {
  HIPCHK(st->out_taxon.ensure((size_t)C * R * 4));
  HIPCHK(st->out_cls.ensure((size_t)C * R));
  HIPCHK(st->out_nd.ensure(R * 4));
  HIPCHK(st->out_tk.ensure(R * 4));
  HIPCHK(st->out_nh.ensure(R * 4));
  return SLK_OK;
}

// the result rows to the caller's memory (complete on return)
int32_t slk::download_rows(slk_stream *st, const HostRows &out, uint64_t R, int32_t C) {
  int32_t rc = copy_out(st, out.taxon, st->out_taxon.p, (size_t)C * R * 4);
  if (!rc) rc = copy_out(st, out.classified, st->out_cls.p, (size_t)C * R);
  if (!rc && out.nd) rc = copy_out(st, out.nd, st->out_nd.p, R * 4);
  if (!rc && out.tk) rc = copy_out(st, out.tk, st->out_tk.p, R * 4);
  return rc;
}

// Classifier.classify (object, Classifier.scala:439-454) for hit lists the caller assembled itself: the host merges the
// hits of fragments that share a title (groupBy("seqTitle"), Classifier.scala:92, then sorted by ordinal :136) and has the
// merged lists classified here.  Host pointers; synchronous.
int32_t slk_classify_hits(slk_index *ix, slk_stream *st, uint64_t R, const uint64_t *hit_offsets, const slk_hit *hits,
                          const uint8_t *distinct, int32_t min_hit_groups, const double *thresholds, int32_t C,
                          int32_t *out_taxon, uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers) {
  int32_t rc = check_ready(ix, st, true);
  if (rc) return rc;
  if ((rc = check_thresholds(thresholds, C))) return rc;
  if (!hit_offsets || (R && (!out_taxon || !out_classified))) return fail(SLK_E_INVALID, "null argument");
  for (uint64_t r = 0; r < R; r++)
    if (hit_offsets[r + 1] < hit_offsets[r] || hit_offsets[r + 1] - hit_offsets[r] > 0x7fffffffULL)
      return fail(SLK_E_INVALID, "hit_offsets must be non-decreasing (read %llu)", (unsigned long long)r);
  const uint64_t n = R ? hit_offsets[R] - hit_offsets[0] : 0;
  if (n && !hits) return fail(SLK_E_INVALID, "null argument");
  rc = set_device(ix);
  if (rc) return rc;
  if (R == 0) return SLK_OK;
  // the staged classify kernel's input: one slot per hit (fragment r's slots start at offsets[r]), meta = kmers|flag|distinct
  const uint64_t h0 = hit_offsets[0];
  std::vector<uint64_t> offs(R + 1);
  std::vector<int32_t> meta(n + 1), taxon(n + 1), count(R);
  for (uint64_t r = 0; r <= R; r++) offs[r] = hit_offsets[r] - h0;
  for (uint64_t r = 0; r < R; r++) count[r] = (int32_t)(offs[r + 1] - offs[r]);
  for (uint64_t i = 0; i < n; i++) {
    const slk_hit &h = hits[h0 + i];
    const int32_t flag = h.taxon == SLK_TAXON_AMBIGUOUS ? SLK_FLAG_AMBIGUOUS : h.taxon == SLK_TAXON_MATE_PAIR_BORDER ? SLK_FLAG_MATE_PAIR_BORDER : SLK_FLAG_SEQUENCE;
    if (h.taxon < SLK_TAXON_MATE_PAIR_BORDER) return fail(SLK_E_INVALID, "hit %llu: taxon %d", (unsigned long long)i, h.taxon);
    meta[i] = pack_meta(h.count, flag, (flag == SLK_FLAG_SEQUENCE && distinct && distinct[h0 + i]) ? 1 : 0);
    taxon[i] = h.taxon;
  }
  HIPCHK(st->offsets.ensure((R + 1) * 8));
  HIPCHK(st->span_meta.ensure((n + 1) * 4));
  HIPCHK(st->span_taxon.ensure((n + 1) * 4));
  HIPCHK(st->span_count.ensure((R + 1) * 4));
  HIPCHK(st->span_keys.ensure((n + 1) * 8));
  HIPCHK(st->out_taxon.ensure((size_t)C * R * 4));
  HIPCHK(st->out_cls.ensure((size_t)C * R));
  HIPCHK(st->out_nd.ensure(R * 4));
  HIPCHK(st->out_tk.ensure(R * 4));
  DrainOnExit drain(st);
  rc = copy_in(st, st->offsets.p, offs.data(), (R + 1) * 8);
  if (!rc) rc = copy_in(st, st->span_meta.p, meta.data(), (n + 1) * 4);
  if (!rc) rc = copy_in(st, st->span_taxon.p, taxon.data(), (n + 1) * 4);
  if (!rc) rc = copy_in(st, st->span_count.p, count.data(), R * 4);
  if (rc) return rc;
  ClassifyCall c;
  c.in.offsets = st->offsets.as<uint64_t>(); c.in.R = R;
  c.out = {st->out_taxon.as<int32_t>(), st->out_cls.as<uint8_t>(), st->out_nd.as<int32_t>(), st->out_tk.as<int32_t>(), nullptr, nullptr, R};
  c.thr = thresholds_of(thresholds, C); c.C = C; c.min_hit_groups = min_hit_groups;
  launch_classify(ix->d_parents, ix->d_nodes_orig, ix->T, c, st->span_meta.as<int32_t>(), st->span_taxon.as<int32_t>(),
                  st->span_count.as<int32_t>(), st->span_keys.as<uint64_t>(), st->s);
  HIPCHK(hipGetLastError());
  rc = download_rows(st, {out_taxon, out_classified, out_num_distinct, out_total_kmers}, R, C);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st->s));
  return SLK_OK;
}

int32_t slk_stream_last_deferred(slk_stream *st, uint64_t *out_count) {
  if (!st || !out_count) return fail(SLK_E_INVALID, "null argument");
  { int32_t rc_ = set_device(st->ix); if (rc_) return rc_; }
  *out_count = 0;
  HIPCHK(hipStreamSynchronize(st->s));
  if (st->defer_list.p && st->last_used_lane)   // (word 9 of the hand-on header: what the first pass handed on)
    HIPCHK(hipMemcpy(out_count, (const uint64_t *)st->defer_list.p + HandOn::HANDED, sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SLK_OK;
}

int32_t slk_stream_set_split_long(slk_stream *st, int64_t min_len) {
  if (!st) return fail(SLK_E_INVALID, "null handle");
  if (min_len < -1) return fail(SLK_E_INVALID, "min_len %lld: -1 (the engine's default), 0 (off) or a number of bases", (long long)min_len);
  st->split_long = min_len;
  return SLK_OK;
}

int32_t slk_stream_set_split_hits(slk_stream *st, int32_t on) {
  if (!st) return fail(SLK_E_INVALID, "null handle");
  st->split_hits = on != 0;
  return SLK_OK;
}

int32_t slk_stream_last_split(slk_stream *st, uint64_t *fragments, uint64_t *pieces, uint64_t *spills) {
  if (!st || !fragments || !pieces || !spills) return fail(SLK_E_INVALID, "null argument");
  { int32_t rc_ = set_device(st->ix); if (rc_) return rc_; }
  *fragments = *pieces = *spills = 0;
  HIPCHK(hipStreamSynchronize(st->s));
  if (st->piece_scratch.p && st->last_used_pieces) {
    uint64_t hdr[PieceHdr::WORDS];
    HIPCHK(hipMemcpy(hdr, st->piece_scratch.p, sizeof(hdr), hipMemcpyDeviceToHost));
    *fragments = hdr[PieceHdr::N_FRAG]; *pieces = hdr[PieceHdr::N_UNIT]; *spills = hdr[PieceHdr::SPILLS];
  }
  return SLK_OK;
}

int32_t slk_stream_split_info(slk_stream *st, uint64_t *grid_waves, uint64_t *scratch_bytes) {
  if (!st || !grid_waves || !scratch_bytes) return fail(SLK_E_INVALID, "null argument");
  *grid_waves = (uint64_t)PIECE_GRID_BLOCKS * 4;
  *scratch_bytes = st->piece_scratch.cap + st->piece_maps.cap + st->piece_hits.cap;
  return SLK_OK;
}

int32_t slk_stream_last_stage_ms(slk_stream *st, float out_ms[3]) {
  if (!st || !out_ms) return fail(SLK_E_INVALID, "null argument");
  if (!st->timed) return fail(SLK_E_STATE, "no classify call has been issued on this stream");
  { int32_t rc_ = set_device(st->ix); if (rc_) return rc_; }
  HIPCHK(hipEventSynchronize(st->ev[3]));
  HIPCHK(hipEventElapsedTime(&out_ms[0], st->ev[0], st->ev[1]));
  HIPCHK(hipEventElapsedTime(&out_ms[1], st->ev[1], st->ev[2]));
  HIPCHK(hipEventElapsedTime(&out_ms[2], st->ev[2], st->ev[3]));
  return SLK_OK;
}

int32_t slk::validate_reads(const uint64_t *offsets, const uint64_t *mate_offsets, uint64_t R) {
  // (4 M reads are 4 M compares per array: split over the copy threads)
  const uint64_t PART = 1 << 18;
  const uint64_t parts = (R + PART - 1) / PART;
  std::vector<uint64_t> bad(parts, ~0ULL);
  host_pool().parallel_for(parts, [&](size_t pi) {
    const uint64_t r1 = std::min<uint64_t>(R, (pi + 1) * PART);
    for (uint64_t r = pi * PART; r < r1; r++) {
      const bool ok = offsets[r + 1] >= offsets[r] && offsets[r + 1] - offsets[r] <= 0x7fffffffULL &&
                      (!mate_offsets || (mate_offsets[r + 1] >= mate_offsets[r] && mate_offsets[r + 1] - mate_offsets[r] <= 0x7fffffffULL));
      if (!ok) { bad[pi] = r; break; }
    }
  });
  for (uint64_t b : bad)
    if (b != ~0ULL)
      return fail(SLK_E_INVALID, "offsets (and mate_offsets) must be non-decreasing with reads shorter than 2^31 (read %llu)", (unsigned long long)b);
  return SLK_OK;
}

int32_t slk::upload_reads(slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const uint8_t *mate_bases,
                          const uint64_t *mate_offsets, uint64_t R, uint64_t *total, uint64_t *mate_total) {
  int32_t rc = validate_reads(offsets, mate_offsets, R);
  if (rc) return rc;
  *total = offsets[R];
  *mate_total = mate_offsets ? mate_offsets[R] : 0;
  HIPCHK(st->bases.ensure(*total));
  HIPCHK(st->offsets.ensure((R + 1) * 8));
  rc = copy_in(st, st->bases.p, bases, *total);
  if (!rc) rc = copy_in(st, st->offsets.p, offsets, (R + 1) * 8);
  if (rc) return rc;
  if (mate_offsets) {
    HIPCHK(st->mate_bases.ensure(*mate_total));
    HIPCHK(st->mate_offsets.ensure((R + 1) * 8));
    rc = copy_in(st, st->mate_bases.p, mate_bases, *mate_total);
    if (!rc) rc = copy_in(st, st->mate_offsets.p, mate_offsets, (R + 1) * 8);
    if (rc) return rc;
  }
  return SLK_OK;
}

// counts (device, int32[R]) -> out_offsets (host, u64[R+1]); uploads the offsets for a gather kernel
int32_t slk::counts_to_offsets(slk_stream *st, const int32_t *d_counts, uint64_t R, uint64_t *out_offsets, uint64_t capacity) {
  out_offsets[0] = 0;
  if (R == 0) return SLK_OK;
  DrainOnExit drain(st);
  HIPCHK(st->out_offsets.ensure((R + 1) * 8));
  HIPCHK(st->scan_tmp.ensure((R / 2048 + 2) * 8));
  launch_counts_to_offsets(d_counts, R, st->out_offsets.as<uint64_t>(), st->scan_tmp.as<uint64_t>(), st->s);   // (kernels.hip)
  HIPCHK(hipGetLastError());
  int32_t rc = copy_out(st, out_offsets, st->out_offsets.p, (R + 1) * 8);
  if (rc) return rc;
  if (out_offsets[R] > capacity)
    return fail(SLK_E_CAPACITY, "output needs %llu entries, capacity is %llu", (unsigned long long)out_offsets[R],
                (unsigned long long)capacity);
  return SLK_OK;
}

// slk_spans_batch / slk_spans_batch_wide: out_keys (nullable) receives the spans' id1..idW rows
static int32_t spans_batch(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const uint8_t *mate_bases,
                           const uint64_t *mate_offsets, uint64_t R, uint64_t *out_span_offsets, slk_span *out_spans, int64_t *out_keys,
                           uint64_t spans_capacity) {
  int32_t rc = check_ready(ix, st, false);
  if (rc) return rc;
  if (ix->W > 1 && !out_keys) return fail(SLK_E_UNSUPPORTED, "slk_spans_batch returns one key word per span: minimizers of up to 32 nt (one id column); use slk_spans_batch_wide");
  if (!offsets || !out_span_offsets || (R && !bases)) return fail(SLK_E_INVALID, "null argument");
  if ((rc = check_mates(mate_bases, mate_offsets))) return rc;
  rc = set_device(ix);
  if (rc) return rc;
  out_span_offsets[0] = 0;
  if (R == 0) return SLK_OK;
  uint64_t total, mate_total;
  DrainOnExit drain(st);
  rc = upload_reads(st, bases, offsets, mate_bases, mate_offsets, R, &total, &mate_total);
  if (rc) return rc;
  bool paired = mate_offsets != nullptr;
  rc = ensure_scratch(st, span_slots(total, mate_total, R, paired), R);
  if (rc) return rc;
  const uint64_t *d_off = st->offsets.as<uint64_t>();
  const uint64_t *d_moff = paired ? st->mate_offsets.as<uint64_t>() : nullptr;
  const uint8_t *d_mate = paired ? st->mate_bases.as<uint8_t>() : nullptr;
  launch_spans(ix, st, {st->bases.as<uint8_t>(), d_off, d_mate, d_moff, R}, st->span_keys.as<uint64_t>(), st->span_meta.as<int32_t>(),
               st->span_count.as<int32_t>());
  HIPCHK(hipGetLastError());
  rc = counts_to_offsets(st, st->span_count.as<int32_t>(), R, out_span_offsets, spans_capacity);
  if (rc) return rc;
  uint64_t n = out_span_offsets[R];
  if (n) {
    if (!out_spans) return fail(SLK_E_INVALID, "out_spans is null");
    HIPCHK(st->out_items.ensure(n * sizeof(slk_span)));
    if (ix->W > 1) {
      HIPCHK(st->out_taxon.ensure(n * 8 * ix->W));   // (free here: this entry classifies nothing)
      launch_wide_gather_spans(ix->W, d_off, d_moff, R, st->span_keys.as<uint64_t>(), st->span_meta.as<int32_t>(), st->out_offsets.as<uint64_t>(),
                               st->out_items.p, st->out_taxon.as<int64_t>(), st->s);
    } else {
      launch_gather_spans(d_off, d_moff, R, st->span_keys.as<uint64_t>(), st->span_meta.as<int32_t>(),
                          st->out_offsets.as<uint64_t>(), st->out_items.p, st->s);
    }
    HIPCHK(hipGetLastError());
    rc = copy_out(st, out_spans, st->out_items.p, n * sizeof(slk_span));
    if (!rc && ix->W > 1) rc = copy_out(st, out_keys, st->out_taxon.p, n * 8 * ix->W);
    if (rc) return rc;
    if (ix->W == 1 && out_keys)
      for (uint64_t i = 0; i < n; i++) out_keys[i] = out_spans[i].key;
  }
  HIPCHK(hipStreamSynchronize(st->s));
  return SLK_OK;
}

int32_t slk_spans_batch(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets,
                        const uint8_t *mate_bases, const uint64_t *mate_offsets, uint64_t R,
                        uint64_t *out_span_offsets, slk_span *out_spans, uint64_t spans_capacity) {
  return spans_batch(ix, st, bases, offsets, mate_bases, mate_offsets, R, out_span_offsets, out_spans, nullptr, spans_capacity);
}

int32_t slk_spans_batch_wide(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets,
                             const uint8_t *mate_bases, const uint64_t *mate_offsets, uint64_t R,
                             uint64_t *out_span_offsets, slk_span *out_spans, int64_t *out_keys, uint64_t spans_capacity) {
  if (!out_keys && spans_capacity) return fail(SLK_E_INVALID, "out_keys is null");
  return spans_batch(ix, st, bases, offsets, mate_bases, mate_offsets, R, out_span_offsets, out_spans, out_keys, spans_capacity);
}

// The reads of a host call: ASCII (bases / mate_bases) or the engine's 3-bit form (host/pack.hpp: 2-bit codes and validity bits,
// 16 bases per word, positions as in the ASCII concatenation).  Packed reads are unpacked on the device, behind their upload, into
// the stream's ASCII buffers -- 6 bytes over the link per 16 bases instead of 16 --, so every kernel of the path reads them as it
// reads text.
struct ReadSource {
  const uint8_t *bases = nullptr, *mate_bases = nullptr;
  const uint32_t *codes = nullptr, *mate_codes = nullptr;
  const uint16_t *valid = nullptr, *mate_valid = nullptr;
  bool packed() const { return codes != nullptr; }
};

// bases [p0, p1) of one mate from the caller's memory to dst (+ the device-side unpack on `run` for packed reads), ordered on `up`
int32_t slk::upload_range(slk_stream *st, Staging *g, hipStream_t up, hipStream_t run, hipEvent_t ev, bool packed, const uint8_t *bases,
                            const uint32_t *codes, const uint16_t *valid, DevBuf &d_codes, DevBuf &d_valid, uint8_t *dst, uint64_t p0, uint64_t p1) {
  if (p1 <= p0) return SLK_OK;
  if (!packed) return copy_in(g, up, dst + p0, bases + p0, p1 - p0);
  const uint64_t w0 = p0 / 16, w1 = (p1 + 15) / 16;
  int32_t rc = copy_in(g, up, d_codes.as<uint32_t>() + w0, codes + w0, (w1 - w0) * 4);
  if (!rc) rc = copy_in(g, up, d_valid.as<uint16_t>() + w0, valid + w0, (w1 - w0) * 2);
  if (rc) return rc;
  if (up != run) {
    HIPCHK(hipEventRecord(ev, up));
    HIPCHK(hipStreamWaitEvent(run, ev, 0));
  }
  // (whole words: a word that straddles two ranges is unpacked by both, to the same bytes, in stream order)
  launch_unpack_bases(d_codes.as<uint32_t>(), d_valid.as<uint16_t>(), w0, w1, dst, run);
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

// Fragments [r0, r1) of a host call as a call of their own (h_offsets / h_mate_offsets: the caller's arrays).  The offsets stay
// ABSOLUTE, so "total bases" is where the sub-batch ENDS: it sizes the span scratch of the unbounded re-run, whose regions are
// addressed by those offsets.  Hit lists: the fragments' span regions are addressed by their absolute offsets but by the fragment's
// number INSIDE the sub-batch (span_region: offsets[r] + mate_offsets[r] + r for pairs), so the span arrays are handed over moved by
// the sub-batch's first fragment number -- the regions then are the ones the whole batch has, and sub-batches do not overlap.  The
// caller has sized the scratch for the whole batch; the result rows keep the whole batch's stride.
static ClassifyCall sub_call(const ClassifyCall &whole, uint64_t r0, uint64_t r1, const uint64_t *h_offsets, const uint64_t *h_mate_offsets) {
  ClassifyCall c = whole;
  const bool paired = whole.in.paired();
  c.in.offsets += r0;
  c.h_offsets = h_offsets + r0;
  if (paired) c.in.mate_offsets += r0;
  c.in.R = r1 - r0; c.in.total = h_offsets[r1]; c.in.mate_total = paired ? h_mate_offsets[r1] : 0;
  c.out.taxon += r0; c.out.classified += r0; c.out.nd += r0; c.out.tk += r0; c.out.nh += r0;
  c.span_shift = whole.want_hits && paired ? r0 : 0;
  return c;
}

static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the stream's buffers at their sizes for a call of R fragments: result rows, reads, and the packed reads as they arrive
int32_t slk::size_host_buffers(slk_stream *st, uint64_t R, int32_t C, uint64_t total, uint64_t mate_total, bool paired, bool pk) {
  const int32_t rc = ensure_outputs(st, R, C);
  if (rc) return rc;
  // (packed reads are unpacked in whole words of 16 bases: the ASCII buffers hold the last word in full)
  HIPCHK(st->bases.ensure((total + 15) / 16 * 16));
  HIPCHK(st->offsets.ensure((R + 1) * 8));
  if (paired) {
    HIPCHK(st->mate_bases.ensure((mate_total + 15) / 16 * 16));
    HIPCHK(st->mate_offsets.ensure((R + 1) * 8));
  }
  if (pk) {
    HIPCHK(st->pk_codes.ensure((total + 15) / 16 * 4 + 4));
    HIPCHK(st->pk_valid.ensure((total + 15) / 16 * 2 + 2));
    if (paired) {
      HIPCHK(st->pk_mate_codes.ensure((mate_total + 15) / 16 * 4 + 4));
      HIPCHK(st->pk_mate_valid.ensure((mate_total + 15) / 16 * 2 + 2));
    }
    if (!st->ev_unpack) HIPCHK(hipEventCreateWithFlags(st->ev_unpack.put(), hipEventDisableTiming));
  }
  return SLK_OK;
}

// A large call is cut into sub-batches: the reads of sub-batch i+1 go up (on a second stream) while the kernels of
// sub-batch i run, so the call costs its upload plus ONE sub-batch of kernel time.  With hit lists too: the sub-batches leave
// their spans in the batch's span arrays (sub_call: span_shift) and the lists are put together for the whole batch at the end.
// *early_down: the result rows came down beside the kernels (below).
static int32_t run_sub_batches(slk_index *ix, slk_stream *st, const ReadSource &src, const uint64_t *offsets, const uint64_t *mate_offsets,
                               const ClassifyCall &whole, uint64_t SUB, const HostRows &out, bool *early_down) {
  const uint64_t R = whole.in.R;
  const bool paired = whole.in.paired(), pk = src.packed();
  int32_t rc, C = whole.C;
  if (whole.want_hits) {   // (once, for the whole batch: a sub-batch must not move the arrays under the kernels of the one before)
    rc = ensure_scratch(st, span_slots(whole.in.total, whole.in.mate_total, R, paired), R);
    if (rc) return rc;
  }
  if (!st->cs) HIPCHK(hipStreamCreateWithFlags(st->cs.put(), hipStreamNonBlocking));
  if (!st->ds) HIPCHK(hipStreamCreateWithFlags(st->ds.put(), hipStreamNonBlocking));
  const uint64_t nsub = (R + SUB - 1) / SUB;
  for (std::vector<Event> *evs : {&st->up_ev, &st->dn_ev})
    while (evs->size() < nsub) {
      Event e;
      HIPCHK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
      evs->push_back(std::move(e));
    }
  // Result buffers the library can DMA into take their rows sub-batch by sub-batch, beside the next sub-batch's kernels (the link
  // is full duplex: the rows come down while the reads go up); pageable ones are filled at the end, through the staging buffers.
  *early_down = pinned().covers(out.taxon, (size_t)C * R * 4) && pinned().covers(out.classified, (size_t)C * R) &&
                (!out.nd || pinned().covers(out.nd, R * 4)) && (!out.tk || pinned().covers(out.tk, R * 4));
  st->reran = false;
  for (uint64_t i = 0; i < nsub; i++) {
    const uint64_t r0 = i * SUB, r1 = std::min(R, r0 + SUB), n = r1 - r0;
    // (the offsets travel with their sub-batch: 8 bytes per read are a tenth of a packed batch, and the first kernels should not
    //  wait for all of them)
    rc = copy_in(&st->staging_c, st->cs, st->offsets.as<uint64_t>() + r0, offsets + r0, (n + 1) * 8);
    if (!rc && paired) rc = copy_in(&st->staging_c, st->cs, st->mate_offsets.as<uint64_t>() + r0, mate_offsets + r0, (n + 1) * 8);
    if (rc) return rc;
    rc = upload_range(st, &st->staging_c, st->cs, st->s, st->ev_unpack, pk, src.bases, src.codes, src.valid, st->pk_codes, st->pk_valid,
                      st->bases.as<uint8_t>(), offsets[r0], offsets[r1]);
    if (!rc && paired)
      rc = upload_range(st, &st->staging_c, st->cs, st->s, st->ev_unpack, pk, src.mate_bases, src.mate_codes, src.mate_valid, st->pk_mate_codes,
                        st->pk_mate_valid, st->mate_bases.as<uint8_t>(), mate_offsets[r0], mate_offsets[r1]);
    if (rc) return rc;
    HIPCHK(hipEventRecord(st->up_ev[i], st->cs));
    HIPCHK(hipStreamWaitEvent(st->s, st->up_ev[i], 0));
    rc = run_classify(ix, st, sub_call(whole, r0, r1, offsets, mate_offsets));
    if (rc) return rc;
    if (*early_down) {
      HIPCHK(hipEventRecord(st->dn_ev[i], st->s));
      HIPCHK(hipStreamWaitEvent(st->ds, st->dn_ev[i], 0));
      for (int32_t c = 0; c < C; c++) {
        HIPCHK(hipMemcpyAsync(out.taxon + (size_t)c * R + r0, st->out_taxon.as<int32_t>() + (size_t)c * R + r0, n * 4, hipMemcpyDeviceToHost, st->ds));
        HIPCHK(hipMemcpyAsync(out.classified + (size_t)c * R + r0, st->out_cls.as<uint8_t>() + (size_t)c * R + r0, n, hipMemcpyDeviceToHost, st->ds));
      }
      if (out.nd) HIPCHK(hipMemcpyAsync(out.nd + r0, st->out_nd.as<int32_t>() + r0, n * 4, hipMemcpyDeviceToHost, st->ds));
      if (out.tk) HIPCHK(hipMemcpyAsync(out.tk + r0, st->out_tk.as<int32_t>() + r0, n * 4, hipMemcpyDeviceToHost, st->ds));
    }
  }
  HIPCHK(hipStreamSynchronize(st->cs));  // (the caller's buffers are free from here on)
  return SLK_OK;
}

// the reads of a call that is not cut up: everything on the stream of the kernels
static int32_t upload_whole(slk_stream *st, const ReadSource &src, const uint64_t *offsets, const uint64_t *mate_offsets, const Reads &in) {
  const bool pk = src.packed();
  int32_t rc = upload_range(st, &st->staging, st->s, st->s, st->ev_unpack, pk, src.bases, src.codes, src.valid, st->pk_codes, st->pk_valid,
                            st->bases.as<uint8_t>(), 0, in.total);
  if (!rc) rc = copy_in(st, st->offsets.p, offsets, (in.R + 1) * 8);
  if (!rc && in.paired()) {
    rc = upload_range(st, &st->staging, st->s, st->s, st->ev_unpack, pk, src.mate_bases, src.mate_codes, src.mate_valid, st->pk_mate_codes,
                      st->pk_mate_valid, st->mate_bases.as<uint8_t>(), 0, in.mate_total);
    if (!rc) rc = copy_in(st, st->mate_offsets.p, mate_offsets, (in.R + 1) * 8);
  }
  return rc;
}

// The hit lists of a batch whose kernels are through: their offsets, then (out_hits given) the lists themselves, as the spans lie or
// merged (slk_stream_set_merged_hits).  th (call timing only): when the offsets, the gather and the download were through.
int32_t slk::assemble_hits(slk_stream *st, const Reads &in, bool want_hits, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity,
                             bool call_timing, double th[3]) {
  const uint64_t R = in.R;
  const bool merged = st->merged_hits && want_hits;
  if (merged) {   // (the merged lists' lengths first: span_count is free once the kernels are through)
    launch_merged_hits(true, in.offsets, in.mate_offsets, R, st->span_meta.as<int32_t>(), st->span_taxon.as<int32_t>(), st->out_nh.as<int32_t>(), nullptr,
                       st->span_count.as<int32_t>(), nullptr, st->s);
    HIPCHK(hipGetLastError());
  }
  int32_t rc = counts_to_offsets(st, merged ? st->span_count.as<int32_t>() : st->out_nh.as<int32_t>(), R, out_hit_offsets, out_hits ? hits_capacity : ~0ULL);
  if (rc) return rc;
  if (call_timing) th[0] = now();
  uint64_t n = out_hit_offsets[R];
  if (n && out_hits) {
    HIPCHK(st->out_items.ensure(n * sizeof(slk_hit)));
    if (merged)
      launch_merged_hits(false, in.offsets, in.mate_offsets, R, st->span_meta.as<int32_t>(), st->span_taxon.as<int32_t>(), st->out_nh.as<int32_t>(),
                         st->out_offsets.as<uint64_t>(), nullptr, st->out_items.p, st->s);
    else
      launch_gather_hits(in.offsets, in.mate_offsets, R, st->span_meta.as<int32_t>(), st->span_taxon.as<int32_t>(),
                         st->out_offsets.as<uint64_t>(), st->out_items.p, st->s);
    HIPCHK(hipGetLastError());
    if (call_timing) { (void)hipStreamSynchronize(st->s); th[1] = now(); }
    rc = copy_out(st, out_hits, st->out_items.p, n * sizeof(slk_hit));
    if (rc) return rc;
    if (call_timing) th[2] = now();
  }
  return SLK_OK;
}

static int32_t classify_batch_host(slk_index *ix, slk_stream *st, const ReadSource &src, const uint64_t *offsets, const uint64_t *mate_offsets,
                                   uint64_t R, int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon,
                                   uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers, uint64_t *out_hit_offsets,
                                   slk_hit *out_hits, uint64_t hits_capacity) {
  int32_t rc = check_ready(ix, st, true);
  if (rc) return rc;
  const bool pk = src.packed();
  if (!offsets || (R && ((!pk && !src.bases) || (pk && !src.valid) || !out_taxon || !out_classified))) return fail(SLK_E_INVALID, "null argument");
  if ((rc = check_thresholds(thresholds, C))) return rc;
  const bool paired = mate_offsets != nullptr;
  if (paired != (pk ? (src.mate_codes != nullptr && src.mate_valid != nullptr) : src.mate_bases != nullptr) ||
      (!paired && (src.mate_codes || src.mate_valid || src.mate_bases)))
    return fail(SLK_E_INVALID, "the second mates' bases and mate_offsets must be given together");
  rc = set_device(ix);
  if (rc) return rc;
  if (out_hit_offsets) out_hit_offsets[0] = 0;
  if (R == 0) return SLK_OK;
  static const bool call_timing = getenv("SLK_DEBUG_CALL_TIMING") != nullptr;  // tuning aid: wall clock of the phases of a call
  double tp[6] = {now(), 0, 0, 0, 0, 0};
  const bool want_hits = out_hit_offsets != nullptr && out_hits != nullptr;
  const HostRows out{out_taxon, out_classified, out_num_distinct, out_total_kmers};
  bool early_down = false;
  rc = validate_reads(offsets, mate_offsets, R);
  if (rc) return rc;
  const uint64_t total = offsets[R], mate_total = paired ? mate_offsets[R] : 0;
  rc = size_host_buffers(st, R, C, total, mate_total, paired, pk);
  if (rc) return rc;
  // (sub-batches of 2^19 reads: measured from pinned memory, 4 M reads of 150 bp -- packed 353 / 576 / 643 / 623 / 403 M reads/s at
  //  2^17 .. 2^21, text 313 / 324 / 327 / 315 / 246: smaller pieces pay per copy -- a sub-batch is five to nine DMAs --, larger ones
  //  leave the last piece's kernels exposed; profiles/r04_packed_entry.json.  Read per call, so that tests can move it.)
  const uint64_t SUB = (uint64_t)std::max(1L, env_long("SLK_HOST_SUBBATCH", 1L << 19));
  ClassifyCall whole;   // (every buffer it names has its size for this call by now)
  whole.in = {st->bases.as<uint8_t>(), st->offsets.as<uint64_t>(), paired ? st->mate_bases.as<uint8_t>() : nullptr,
              paired ? st->mate_offsets.as<uint64_t>() : nullptr, R, total, mate_total};
  whole.out = {st->out_taxon.as<int32_t>(), st->out_cls.as<uint8_t>(), st->out_nd.as<int32_t>(), st->out_tk.as<int32_t>(),
               st->out_nh.as<int32_t>(), nullptr, R};
  whole.thr = thresholds_of(thresholds, C); whole.C = C; whole.min_hit_groups = min_hit_groups; whole.want_hits = want_hits;
  whole.h_offsets = offsets;
  DrainOnExit drain(st);   // (from the first copy queued below, no return leaves work behind that touches the caller's memory)
  if (use_fused(ix) && R >= 2 * SUB) {
    rc = run_sub_batches(ix, st, src, offsets, mate_offsets, whole, SUB, out, &early_down);
    if (rc) return rc;
    if (call_timing) tp[1] = now();
  } else {
    rc = upload_whole(st, src, offsets, mate_offsets, whole.in);
    if (rc) return rc;
    if (call_timing) { (void)hipStreamSynchronize(st->s); tp[1] = now(); }
    rc = run_classify(ix, st, whole);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(st->s));
  tp[2] = now();
  rc = check_status(st);  // (re-runs the batch through the unbounded path if a taxon map overflowed)
  if (rc) return rc;
  if (early_down) HIPCHK(hipStreamSynchronize(st->ds));
  if (!early_down || st->reran) {   // (rows that came down early are stale if the batch was classified again)
    rc = download_rows(st, out, R, C);
    if (rc) return rc;
  }
  if (call_timing) { (void)hipStreamSynchronize(st->s); tp[3] = now(); }
  double th[3] = {0, 0, 0};
  if (out_hit_offsets) {
    rc = assemble_hits(st, whole.in, want_hits, out_hit_offsets, out_hits, hits_capacity, call_timing, th);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(st->s));
  if (call_timing)
    fprintf(stderr, "slk_classify_batch%s R=%llu: upload %.2f ms, kernels %.2f, results %.2f, hit lists %.2f (offsets %.2f, gather %.2f, download %.2f)\n",
            pk ? "_packed" : "", (unsigned long long)R, tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], now() - tp[3], th[0] ? th[0] - tp[3] : 0.0,
            th[1] ? th[1] - th[0] : 0.0, th[2] ? th[2] - th[1] : 0.0);
  return check_status(st);
}

int32_t slk_classify_batch(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets,
                           const uint8_t *mate_bases, const uint64_t *mate_offsets, uint64_t R,
                           int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon,
                           uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers,
                           uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity) {
  if (int32_t rc = check_mates(mate_bases, mate_offsets)) return rc;
  ReadSource src;
  src.bases = bases; src.mate_bases = mate_bases;
  return classify_batch_host(ix, st, src, offsets, mate_offsets, R, min_hit_groups, thresholds, C, out_taxon, out_classified, out_num_distinct,
                             out_total_kmers, out_hit_offsets, out_hits, hits_capacity);
}

// The same call with the reads in the engine's 3-bit form (host/pack.hpp; slk_pack_bases makes it): 6 bytes per 16 bases over the
// link instead of 16.  InputFragment.nucleotides (S/kmers/minimizer/MinSplitter.scala:31-32) already encoded as
// BitRepresentation.charToTwobit would (S/kmers/util/BitRepresentation.scala:127-135), with the isValid test (:140-143) as a bit.
int32_t slk_classify_batch_packed(slk_index *ix, slk_stream *st, const uint32_t *codes, const uint16_t *valid, const uint64_t *offsets,
                                  const uint32_t *mate_codes, const uint16_t *mate_valid, const uint64_t *mate_offsets, uint64_t R,
                                  int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon,
                                  uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers,
                                  uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity) {
  if (R && (!codes || !valid)) return fail(SLK_E_INVALID, "null argument");
  if ((mate_codes == nullptr) != (mate_offsets == nullptr) || (mate_valid == nullptr) != (mate_offsets == nullptr))
    return fail(SLK_E_INVALID, "mate_codes, mate_valid and mate_offsets must be given together");
  ReadSource src;
  src.codes = codes; src.valid = valid; src.mate_codes = mate_codes; src.mate_valid = mate_valid;
  if (R == 0) { static const uint32_t z = 0; src.codes = &z; }   // (an empty batch is a packed one all the same)
  return classify_batch_host(ix, st, src, offsets, mate_offsets, R, min_hit_groups, thresholds, C, out_taxon, out_classified, out_num_distinct,
                             out_total_kmers, out_hit_offsets, out_hits, hits_capacity);
}

// slk_classify_batch with the reads still FASTA / FASTQ text: the text goes up as it is, textparse.hip finds the records and leaves
// them in the stream's read buffers in the layout the kernels take, and the batch goes the way of slk_classify_batch_device from
// there.  What comes back beside the results is where every record's sequence and title lie.
int32_t slk_classify_text(slk_index *ix, slk_stream *st, const uint8_t *text, uint64_t n, int32_t format, int32_t final,
                          int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon, uint8_t *out_classified,
                          int32_t *out_num_distinct, int32_t *out_total_kmers, uint64_t *out_offsets, uint64_t *out_title_pos,
                          uint32_t *out_title_len, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t records_capacity,
                          uint64_t hits_capacity, uint64_t *out_records, uint64_t *out_consumed) {
  int32_t rc = check_ready(ix, st, true);
  if (rc) return rc;
  if (!out_records || !out_consumed || !out_offsets || (n && !text) ||
      (records_capacity && (!out_taxon || !out_classified || !out_title_pos || !out_title_len)))
    return fail(SLK_E_INVALID, "null argument");
  *out_records = *out_consumed = 0;
  if ((rc = check_thresholds(thresholds, C))) return rc;
  if ((rc = check_parse_args(n, format))) return rc;
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "slk_classify_text supports minimizers of up to 32 nt (one id column)");
  rc = set_device(ix);
  if (rc) return rc;
  out_offsets[0] = 0;
  if (out_hit_offsets) out_hit_offsets[0] = 0;
  DrainOnExit drain(st);
  uint64_t counts[4] = {0, 0, 0, 0};
  rc = parse_uploaded(st, text, n, format, final != 0, n, records_capacity, counts);   // (the sequences are fewer bytes than the text)
  const uint64_t R = counts[0], total = counts[1];
  *out_records = R;   // (with SLK_E_CAPACITY too: the records_capacity the text needs)
  if (rc) return rc;
  *out_consumed = counts[2];
  if (R == 0) return SLK_OK;
  rc = copy_out(st, out_offsets, st->offsets.p, (R + 1) * 8);
  if (!rc) rc = copy_out(st, out_title_pos, st->parse_title_pos.p, R * 8);
  if (!rc) rc = copy_out(st, out_title_len, st->parse_title_len.p, R * 4);
  if (!rc) rc = validate_reads(out_offsets, nullptr, R);
  if (!rc) rc = ensure_outputs(st, R, C);
  if (rc) return rc;
  const bool want_hits = out_hit_offsets != nullptr && out_hits != nullptr;
  ClassifyCall whole;
  whole.in = {st->bases.as<uint8_t>(), st->offsets.as<uint64_t>(), nullptr, nullptr, R, total, 0};
  whole.out = {st->out_taxon.as<int32_t>(), st->out_cls.as<uint8_t>(), st->out_nd.as<int32_t>(), st->out_tk.as<int32_t>(),
               st->out_nh.as<int32_t>(), nullptr, R};
  whole.thr = thresholds_of(thresholds, C); whole.C = C; whole.min_hit_groups = min_hit_groups; whole.want_hits = want_hits;
  whole.h_offsets = out_offsets;
  st->reran = false;
  rc = run_classify(ix, st, whole);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st->s));
  rc = check_status(st);  // (re-runs the batch through the unbounded path if a taxon map overflowed)
  if (rc) return rc;
  rc = download_rows(st, HostRows{out_taxon, out_classified, out_num_distinct, out_total_kmers}, R, C);
  if (rc) return rc;
  if (out_hit_offsets) {
    double th[3] = {0, 0, 0};
    rc = assemble_hits(st, whole.in, want_hits, out_hit_offsets, out_hits, hits_capacity, false, th);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(st->s));
  return check_status(st);
}

// slk_classify_text for two mate files: both texts go up, textparse.hip parses text 1 into the stream's read buffers and text 2 into
// its mate buffers and pairs them in lockstep; the first P records of either side are the batch (offsets[P] ends the reads of the
// pairs, so the arrays serve as they lie), classified with mates as slk_classify_batch_device would.
int32_t slk_classify_text_paired(slk_index *ix, slk_stream *st, const uint8_t *text1, uint64_t n1, int32_t format1, int32_t final1,
                                 const uint8_t *text2, uint64_t n2, int32_t format2, int32_t final2, int32_t min_hit_groups,
                                 const double *thresholds, int32_t C, int32_t *out_taxon, uint8_t *out_classified, int32_t *out_num_distinct,
                                 int32_t *out_total_kmers, uint64_t *out_offsets, uint64_t *out_mate_offsets, uint64_t *out_title_pos,
                                 uint32_t *out_title_len, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t records_capacity,
                                 uint64_t hits_capacity, slk_pair_record *out_pair) {
  int32_t rc = check_ready(ix, st, true);
  if (rc) return rc;
  if (!out_pair || !out_offsets || !out_mate_offsets || (n1 && !text1) || (n2 && !text2) ||
      (records_capacity && (!out_taxon || !out_classified || !out_title_pos || !out_title_len)))
    return fail(SLK_E_INVALID, "null argument");
  uint64_t pair[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(out_pair, pair, sizeof(pair));
  if ((rc = check_thresholds(thresholds, C))) return rc;
  if ((rc = check_parse_args(n1, format1))) return rc;
  if ((rc = check_parse_args(n2, format2))) return rc;
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "slk_classify_text_paired supports minimizers of up to 32 nt (one id column)");
  rc = set_device(ix);
  if (rc) return rc;
  out_offsets[0] = out_mate_offsets[0] = 0;
  if (out_hit_offsets) out_hit_offsets[0] = 0;
  DrainOnExit drain(st);
  rc = parse_pair_uploaded(st, PairText{text1, n1, format1, final1 != 0, n1, records_capacity},
                           PairText{text2, n2, format2, final2 != 0, n2, records_capacity}, pair);
  memcpy(out_pair, pair, sizeof(pair));   // (with SLK_E_CAPACITY too: the records_capacity the texts need)
  if (rc) return rc;
  const uint64_t P = pair[0], R1 = pair[4];
  rc = copy_out(st, out_title_pos, st->parse_title_pos.p, R1 * 8);
  if (!rc) rc = copy_out(st, out_title_len, st->parse_title_len.p, R1 * 4);
  if (rc) return rc;
  if (P == 0) return SLK_OK;
  rc = copy_out(st, out_offsets, st->offsets.p, (P + 1) * 8);
  if (!rc) rc = copy_out(st, out_mate_offsets, st->mate_offsets.p, (P + 1) * 8);
  if (!rc) rc = validate_reads(out_offsets, out_mate_offsets, P);
  if (!rc) rc = ensure_outputs(st, P, C);
  if (rc) return rc;
  const bool want_hits = out_hit_offsets != nullptr && out_hits != nullptr;
  ClassifyCall whole;
  whole.in = {st->bases.as<uint8_t>(), st->offsets.as<uint64_t>(), st->mate_bases.as<uint8_t>(), st->mate_offsets.as<uint64_t>(), P, pair[6], pair[7]};
  whole.out = {st->out_taxon.as<int32_t>(), st->out_cls.as<uint8_t>(), st->out_nd.as<int32_t>(), st->out_tk.as<int32_t>(),
               st->out_nh.as<int32_t>(), nullptr, P};
  whole.thr = thresholds_of(thresholds, C); whole.C = C; whole.min_hit_groups = min_hit_groups; whole.want_hits = want_hits;
  st->reran = false;
  rc = run_classify(ix, st, whole);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st->s));
  rc = check_status(st);  // (re-runs the batch through the unbounded path if a taxon map overflowed)
  if (rc) return rc;
  rc = download_rows(st, HostRows{out_taxon, out_classified, out_num_distinct, out_total_kmers}, P, C);
  if (rc) return rc;
  if (out_hit_offsets) {
    double th[3] = {0, 0, 0};
    rc = assemble_hits(st, whole.in, want_hits, out_hit_offsets, out_hits, hits_capacity, false, th);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(st->s));
  return check_status(st);
}
