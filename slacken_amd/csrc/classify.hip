// classify.hip -- the dispatch of a batch to the kernels of lane.hip / fused.hip / kernels.hip / wide.hip: the passes of the lane path as
// laneplan.h plans them, the staged kernels, the unbounded re-run; and the C ABI's entries that take device arrays.  Host-side only.
#include "hostside.h"
#include "laneplan.h"

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

// The fused wave-per-read kernels (fused.hip) cover windows of up to 32 m-mers; wider windows (and SLK_FORCE_V1=1, an
// A/B switch for tests) run the three separate lane-per-read kernels of kernels.hip.  Both are HIP: no CPU path.
// With the switch as a value: what a classify call decided once (run_classify).  Without: the environment as it is now, for the
// callers that decide per index or per entry, outside a classify call.
bool slk::use_fused(const slk_index *ix, bool force_v1) { return !force_v1 && ix->W == 1 && ix->sp.w <= 32; }
bool slk::use_fused(const slk_index *ix) { return use_fused(ix, env_on("SLK_FORCE_V1")); }

bool slk::lane_path_ok(const slk_index *ix, bool force_v1) {
  return use_fused(ix, force_v1) && ix->sp.w <= 32 && ix->internal_taxon_bits() <= 22 && ix->d_nodes != nullptr;
}
bool slk::lane_path_ok(const slk_index *ix) { return lane_path_ok(ix, env_on("SLK_FORCE_V1")); }

// The fused kernels keep a fragment's taxon -> count map in LDS (12 slots per lane, 128 per wave).  A fragment that hits more
// distinct taxa than that (long reads across conserved regions can) raises status bit 1; the batch is then classified again
// by the staged kernels, whose per-fragment map lives in HBM scratch and is unbounded -- the same three kernels that serve
// windows wider than 32 m-mers.  Slower (HBM intermediates), rare, and bit-identical for every other fragment.
// (Only a call that ran fused is ever run again -- Queued.valid, as run_classify read the switches --, and this way never asks them.)
int32_t slk::run_unbounded(slk_stream *st, const ClassifyCall &c) {
  slk_index *ix = st->ix;
  st->last_route |= SLK_ROUTE_RERUN;
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

// the part of FusedArgs every job shares: the splitter, the table, the taxonomy in the table's ids, the reads, the status word
FusedArgs slk::fused_args(const slk_index *ix, const slk_stream *st, const Reads &in) {
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

// the spans of a batch, by the kernel that scans for this index (slk_scan_device: SLK_FORCE_V1 as the environment has it at the call)
void slk::launch_spans(const slk_index *ix, slk_stream *st, const Reads &in, uint64_t *keys, int32_t *meta, int32_t *count) {
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

// ---- the fused branch of run_classify, step by step ----
// the FusedArgs of a classify call: results, thresholds, and with hit lists the span arrays they are written to
static FusedArgs call_args(const slk_index *ix, const slk_stream *st, const ClassifyCall &c) {
  FusedArgs A = fused_args(ix, st, c.in);
  A.out_stride = c.out.stride;
  A.min_hit_groups = c.min_hit_groups; A.thr = c.thr; A.C = c.C;
  A.out_taxon = c.out.taxon; A.out_classified = c.out.classified;
  A.out_nd = c.out.nd; A.out_tk = c.out.tk; A.out_nh = c.out.nh; A.out_np = c.out.np;
  A.span_meta = c.want_hits ? st->span_meta.as<int32_t>() + c.span_shift : nullptr;
  A.span_taxon = c.want_hits ? st->span_taxon.as<int32_t>() + c.span_shift : nullptr;
  A.span_count = c.want_hits ? st->span_count.as<int32_t>() : nullptr;
  return A;
}

// (scratch of the hit lists of the segment pass and the piece route: the spans' places before the borders are settled)
static uint64_t *provisional_spans(const slk_stream *st, const ClassifyCall &c) { return st->span_keys.as<uint64_t>() + c.span_shift; }

// the hand-on buffer, cleared, and the first pass over the whole batch (or the routing kernel that stands for it); fills A's hand-on fields
static int32_t first_pass(slk_stream *st, const LanePlan &plan, FusedArgs &A) {
  const size_t hdr_bytes = HandOn::WORDS * sizeof(uint64_t);
  HIPCHK(st->defer_list.ensure(plan.hand_bytes));
  HIPCHK(hipMemsetAsync(st->defer_list.p, 0, hdr_bytes, st->s));
  A.hand_hdr = (unsigned long long *)st->defer_list.p;
  A.hand_lists = (uint32_t *)((char *)st->defer_list.p + hdr_bytes);
  A.hand_stride = A.R; A.hand_long_cap = plan.long_cap; A.route_first = plan.route_first ? 1 : 0;
  A.long_max = plan.long_max; memcpy(A.long_bound, plan.long_bound, sizeof(A.long_bound));
  A.seg_min_len = plan.seg_min_len; A.wave_min = plan.wave_min; A.wave_ratio_q10 = plan.wave_ratio_q10;
  st->last_route |= plan.route_first ? SLK_ROUTE_ROUTING : SLK_ROUTE_LANE;
  if (plan.route_first) launch_route(A, st->s);
  else launch_lane(A, nullptr, 1000, st->s);  // (the one-word map entries carry 10-bit k-mer counts)
  return SLK_OK;
}

// the piece route on s2: its scratch as piece_layout carves it, the header's memset, the cut and its passes -- before the segment
// pass, since the cut takes its fragments out of that pass's list
static int32_t piece_pass(slk_stream *st, const ClassifyCall &c, const LanePlan &plan, const FusedArgs &A, uint32_t taxa_bound) {
  const PieceLayout lay = piece_layout(plan);
  HIPCHK(st->piece_scratch.ensure(lay.scratch_bytes));
  HIPCHK(st->piece_maps.ensure(lay.maps_bytes));
  if (plan.piece_hits) HIPCHK(st->piece_hits.ensure(lay.hits_bytes));
  PieceArgs X{};
  char *const base = (char *)st->piece_scratch.p;
  X.hdr = (unsigned long long *)base; X.frags = (PieceFrag *)(base + lay.frags_at); X.units = (uint64_t *)(base + lay.units_at);
  X.records = (PieceRecord *)(base + lay.records_at);
  X.map_key = st->piece_maps.as<int32_t>(); X.map_cnt = X.map_key + plan.piece_map;
  X.frag_cap = plan.piece_frags; X.unit_cap = plan.piece_units; X.map_cap = plan.piece_map;
  X.seg_list = A.hand_lists + HandOn::list_at(HandOn::SEG, A.R, plan.long_cap); X.seg_count = A.hand_hdr + HandOn::SEG;
  X.min_len = plan.piece_min_len; X.windows = plan.piece_windows; X.taxa_bound = taxa_bound;
  HIPCHK(hipMemsetAsync(X.hdr, 0, lay.frags_at, st->s2));
  FusedArgs P = A;
  if (plan.piece_hits) {
    X.hits = st->piece_hits.as<PieceHitRecord>();
    P.span_keys = provisional_spans(st, c);
  }
  launch_pieces(P, X, st->s2);
  st->last_used_pieces = true;
  st->last_route |= SLK_ROUTE_PIECES;
  return SLK_OK;
}

static void segment_pass(slk_stream *st, const ClassifyCall &c, const LanePlan &plan, const FusedArgs &A) {
  FusedArgs B = A;
  if (c.want_hits) B.span_keys = provisional_spans(st, c);
  B.work_list = A.hand_lists + HandOn::list_at(HandOn::SEG, A.R, plan.long_cap); B.work_count = A.hand_hdr + HandOn::SEG; B.work_draw = A.hand_hdr + HandOn::SEG_DRAW;
  launch_segments(B, st->s2);
  st->last_route |= SLK_ROUTE_SEGMENT;
}

// the wave kernel over its lists strung together longest first (launch_order_wave_list)
static void ordered_wave_pass(slk_stream *st, const ClassifyCall &c, const LanePlan &plan, const FusedArgs &A) {
  FusedArgs W = A;
  launch_order_wave_list(W, st->s2);
  W.work_list = A.hand_lists + HandOn::ordered_at(A.R, plan.long_cap); W.work_count = A.hand_hdr + HandOn::ORDERED; W.work_draw = A.hand_hdr + HandOn::WAVE_DRAW;
  launch_fused(c.want_hits ? MODE_HITS : MODE_CLASSIFY, W, st->s2);
  st->last_route |= SLK_ROUTE_WAVE;
}

// what the long variant handed on in turn (map overflows), when both streams are through
static void late_list_pass(slk_stream *st, const ClassifyCall &c, const LanePlan &plan, FusedArgs A) {
  A.work_list = A.hand_lists + HandOn::list_at(HandOn::LATE, A.R, plan.long_cap); A.work_count = A.hand_hdr + HandOn::N_LATE; A.work_draw = A.hand_hdr + HandOn::LATE_DRAW;
  launch_fused(c.want_hits ? MODE_HITS : MODE_CLASSIFY, A, st->s);
  st->last_route |= SLK_ROUTE_WAVE;
}

// The passes over the hand-on lists depend on the first pass only, and the long variant runs BESIDE the other two (which
// follow each other on a second stream): with a few hundred thousand long fragments in a batch the long variant is a handful
// of waves per CU working through 5 000 lockstep steps, the segment pass not much more, and the wave kernel behind them on one
// stream waited for both (nanopore-like mix: 1.1 + 4.9 + 5.8 ms one after the other, 77-84 Gbp/s; 95-101 this way;
// profiles/r04_long_mixed_trace.txt).  Segment pass before wave pass: the wave kernel is bound by instruction issue and holds
// every wave slot until it is through, the other two are chains of dependent steps that share a CU well.  What the long
// variant hands on in turn (map overflows) goes to a list of its own that a second launch of the wave kernel takes when
// both streams are through.
static int32_t run_lane_path(slk_stream *st, const ClassifyCall &c, const LanePlan &plan, FusedArgs A, uint32_t taxa_bound) {
  st->last_used_lane = true;
  int32_t rc = first_pass(st, plan, A);
  if (!rc) rc = fork_ready(st);
  if (rc) return rc;
  HIPCHK(hipEventRecord(st->ev_fork, st->s));
  if (A.long_max) st->last_route |= SLK_ROUTE_LONG;
  if (A.long_max) launch_lane_long(A, A.long_max, st->s);   // (first: its chain of steps is the longest, whoever comes first gets the CUs)
  HIPCHK(hipStreamWaitEvent(st->s2, st->ev_fork, 0));
  if (plan.piece_min_len && (rc = piece_pass(st, c, plan, A, taxa_bound))) return rc;
  if (plan.seg_on) segment_pass(st, c, plan, A);
  ordered_wave_pass(st, c, plan, A);
  HIPCHK(hipEventRecord(st->ev_join, st->s2));
  HIPCHK(hipStreamWaitEvent(st->s, st->ev_join, 0));
  if (A.long_max) late_list_pass(st, c, plan, A);
  return SLK_OK;
}

// the batch by the fused kernels: the lane path where the index and the plan allow it, else the wave-per-fragment kernel alone
static int32_t run_fused(slk_index *ix, slk_stream *st, const ClassifyCall &c, const PlanSwitches &sw) {
  const Reads &in = c.in;
  const FusedArgs A = call_args(ix, st, c);
  const uint32_t taxa_bound = 1u << std::min(ix->internal_taxon_bits(), 22);   // (lane_path_ok: at most 22 bits)
  LanePlan plan;
  if (lane_path_ok(ix, sw.force_v1)) {
    PlanInput pi;
    pi.R = in.R; pi.all_bases = in.total + in.mate_total; pi.paired = in.paired(); pi.want_hits = c.want_hits;
    pi.w = ix->sp.w; pi.k = ix->sp.k; pi.split_long = st->split_long; pi.split_hits = st->split_hits;
    pi.taxa_bound = taxa_bound; pi.h_offsets = c.h_offsets;
    plan = plan_lane(pi, sw);
  }
  st->last_used_pieces = false;
  st->split_reported = false;
  if (plan.lane) {
    const int32_t rc = run_lane_path(st, c, plan, A, taxa_bound);
    if (rc) return rc;
  } else {
    launch_fused(c.want_hits ? MODE_HITS : MODE_CLASSIFY, A, st->s);
    st->last_route |= SLK_ROUTE_WAVE;
  }
  HIPCHK(hipEventRecord(st->ev[1], st->s));   // (no stages to tell apart: slk_stream_last_stage_ms reports all of it as the first)
  HIPCHK(hipEventRecord(st->ev[2], st->s));
  return SLK_OK;
}

// the batch by the three staged kernels (wide minimizers, windows over 32 m-mers, SLK_FORCE_V1)
static int32_t run_staged(slk_index *ix, slk_stream *st, const ClassifyCall &c) {
  const Reads &in = c.in;
  st->last_route |= SLK_ROUTE_STAGED;
  uint64_t *const keys = st->span_keys.as<uint64_t>();
  int32_t *const meta = st->span_meta.as<int32_t>(), *const taxa = st->span_taxon.as<int32_t>(), *const count = st->span_count.as<int32_t>();
  if (ix->W > 1) launch_wide_scan(ix->wp, in.bases, in.offsets, in.mate_bases, in.mate_offsets, in.R, keys, meta, count, st->s);
  else launch_scan(ix->sp, in.bases, in.offsets, in.mate_bases, in.mate_offsets, in.R, keys, meta, count, st->s);
  HIPCHK(hipEventRecord(st->ev[1], st->s));
  if (ix->W > 1) launch_wide_probe(ix->wt, ix->W, in.offsets, in.mate_offsets, in.R, keys, meta, count, taxa, st->s);
  else launch_probe(ix->view(), in.offsets, in.mate_offsets, in.R, keys, meta, count, taxa, st->s);
  HIPCHK(hipEventRecord(st->ev[2], st->s));
  // the key slots are dead after the probe: the per-read taxon->count map reuses them
  launch_classify(ix->d_parents, ix->d_nodes_orig, ix->T, c, meta, taxa, count, keys, st->s);
  return SLK_OK;
}

int32_t slk::run_classify(slk_index *ix, slk_stream *st, const ClassifyCall &call) { return run_classify(ix, st, call, read_plan_switches()); }

int32_t slk::run_classify(slk_index *ix, slk_stream *st, const ClassifyCall &call, const PlanSwitches &sw) {
  ClassifyCall c = call;
  if (c.out.stride == 0) c.out.stride = c.in.R;
  const Reads &in = c.in;
  // The switches, read once per call (above, or by the host entry that cuts its batch up): the branch taken here, the scratch sized
  // for it, the plan of the lane path and whether check_status may run the call again (Queued.valid) all follow from that one reading,
  // whatever the environment says a moment later.
  const bool fused = use_fused(ix, sw.force_v1);
  int32_t rc;
  st->last_used_lane = false;
  st->last_route = 0;
  if (!fused || c.want_hits) {
    rc = ensure_scratch(st, span_slots(in.total, in.mate_total, in.R, in.paired()) + c.span_shift, in.R);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(st->ev[0], st->s));
  if (st->queued.size() >= 4096) {  // (a caller that never synchronises: settle what is queued before taking more)
    HIPCHK(hipStreamSynchronize(st->s));
    rc = check_status(st);
    if (rc) return rc;
  }
  st->queued.push_back({c, fused});
  rc = fused ? run_fused(ix, st, c, sw) : run_staged(ix, st, c);
  if (rc) return rc;
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
