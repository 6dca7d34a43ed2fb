// shardstep.hip -- slk_shard_step_device (include/slacken_amd.h): one step of the table-sharded pipeline, up to three jobs of three
// different batches in one kernel (engine.h: ShardIO; lane.hip: lane_step_kernel).  Host-side only.
#include "hostside.h"
#include "laneplan.h"

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
  // (per index, with SLK_FORCE_V1 as the environment has it at this call: the switch set refuses the step, which has no staged form)
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
    // in the scan, or a kernel of their own (laneplan.h: shard_side_per_tile)
    const uint32_t per_tile = shard_side_per_tile(scans, scans ? emit->R : 0, scans ? emit->total_bases + emit->total_mate_bases : 0, ix->sp.w, lookup->n);
    if (per_tile) {
      S.side_keys = lookup->d_keys; S.side_n = lookup->n; S.side_out = lookup->d_out_taxa;
      S.side_per_tile = per_tile;
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
