// stream.hip -- a stream of the C ABI (include/slacken_amd.h): its lifetime and settings, the status word with the unbounded
// re-run's trigger (check_status), the second stream of a call (fork_ready), and what a caller may ask about the last call.
// Host-side only.
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

int32_t slk::check_ready(const slk_index *ix, const slk_stream *st, bool need_tax) {
  if (!ix || !st) return fail(SLK_E_INVALID, "null handle");
  if (st->ix != ix) return fail(SLK_E_INVALID, "stream belongs to a different index");
  if (!ix->finalized) return fail(SLK_E_STATE, "index is not finalized");
  if (need_tax && !ix->d_parents) return fail(SLK_E_STATE, "taxonomy not set");
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

// the second stream of a classify call or a sharded step, and the two events that fork it from s and join it again
int32_t slk::fork_ready(slk_stream *st) {
  if (st->ev_join) return SLK_OK;
  HIPCHK(hipStreamCreateWithFlags(st->s2.put(), hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(st->ev_fork.put(), hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(st->ev_join.put(), hipEventDisableTiming));
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

// (host-side bookkeeping alone, no device call: the bits are set where the launches are issued -- classify.hip --, the re-run's when
//  check_status issues it, i.e. in the caller's slk_stream_synchronize or at the end of a host entry)
int32_t slk_stream_last_route(slk_stream *st, uint32_t *mask) {
  if (!st || !mask) return fail(SLK_E_INVALID, "null argument");
  *mask = st->last_route;
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

// (what the stream HOLDS: the buffers' capacities, which grow past the bytes laneplan.h's piece_layout asks for and never shrink)
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
