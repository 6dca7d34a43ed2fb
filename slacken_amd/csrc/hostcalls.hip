// hostcalls.hip -- the entries of the C ABI (include/slacken_amd.h) that take host memory: validation, uploads, sub-batches, the call
// over a stream's buffers (host_call) and the one way a synchronous call ends (finish_host_call), hit lists, spans, text.  Host-side only.
#include "hostside.h"

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

// ASCII reads, whole, into read buffers of exactly their size: for the entries that classify nothing on this stream's result rows
// (spans_batch) or size them per group (shardset.hip).  The classify entry's upload (size_host_buffers + upload_whole) also takes
// packed reads, rounds the buffers up to whole words of 16 bases and sizes the result rows with them, so neither serves the other.
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
  if ((rc = ensure_scratch(st, n + 1, R))) return rc;   // (a slot per hit; the key slots are the staged kernel's map scratch)
  if ((rc = ensure_outputs(st, R, C))) return rc;
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

// The call of a host entry over the stream's own buffers (sized by now: size_host_buffers, or the parser and ensure_outputs): reads
// and mates where the upload or the parser leaves them, the result rows, the thresholds by value.  h_offsets: the fragments' offsets
// as the host holds them, or null (engine.h: ClassifyCall.h_offsets).  A new call starts: what an earlier one re-ran is forgotten.
ClassifyCall slk::host_call(slk_stream *st, uint64_t R, uint64_t total, uint64_t mate_total, bool paired, const double *thresholds, int32_t C,
                            int32_t min_hit_groups, bool want_hits, const uint64_t *h_offsets) {
  ClassifyCall c;
  c.in = {st->bases.as<uint8_t>(), st->offsets.as<uint64_t>(), paired ? st->mate_bases.as<uint8_t>() : nullptr,
          paired ? st->mate_offsets.as<uint64_t>() : nullptr, R, total, mate_total};
  c.out = {st->out_taxon.as<int32_t>(), st->out_cls.as<uint8_t>(), st->out_nd.as<int32_t>(), st->out_tk.as<int32_t>(),
           st->out_nh.as<int32_t>(), nullptr, R};
  c.thr = thresholds_of(thresholds, C); c.C = C; c.min_hit_groups = min_hit_groups; c.want_hits = want_hits;
  c.h_offsets = h_offsets;
  st->reran = false;
  return c;
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
                               const ClassifyCall &whole, uint64_t SUB, const HostRows &out, bool *early_down, const PlanSwitches &sw) {
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
    rc = run_classify(ix, st, sub_call(whole, r0, r1, offsets, mate_offsets), sw);
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

// The reads of a classify call that is not cut up: everything on the stream of the kernels, packed reads too, into the buffers
// size_host_buffers rounded up for them (upload_reads, for the entries that take ASCII alone, sizes its own exactly).
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

// where a synchronous host call's results go: the rows, and the hit lists (hit_offsets null: none asked for)
struct HostOut { HostRows rows; uint64_t *hit_offsets; slk_hit *hits; uint64_t hits_capacity; };
// SLK_DEBUG_CALL_TIMING (tuning aid: wall clock of the phases of a call): the entry's name, when the call began, when its reads were up
struct CallTiming { const char *entry; double start, uploaded; };

// The end of a synchronous host call whose kernels are queued on st->s: wait for them, settle the status word (which classifies the
// batch again by the unbounded kernels if a taxon map overflowed), bring the rows down -- unless they came down early, beside the
// kernels, and nothing re-ran: early rows are stale after a re-run --, put the hit lists together, and settle the status once more.
static int32_t finish_host_call(slk_stream *st, const ClassifyCall &call, const HostOut &out, bool early_down, const CallTiming *tm) {
  const uint64_t R = call.in.R;
  HIPCHK(hipStreamSynchronize(st->s));
  const double t_kernels = tm ? now() : 0;
  int32_t rc = check_status(st);
  if (rc) return rc;
  if (early_down) HIPCHK(hipStreamSynchronize(st->ds));
  if (!early_down || st->reran) {
    rc = download_rows(st, out.rows, R, call.C);
    if (rc) return rc;
  }
  double t_rows = 0, th[3] = {0, 0, 0};
  if (tm) { (void)hipStreamSynchronize(st->s); t_rows = now(); }
  if (out.hit_offsets) {
    rc = assemble_hits(st, call.in, call.want_hits, out.hit_offsets, out.hits, out.hits_capacity, tm != nullptr, th);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(st->s));
  if (tm)
    fprintf(stderr, "%s R=%llu: upload %.2f ms, kernels %.2f, results %.2f, hit lists %.2f (offsets %.2f, gather %.2f, download %.2f)\n",
            tm->entry, (unsigned long long)R, tm->uploaded - tm->start, t_kernels - tm->uploaded, t_rows - t_kernels, now() - t_rows,
            th[0] ? th[0] - t_rows : 0.0, th[1] ? th[1] - th[0] : 0.0, th[2] ? th[2] - th[1] : 0.0);
  return check_status(st);
}

// a batch the parser left in the stream's read buffers (paired: and its mate buffers), from the result rows' sizing to the end
static int32_t classify_parsed(slk_index *ix, slk_stream *st, uint64_t R, uint64_t total, uint64_t mate_total, bool paired, int32_t min_hit_groups,
                               const double *thresholds, int32_t C, const uint64_t *h_offsets, const HostOut &out) {
  int32_t rc = ensure_outputs(st, R, C);
  if (rc) return rc;
  const ClassifyCall whole = host_call(st, R, total, mate_total, paired, thresholds, C, min_hit_groups, out.hit_offsets != nullptr && out.hits != nullptr, h_offsets);
  if ((rc = run_classify(ix, st, whole))) return rc;
  return finish_host_call(st, whole, out, false, nullptr);
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
  static const bool call_timing = getenv("SLK_DEBUG_CALL_TIMING") != nullptr;
  CallTiming tm{pk ? "slk_classify_batch_packed" : "slk_classify_batch", now(), 0};
  const HostOut out{{out_taxon, out_classified, out_num_distinct, out_total_kmers}, out_hit_offsets, out_hits, hits_capacity};
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
  const ClassifyCall whole = host_call(st, R, total, mate_total, paired, thresholds, C, min_hit_groups, out_hit_offsets != nullptr && out_hits != nullptr, offsets);
  DrainOnExit drain(st);   // (from the first copy queued below, no return leaves work behind that touches the caller's memory)
  // (the switches as this call reads them, once: cutting the batch up is the fused kernels' -- the staged ones take no span_shift --, so
  //  the sub-batches' run_classify must see what this line saw)
  const PlanSwitches sw = read_plan_switches();
  if (use_fused(ix, sw.force_v1) && R >= 2 * SUB) {
    rc = run_sub_batches(ix, st, src, offsets, mate_offsets, whole, SUB, out.rows, &early_down, sw);
    if (rc) return rc;
    if (call_timing) tm.uploaded = now();
  } else {
    rc = upload_whole(st, src, offsets, mate_offsets, whole.in);
    if (rc) return rc;
    if (call_timing) { (void)hipStreamSynchronize(st->s); tm.uploaded = now(); }
    rc = run_classify(ix, st, whole, sw);
    if (rc) return rc;
  }
  return finish_host_call(st, whole, out, early_down, call_timing ? &tm : nullptr);
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
  if (rc) return rc;
  return classify_parsed(ix, st, R, total, 0, false, min_hit_groups, thresholds, C, out_offsets,
                         {{out_taxon, out_classified, out_num_distinct, out_total_kmers}, out_hit_offsets, out_hits, hits_capacity});
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
  if (rc) return rc;
  return classify_parsed(ix, st, P, pair[6], pair[7], true, min_hit_groups, thresholds, C, nullptr,   // (pairs never take the piece route: no use for their offsets)
                         {{out_taxon, out_classified, out_num_distinct, out_total_kmers}, out_hit_offsets, out_hits, hits_capacity});
}
