// pipe.hip -- slk_pipe (include/slacken_amd.h): batches in flight on the C ABI.  A pipe is `depth` slots; a slot is a whole
// slk_stream -- streams, read and result buffers, span scratch, status word, the record of the queued call for the unbounded
// re-run -- plus the scratch of the compact read forms (readform.hip) and pinned memory for the result rows.  slk_pipe_submit
// queues one batch on a free slot's stream with the pieces the synchronous entry is made of (hostcalls.hip: upload_range,
// host_call; classify.hip: run_classify) and returns; slk_pipe_collect synchronises that slot alone and finishes the batch as
// hostcalls.hip's finish_host_call does (check_status, assemble_hits), in a shape of its own: its rows lie in the slot's pinned
// memory already, a failure gives the slot up, and SLK_E_CAPACITY from the hit lists leaves the ticket for a second collect.
// No sub-batches inside a submit: the overlap comes from the slots.  Host-side only.
#include "hostside.h"

namespace {

struct PinnedBuf {   // pinned host memory that grows on demand (the owner selects the device before it dies)
  PinnedPtr<void> p;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    p.reset(); cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    const hipError_t e = hipHostMalloc(p.put(), want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
};

struct SideForm {   // what submit found one side of a batch to be
  bool packed = false, sparse = false;
  uint64_t total = 0;
};

struct Slot {
  slk_stream *st = nullptr;
  uint64_t ticket = 0;     // 0: free
  bool settled = false;    // synchronised and checked: the hit lists are what is left (a collect that returned SLK_E_CAPACITY)
  uint64_t R = 0;
  int32_t C = 0, hits = 0;
  Reads in;                // the batch on the device, for the hit lists
  DevBuf lengths[2], exc_word[2], exc_bits[2], scan_tmp;   // the compact forms as they arrive, per side
  PinnedBuf rows;          // taxon [C][R] | num_distinct [R] | total_kmers [R] | classified [C][R]
  int32_t *taxon() const { return (int32_t *)rows.p.get(); }
  int32_t *nd() const { return taxon() + (size_t)C * R; }
  int32_t *tk() const { return nd() + R; }
  uint8_t *cls() const { return (uint8_t *)(tk() + R); }
};

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct slk_pipe {
  slk_index *ix = nullptr;
  int32_t device = 0;
  std::vector<Slot> slots;
  uint64_t next_ticket = 1;
  bool merged = false;
};

// One side's form and its bases, from the caller's memory alone: nothing is queued or allocated here.
static int32_t check_side(const slk_reads &s, uint64_t R, const char *what, SideForm *f) {
  if ((s.bases != nullptr) == (s.codes != nullptr)) return fail(SLK_E_INVALID, "%s: exactly one of bases and codes", what);
  if (s.bases && (s.valid || s.exc_word || s.exc_bits || s.n_exc)) return fail(SLK_E_INVALID, "%s: ASCII bases take no validity arrays", what);
  if (s.valid && (s.n_exc || s.exc_word || s.exc_bits)) return fail(SLK_E_INVALID, "%s: valid and exceptions are two forms of one thing", what);
  if (s.n_exc && (!s.exc_word || !s.exc_bits)) return fail(SLK_E_INVALID, "%s: n_exc without exc_word / exc_bits", what);
  if ((s.offsets ? 1 : 0) + (s.lengths ? 1 : 0) + (s.uniform_len ? 1 : 0) != 1)
    return fail(SLK_E_INVALID, "%s: exactly one of offsets, lengths and uniform_len", what);
  f->packed = s.codes != nullptr;
  f->sparse = f->packed && !s.valid;
  const bool compact = f->sparse || !s.offsets;
  if (compact && R >= (1ULL << 32)) return fail(SLK_E_INVALID, "%s: a batch in a compact form holds fewer than 2^32 reads", what);
  if (s.offsets) {
    const int32_t rc = validate_reads(s.offsets, nullptr, R);
    if (rc) return rc;
    f->total = s.offsets[R];
  } else if (s.lengths) {
    const uint64_t PART = 1 << 18, parts = (R + PART - 1) / PART;
    std::vector<uint64_t> sums(parts, 0);
    std::vector<uint8_t> bad(parts, 0);
    host_pool().parallel_for(parts, [&](size_t pi) {
      const uint64_t r1 = std::min<uint64_t>(R, (pi + 1) * PART);
      uint64_t sum = 0;
      uint32_t top = 0;
      for (uint64_t r = pi * PART; r < r1; r++) { sum += s.lengths[r]; top |= s.lengths[r]; }
      sums[pi] = sum; bad[pi] = top > 0x7fffffffu;
    });
    for (uint64_t pi = 0; pi < parts; pi++) {
      if (bad[pi]) return fail(SLK_E_INVALID, "%s: reads are shorter than 2^31", what);
      f->total += sums[pi];
    }
  } else {
    if (s.uniform_len > 0x7fffffffu) return fail(SLK_E_INVALID, "%s: reads are shorter than 2^31", what);
    f->total = R * s.uniform_len;
  }
  if (compact && f->total >= (1ULL << 32)) return fail(SLK_E_INVALID, "%s: a side in a compact form holds fewer than 2^32 bases", what);
  const uint64_t nwords = (f->total + 15) / 16;
  for (uint64_t i = 0; i < s.n_exc; i++)
    if (s.exc_word[i] >= nwords || (i && s.exc_word[i] <= s.exc_word[i - 1]))
      return fail(SLK_E_INVALID, "%s: exc_word must be strictly ascending and below ceil(total / 16) (entry %llu)", what, (unsigned long long)i);
  return SLK_OK;
}

// the device buffers of one side's compact forms, at their sizes (before anything of the batch is queued)
static int32_t size_side(Slot &sl, int k, const slk_reads &s, const SideForm &f, uint64_t R) {
  if (s.lengths) {
    HIPCHK(sl.lengths[k].ensure(R * 4));
    HIPCHK(sl.scan_tmp.ensure((R / READFORM_TILE + 2) * 8));
  }
  if (f.sparse && s.n_exc) {
    HIPCHK(sl.exc_word[k].ensure(s.n_exc * 4));
    HIPCHK(sl.exc_bits[k].ensure(s.n_exc * 2));
  }
  return SLK_OK;
}

// One side on its way: the bases as text in d_bases, the offsets in d_offsets, all ordered on the slot's stream.
static int32_t queue_side(Slot &sl, int k, const slk_reads &s, const SideForm &f, uint64_t R, uint8_t *d_bases, DevBuf &d_codes, DevBuf &d_valid,
                          uint64_t *d_offsets) {
  slk_stream *st = sl.st;
  int32_t rc = SLK_OK;
  if (!f.sparse) {
    rc = upload_range(st, &st->staging, st->s, st->s, st->ev_unpack, f.packed, s.bases, s.codes, s.valid, d_codes, d_valid, d_bases, 0, f.total);
  } else {
    const uint64_t nwords = (f.total + 15) / 16;
    rc = copy_in(st, d_codes.p, s.codes, nwords * 4);
    if (!rc) rc = copy_in(st, sl.exc_word[k].p, s.exc_word, s.n_exc * 4);
    if (!rc) rc = copy_in(st, sl.exc_bits[k].p, s.exc_bits, s.n_exc * 2);
    if (!rc) {
      launch_unpack_sparse(d_codes.as<uint32_t>(), nwords, sl.exc_word[k].as<uint32_t>(), sl.exc_bits[k].as<uint16_t>(), s.n_exc, d_bases, st->s);
      HIPCHK(hipGetLastError());
    }
  }
  if (rc) return rc;
  if (s.offsets) return copy_in(st, d_offsets, s.offsets, (R + 1) * 8);
  if (s.lengths) {
    rc = copy_in(st, sl.lengths[k].p, s.lengths, R * 4);
    if (rc) return rc;
    launch_lengths_to_offsets(sl.lengths[k].as<uint32_t>(), R, d_offsets, sl.scan_tmp.as<uint64_t>(), f.total, st->d_status, st->s);
  } else {
    launch_uniform_offsets(s.uniform_len, R, d_offsets, st->s);
  }
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

// a slot whose batch is given up: nothing of it stays queued, and the stream is as new
static void quiesce(Slot &sl) {
  slk_stream *st = sl.st;
  for (hipStream_t s : {st->s.get(), st->s2.get()})
    if (s && hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
  st->queued.clear();
  if (*st->h_status != 0) {
    *st->h_status = 0;
    if (hipMemset(st->d_status, 0, sizeof(int32_t)) != hipSuccess) (void)hipGetLastError();
  }
}
static void release(Slot &sl) { sl.ticket = 0; sl.settled = false; }

int32_t slk_pipe_create(slk_index *ix, int32_t depth, slk_pipe **out) {
  if (!ix || !out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (depth < 1 || depth > 8) return fail(SLK_E_INVALID, "depth %d outside 1..8", depth);
  std::unique_ptr<slk_pipe> p(new slk_pipe());
  p->ix = ix; p->device = ix->device;
  p->slots.resize(depth);
  int32_t rc = SLK_OK;
  for (Slot &sl : p->slots)
    if ((rc = slk_stream_create(ix, &sl.st))) break;
  if (rc) {
    for (Slot &sl : p->slots) slk_stream_destroy(sl.st);
    return rc;
  }
  *out = p.release();
  return SLK_OK;
}

int32_t slk_pipe_set_merged_hits(slk_pipe *p, int32_t on) {
  if (!p) return fail(SLK_E_INVALID, "null handle");
  p->merged = on != 0;
  return SLK_OK;
}

int32_t slk_pipe_pending(const slk_pipe *p, int32_t *n_pending) {
  if (!p || !n_pending) return fail(SLK_E_INVALID, "null argument");
  int32_t n = 0;
  for (const Slot &sl : p->slots) n += sl.ticket != 0;
  *n_pending = n;
  return SLK_OK;
}

void slk_pipe_destroy(slk_pipe *p) {
  if (!p) return;
  for (Slot &sl : p->slots) slk_stream_destroy(sl.st);   // (selects the device and waits for the slot's streams)
  delete p;   // (the pinned rows go here: the device is still selected)
}

int32_t slk_pipe_submit(slk_pipe *p, uint64_t R, const slk_reads *reads, const slk_reads *mates, int32_t min_hit_groups, const double *thresholds,
                        int32_t C, int32_t hits, uint64_t *ticket) {
  if (!p || !reads || !ticket) return fail(SLK_E_INVALID, "null argument");
  slk_index *ix = p->ix;
  int32_t rc = check_ready(ix, p->slots[0].st, true);
  if (rc) return rc;
  if ((rc = check_thresholds(thresholds, C))) return rc;
  if (hits < 0 || hits > 2) return fail(SLK_E_INVALID, "hits %d outside 0..2", hits);
  static const bool call_timing = getenv("SLK_DEBUG_CALL_TIMING") != nullptr;   // tuning aid: wall clock of the phases of a call
  const double t0 = call_timing ? wall_ms() : 0;
  SideForm f[2];
  if ((rc = check_side(*reads, R, "reads", &f[0]))) return rc;
  if (mates && (rc = check_side(*mates, R, "mates", &f[1]))) return rc;
  Slot *slot = nullptr;
  for (Slot &sl : p->slots)
    if (!sl.ticket) { slot = &sl; break; }
  if (!slot) return fail(SLK_E_STATE, "%d tickets are uncollected: collect one first", (int)p->slots.size());
  rc = set_device(ix);
  if (rc) return rc;
  Slot &sl = *slot;
  slk_stream *st = sl.st;
  const bool paired = mates != nullptr;
  sl.R = R; sl.C = C; sl.hits = hits; sl.in = Reads{};
  st->merged_hits = p->merged;
  const double t1 = call_timing ? wall_ms() : 0;
  if (R) {
    rc = size_host_buffers(st, R, C, f[0].total, f[1].total, paired, f[0].packed || f[1].packed);   // (each side in its own form)
    if (!rc) rc = size_side(sl, 0, *reads, f[0], R);
    if (!rc && paired) rc = size_side(sl, 1, *mates, f[1], R);
    if (rc) return rc;
    HIPCHK(sl.rows.ensure((size_t)C * R * 5 + R * 8));
    // (no host offsets: a side may come as lengths or as one uniform length, and the piece route then plans from the totals)
    const ClassifyCall call = host_call(st, R, f[0].total, f[1].total, paired, thresholds, C, min_hit_groups, hits == 2, nullptr);
    sl.in = call.in;
    // (from the first copy queued, a failure leaves nothing behind that reads the caller's memory)
    rc = queue_side(sl, 0, *reads, f[0], R, st->bases.as<uint8_t>(), st->pk_codes, st->pk_valid, st->offsets.as<uint64_t>());
    if (!rc && paired)
      rc = queue_side(sl, 1, *mates, f[1], R, st->mate_bases.as<uint8_t>(), st->pk_mate_codes, st->pk_mate_valid, st->mate_offsets.as<uint64_t>());
    if (!rc) rc = run_classify(ix, st, call);
    if (!rc) {
      const hipError_t e = [&] {
        hipError_t e_ = hipMemcpyAsync(sl.taxon(), st->out_taxon.p, (size_t)C * R * 4, hipMemcpyDeviceToHost, st->s);
        if (e_ == hipSuccess) e_ = hipMemcpyAsync(sl.nd(), st->out_nd.p, R * 4, hipMemcpyDeviceToHost, st->s);
        if (e_ == hipSuccess) e_ = hipMemcpyAsync(sl.tk(), st->out_tk.p, R * 4, hipMemcpyDeviceToHost, st->s);
        if (e_ == hipSuccess) e_ = hipMemcpyAsync(sl.cls(), st->out_cls.p, (size_t)C * R, hipMemcpyDeviceToHost, st->s);
        return e_;
      }();
      if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(SLK_E_HIP, "queueing the result rows failed: %s", hipGetErrorString(e)); }
    }
    if (rc) { quiesce(sl); return rc; }
  }
  sl.ticket = p->next_ticket++;
  sl.settled = false;
  *ticket = sl.ticket;
  if (call_timing)
    fprintf(stderr, "slk_pipe_submit R=%llu ticket %llu: checks %.2f ms, queueing %.2f\n", (unsigned long long)R, (unsigned long long)sl.ticket, t1 - t0,
            wall_ms() - t1);
  return SLK_OK;
}

int32_t slk_pipe_collect(slk_pipe *p, uint64_t ticket, int32_t *out_taxon, uint8_t *out_classified, int32_t *out_num_distinct,
                         int32_t *out_total_kmers, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity) {
  if (!p) return fail(SLK_E_INVALID, "null handle");
  Slot *slot = nullptr;
  for (Slot &s : p->slots)
    if (ticket && s.ticket == ticket) { slot = &s; break; }
  if (!slot) return fail(SLK_E_STATE, "ticket %llu is not pending on this pipe", (unsigned long long)ticket);
  Slot &sl = *slot;
  slk_stream *st = sl.st;
  const uint64_t R = sl.R;
  const int32_t C = sl.C;
  if (R && (!out_taxon || !out_classified)) return fail(SLK_E_INVALID, "null argument");
  if (out_hit_offsets && !sl.hits) return fail(SLK_E_INVALID, "ticket %llu was submitted without hits", (unsigned long long)ticket);
  int32_t rc = set_device(p->ix);
  if (rc) return rc;
  if (out_hit_offsets) out_hit_offsets[0] = 0;
  if (R == 0) { release(sl); return SLK_OK; }
  static const bool call_timing = getenv("SLK_DEBUG_CALL_TIMING") != nullptr;
  double tp[4] = {call_timing ? wall_ms() : 0, 0, 0, 0};
  if (!sl.settled) {
    const hipError_t e = hipStreamSynchronize(st->s);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      quiesce(sl); release(sl);
      return fail(SLK_E_HIP, "batch %llu failed on the device: %s", (unsigned long long)ticket, hipGetErrorString(e));
    }
    if (*st->h_status & READFORM_STATUS_BIT) {
      quiesce(sl); release(sl);
      return fail(SLK_E_INVALID, "batch %llu: the lengths no longer sum to what slk_pipe_submit saw (input changed while in flight)", (unsigned long long)ticket);
    }
    rc = check_status(st);   // (re-runs the batch through the unbounded path if a taxon map overflowed)
    if (rc) { quiesce(sl); release(sl); return rc; }
    if (st->reran) {   // (the rows that came down behind the kernels are stale)
      rc = download_rows(st, HostRows{sl.taxon(), sl.cls(), sl.nd(), sl.tk()}, R, C);
      if (rc) { quiesce(sl); release(sl); return rc; }
    }
    sl.settled = true;
  }
  if (call_timing) tp[1] = wall_ms();
  if (out_hit_offsets) {
    double th[3] = {0, 0, 0};
    rc = assemble_hits(st, sl.in, sl.hits == 2, out_hit_offsets, sl.hits == 2 ? out_hits : nullptr, hits_capacity, false, th);
    if (rc == SLK_E_CAPACITY) return rc;   // (the ticket stays: out_hit_offsets says what the lists need)
    if (rc) { quiesce(sl); release(sl); return rc; }
  }
  if (call_timing) tp[2] = wall_ms();
  parallel_memcpy(out_taxon, sl.taxon(), (size_t)C * R * 4);
  parallel_memcpy(out_classified, sl.cls(), (size_t)C * R);
  if (out_num_distinct) parallel_memcpy(out_num_distinct, sl.nd(), R * 4);
  if (out_total_kmers) parallel_memcpy(out_total_kmers, sl.tk(), R * 4);
  release(sl);
  if (call_timing)
    fprintf(stderr, "slk_pipe_collect R=%llu ticket %llu: wait %.2f ms, hit lists %.2f, rows %.2f\n", (unsigned long long)R, (unsigned long long)ticket,
            tp[1] - tp[0], tp[2] - tp[1], wall_ms() - tp[2]);
  return SLK_OK;
}
