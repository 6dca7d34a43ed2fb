// classify_stream.hpp -- one pass of the hot path over all input fragments: batches are parsed ahead on reader threads, classified by a
// few workers, and handed on in input order (inputs: S/kmers/input/FileInputs.scala:64-85,156-221, InputReader.scala:105-131).
#pragma once
#include <atomic>
#include <functional>

#include "device_index.hpp"
#include "pack.hpp"

namespace slk_host {

// Several input files (or pairs) are read side by side, each on its own threads (a gzip file on the cores' share of it, pargz.hpp), and
// their batches are taken in turn: the order of the output is deterministic, though interleaved between files at batch
// granularity (the reference's output order is whatever Spark's partitions give).
class InputRotation {
  const std::vector<std::string> &files_;
  const bool paired_;
  RepeatedTitles *rep_;
  const size_t unit_, nsrc_;
  size_t next_src_ = 0, turn_ = 0;
  std::vector<std::unique_ptr<BatchPrefetcher>> active_;
  std::unique_ptr<BatchPrefetcher> open_next() {
    if (next_src_ >= nsrc_) return nullptr;
    std::vector<std::string> fs(files_.begin() + next_src_ * unit_, files_.begin() + (next_src_ + 1) * unit_);
    next_src_++;
    return std::make_unique<BatchPrefetcher>(fs, paired_, rep_);
  }
 public:
  InputRotation(const std::vector<std::string> &files, bool paired, RepeatedTitles *rep)
      : files_(files), paired_(paired), rep_(rep), unit_(paired ? 2 : 1), nsrc_(files.size() / unit_) {
    const char *cenv = getenv("SLK_INPUT_STREAMS");
    const size_t conc = std::max<size_t>(1, std::min<size_t>(nsrc_, cenv ? (size_t)atol(cenv) : 8));
    gz_concurrent_files() = (int)(conc * unit_);
    while (active_.size() < conc) { auto r = open_next(); if (!r) break; active_.push_back(std::move(r)); }
  }
  FragmentBatchPtr next() {
    while (!active_.empty()) {
      if (turn_ >= active_.size()) turn_ = 0;
      auto b = active_[turn_]->next();
      if (b) { turn_++; return b; }
      auto r = open_next();  // this file is exhausted: the next unopened one takes its place in the rotation
      if (r) active_[turn_] = std::move(r);
      else active_.erase(active_.begin() + turn_);
    }
    return nullptr;
  }
};

// Batches carry the ticket they were taken with and are handed on in ticket order, whichever worker is done first.  The first
// failure is kept and releases everybody who waits for a turn.
class OrderedHandOver {
  std::mutex mu_;
  std::condition_variable cv_;
  size_t next_out_ = 0;
  std::exception_ptr failure_;
  std::atomic<bool> failed_{false};
 public:
  size_t next_ticket = 0;   // under the lock of the input: a ticket is taken together with its batch
  bool failed() const { return failed_; }
  template <class Hand> void deliver(size_t ticket, Hand hand) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return next_out_ == ticket || failure_; });
    if (!failure_) hand();
    next_out_ = ticket + 1;
    cv_.notify_all();
  }
  void fail(std::exception_ptr e) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!failure_) failure_ = e;
    failed_ = true;
    next_out_ = (size_t)-1;  // (nobody waits for a ticket any more)
    cv_.notify_all();
  }
  void rethrow_failure() { if (failure_) std::rethrow_exception(failure_); }
};

// The batches are classified by a few worker threads, each with a stream of its own (its scratch, its staging buffers, its
// HIP stream): one worker's copies overlap another's kernels.  Batches are taken and handed to f in input order.
// --shard-table: a worker takes up to one batch per device table, classifies them as ONE round of its shard set, and hands them
// on in input order; a second worker's round (its own set) overlaps the first one's copies and host work.
template <class F> struct ClassifyPass {
  DeviceIndex &dev;
  const int min_hits;
  const std::vector<double> &thresholds;
  const bool want_spans, want_hits;
  const std::function<void(const FragmentBatch &)> &pre;
  F &f;
  InputRotation input;
  std::mutex mu_in, mu_stat;
  OrderedHandOver order;
  std::atomic<size_t> total{0}, n_batches{0};
  double t_input = 0, t_device = 0, t_hand_over = 0;   // where the wall clock of the workers goes, by stage (SLK_HOST_TIMING)
  // SLK_CLI_PACKED=1: reports-only calls send the reads packed (3 bits per base).  Off by default: this host is bound by parsing, not
  // by the link -- 10 M reads from a FASTQ file, reports only: 0.83 s as text, 0.87 s packed (the packing is the workers' time;
  // profiles/r04_cli_packed_ab.txt) -- the packed entry pays where the caller's reads are packed already or the link is the limit.
  const bool packed_calls = getenv("SLK_CLI_PACKED") && getenv("SLK_CLI_PACKED")[0] == '1';

  struct Lane { slk_index *ix = nullptr; slk_stream *st = nullptr; slk_shardset *set = nullptr; };   // what a worker drives: a stream or a shard set
  struct Scratch { std::vector<int32_t> nd, tk; std::vector<uint32_t> pk_codes, pk_mcodes; std::vector<uint16_t> pk_valid, pk_mvalid; };   // a worker's own

  // a batch's fragments into the record both modes fill; returns what the call is given for it
  slk_shard_batch prepare(FragmentBatchPtr frags, ClassifiedBatch &b, Scratch &s) {
    n_batches++;
    b.frags = std::move(frags);
    b.C = (int)thresholds.size();
    const FragmentBatch &fb = *b.frags;
    const size_t n = fb.size();
    total += n;
    if (pre) pre(fb);   // (on the worker's own time, not under the output's lock)
    b.taxon.resize((size_t)b.C * n); b.classified.resize((size_t)b.C * n); s.nd.resize(n); s.tk.resize(n);
    b.hit_offs.resize(n + 1);
    const size_t cap = fb.bases.size() + fb.mate_bases.size() + n + 1;
    if (want_hits) b.reserve_hits(cap);
    return slk_shard_batch{fb.bases.data(), fb.offs.data(), fb.paired ? fb.mate_bases.data() : nullptr, fb.paired ? fb.mate_offs.data() : nullptr,
                           n, b.taxon.data(), b.classified.data(), s.nd.data(), s.tk.data(), b.hit_offs.data(), want_hits ? b.hits.get() : nullptr, cap};
  }

  void classify_replicated(const Lane &lane, const slk_shard_batch &c, ClassifiedBatch &b, Scratch &s) {
    const FragmentBatch &fb = *b.frags;
    if (!want_hits && packed_calls) {
      // reports only: nothing but the reads crosses the link, so they cross it in the engine's 3-bit form -- packed here, on the
      // worker's own time (pack.hpp: AVX2 + BMI2), 6 bytes per 16 bases instead of 16
      s.pk_codes.resize((fb.bases.size() + 15) / 16 + 1); s.pk_valid.resize(s.pk_codes.size());
      slk::pack_bases(fb.bases.data(), fb.bases.size(), s.pk_codes.data(), s.pk_valid.data());
      if (fb.paired) {
        s.pk_mcodes.resize((fb.mate_bases.size() + 15) / 16 + 1); s.pk_mvalid.resize(s.pk_mcodes.size());
        slk::pack_bases(fb.mate_bases.data(), fb.mate_bases.size(), s.pk_mcodes.data(), s.pk_mvalid.data());
      }
      SLK_CALL(slk_classify_batch_packed(lane.ix, lane.st, s.pk_codes.data(), s.pk_valid.data(), c.offsets, fb.paired ? s.pk_mcodes.data() : nullptr,
                                         fb.paired ? s.pk_mvalid.data() : nullptr, c.mate_offsets, c.R, min_hits, thresholds.data(), b.C, c.out_taxon,
                                         c.out_classified, c.out_num_distinct, c.out_total_kmers, c.out_hit_offsets, nullptr, c.hits_capacity));
    } else {
      SLK_CALL(slk_classify_batch(lane.ix, lane.st, c.bases, c.offsets, c.mate_bases, c.mate_offsets, c.R, min_hits, thresholds.data(), b.C,
                                  c.out_taxon, c.out_classified, c.out_num_distinct, c.out_total_kmers, c.out_hit_offsets, c.out_hits, c.hits_capacity));
    }
    if (want_spans) {
      b.span_offs.resize(c.R + 1);
      b.spans.resize(c.hits_capacity);
      SLK_CALL(slk_spans_batch(lane.ix, lane.st, c.bases, c.offsets, c.mate_bases, c.mate_offsets, c.R, b.span_offs.data(), b.spans.data(), c.hits_capacity));
    }
  }

  size_t take(size_t G, std::vector<FragmentBatchPtr> &in) {   // up to G batches, in input order; returns the ticket of the first
    std::lock_guard<std::mutex> lk(mu_in);
    const size_t ticket0 = order.next_ticket;
    for (FragmentBatchPtr fb; in.size() < G && (fb = input.next()); order.next_ticket++) in.push_back(std::move(fb));
    return ticket0;
  }

  void work(const Lane &lane) {
    const size_t G = lane.set ? dev.ixs.size() : 1;   // the group a worker takes at a time: a batch, or a round of one per device table
    std::vector<Scratch> scratch(G);
    std::vector<FragmentBatchPtr> in;
    std::vector<std::shared_ptr<ClassifiedBatch>> out;
    std::vector<slk_shard_batch> round;
    double w_input = 0, w_device = 0, w_hand_over = 0;
    try {
      while (!order.failed()) {
        const double t0 = wall_seconds();
        in.clear();
        const size_t ticket0 = take(G, in);
        if (in.empty()) break;
        const double t1 = wall_seconds();
        out.clear();
        round.assign(G, slk_shard_batch{});
        for (size_t g = 0; g < in.size(); g++) {
          out.push_back(new_classified_batch());
          round[g] = prepare(std::move(in[g]), *out[g], scratch[g]);
        }
        if (lane.set) SLK_CALL(slk_shardset_classify(lane.set, round.data(), min_hits, thresholds.data(), (int)thresholds.size()));
        else classify_replicated(lane, round[0], *out[0], scratch[0]);
        const double t2 = wall_seconds();
        for (size_t g = 0; g < out.size(); g++)
          order.deliver(ticket0 + g, [&] { f(std::shared_ptr<const ClassifiedBatch>(std::move(out[g]))); });
        w_input += t1 - t0; w_device += t2 - t1; w_hand_over += wall_seconds() - t2;
      }
    } catch (...) {
      order.fail(std::current_exception());
    }
    std::lock_guard<std::mutex> lk(mu_stat);
    t_input += w_input; t_device += w_device; t_hand_over += w_hand_over;
  }
};

// merged_hits: the hit lists come merged as TaxonCounts.fromHits merges them (slk_stream_set_merged_hits) -- for a consumer that only
// prints them (OutputSink), a sixth of the bytes on the way back; never with spans (their lists go by position) nor on a shard set.
// Batches are handed to f with shared ownership: output formatting keeps them alive on its own threads.
template <class F>
void classify_stream(DeviceIndex &dev, const std::vector<std::string> &files, bool paired, int min_hits, const std::vector<double> &thresholds,
                     bool want_spans, bool want_hits, F f, RepeatedTitles *rep = nullptr,
                     const std::function<void(const FragmentBatch &)> &pre = nullptr, bool merged_hits = false) {
  if (want_spans && dev.sharded) die("internal: classify_stream serves no spans from a sharded table");
  using Pass = ClassifyPass<F>;
  Pass pass{dev, min_hits, thresholds, want_spans, want_hits, pre, f, InputRotation(files, paired, rep)};
  const char *wenv = getenv("SLK_CLASSIFY_THREADS");
  // (SLK_CLASSIFY_THREADS: threads per device; with several devices worker i drives device i mod N, each on its own table)
  const size_t per_dev = std::max<size_t>(1, std::min<size_t>(8, wenv ? (size_t)atol(wenv) : 2));
  const size_t n_workers = per_dev * dev.ixs.size();
  static const bool no_merge = getenv("SLK_CLI_MERGED_HITS") && getenv("SLK_CLI_MERGED_HITS")[0] == '0';   // (A/B switch)
  const bool merge = merged_hits && want_hits && !want_spans && !no_merge;
  std::vector<typename Pass::Lane> lanes(dev.sharded ? dev.sets.size() : n_workers);   // (sharded: a worker per shard set)
  for (size_t i = 0; i < lanes.size(); i++) {
    if (dev.sharded) { lanes[i].set = dev.sets[i]; continue; }
    lanes[i].ix = dev.ixs[i % dev.ixs.size()];
    lanes[i].st = dev.st;   // the first worker runs on the calling thread with the device's own stream
    if (i > 0) SLK_CALL(slk_stream_create(lanes[i].ix, &lanes[i].st));
    SLK_CALL(slk_stream_set_merged_hits(lanes[i].st, merge ? 1 : 0));
    SLK_CALL(slk_stream_set_split_long(lanes[i].st, dev.split_long));
    SLK_CALL(slk_stream_set_split_hits(lanes[i].st, dev.split_hits ? 1 : 0));
  }
  std::vector<std::thread> workers;
  for (size_t i = 1; i < lanes.size(); i++) workers.emplace_back([&pass, &lanes, i] { pass.work(lanes[i]); });
  pass.work(lanes[0]);
  for (auto &t : workers) t.join();
  for (size_t i = 1; i < lanes.size(); i++) if (lanes[i].st) slk_stream_destroy(lanes[i].st);
  if (!dev.sharded) (void)slk_stream_set_merged_hits(dev.st, 0);   // (the device's own stream serves other callers: un-merged lists again)
  if (!dev.sharded) (void)slk_stream_set_split_long(dev.st, -1);
  if (!dev.sharded) (void)slk_stream_set_split_hits(dev.st, 0);
  pass.order.rethrow_failure();
  if (getenv("SLK_HOST_TIMING"))
    std::cerr << "host timing: " << pass.n_batches << " batches on " << n_workers << " classify thread(s) over " << dev.ixs.size() << " device table(s); summed over them: waiting for input "
              << pass.t_input << " s, upload+kernels+download " << pass.t_device << " s, waiting for their turn and handing over to the output threads "
              << pass.t_hand_over << " s" << std::endl;
  std::cerr << pass.total << " fragments" << std::endl;
}

// ---- --device-parse: the device finds the records (slk_classify_text, slk_parse_text) --------------------------------
// The raw bytes of a file -- a plain file's, or what the inflate threads deliver -- go to the device in chunks.  A chunk that is not
// the file's last is parsed with final = 0: the device takes the records that are decided inside it and says where the next chunk
// starts (`consumed`).  That position follows from the last few lines of the chunk alone, so the reader computes it here as well
// (text_chunk_cut: a walk back over two lines, or to the last '>') and carries text[cut, n) over without waiting for the device; the
// workers then run side by side, and each checks the device's answer against the cut it was given.

// the largest line start below q (seqio.hpp: is_line_start); q > 0
inline size_t prev_line_start(const char *d, size_t q) {
  for (size_t p = q - 1; p > 0; p--)
    if (d[p - 1] == '\n' || (d[p - 1] == '\r' && d[p] != '\n')) return p;
  return 0;
}
// `consumed` of a non-final chunk, as the device parser defines it: FASTQ -- the start of the last but one line that is present (a
// line is present when its terminator lies inside the chunk; a \r on the last byte is undecided), FASTA -- the last '>'; 0: the chunk
// must grow
inline size_t text_chunk_cut(const char *d, size_t n, bool fastq) {
  if (n == 0) return 0;
  if (!fastq) {
    const void *g = memrchr(d, '>', n);
    return g ? (size_t)((const char *)g - d) : 0;
  }
  const size_t end = d[n - 1] == '\n' ? n : prev_line_start(d, n);   // where the lines that are present end
  if (end == 0) return 0;
  const size_t last = prev_line_start(d, end);
  return last == 0 ? 0 : prev_line_start(d, last);
}

struct PinnedText {   // a worker's chunk in pinned memory: the upload is a DMA out of it
  char *p = nullptr;
  size_t cap = 0;
  PinnedText() = default;
  PinnedText(const PinnedText &) = delete;
  ~PinnedText() { if (p) (void)slk_host_free(p); }
  void ensure(size_t bytes, size_t keep) {   // the first `keep` bytes survive
    if (bytes <= cap) return;
    void *q = nullptr;
    const size_t want = bytes + bytes / 4 + 4096;
    SLK_CALL(slk_host_alloc(want, &q));
    if (keep) memcpy(q, p, keep);
    if (p) (void)slk_host_free(p);
    p = (char *)q;
    cap = want;
  }
};

// The chunks of a list of files, in order; one caller at a time.  A compressed file or a pipe is read through ByteSource into the
// caller's pinned buffer, behind what the chunk before left over.  A plain file is mapped, as the host parser maps it: a chunk is a
// range of the mapping (c.p points into it: the library stages the upload on its copy threads, as it does for a parsed batch), the next
// one starts at the cut, and nothing is copied here.  The mappings live as long as this object.
class TextChunks {
 public:
  static constexpr size_t MAX_CHUNK = (size_t)1 << 30;
  struct Chunk { const char *p = nullptr; size_t n = 0, cut = 0; bool final = false, fastq = false; };
 private:
  const std::vector<std::string> &files_;
  size_t next_file_ = 0;
  std::unique_ptr<ByteSource> src_;
  std::string file_, carry_;
  bool fastq_ = false;
  const size_t chunk_ = io_chunk_bytes();
  struct Mapping { const char *p; size_t n; };
  std::vector<Mapping> maps_;
  const char *map_ = nullptr;   // the plain file being read, or null
  size_t map_len_ = 0, map_pos_ = 0;

  friend class PairedTextChunks;
  static bool plain_file(const std::string &file) {
    if (!ByteSource::regular_file(file) || ends_with(file, ".gz") || ends_with(file, ".bz2")) return false;
    FILE *f = fopen(file.c_str(), "rb");
    if (!f) die("cannot open " + file);
    unsigned char m[2] = {0, 0};
    const size_t k = fread(m, 1, 2, f);
    fclose(f);
    return !(k == 2 && m[0] == 0x1f && m[1] == 0x8b);   // (zlib would inflate a gzip file under any name)
  }
  bool open_next() {
    if (next_file_ >= files_.size()) return false;
    file_ = files_[next_file_++];
    fastq_ = RecordStream::is_fastq_name(file_);
    carry_.clear();
    if (!plain_file(file_)) { src_ = std::make_unique<ByteSource>(file_); return true; }
    const int fd = open(file_.c_str(), O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) die("cannot open " + file_);
    map_len_ = (size_t)sb.st_size;
    map_pos_ = 0;
    void *m = map_len_ ? mmap(nullptr, map_len_, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (map_len_ && m == MAP_FAILED) die("cannot map " + file_);
    if (map_len_) { madvise(m, map_len_, MADV_SEQUENTIAL); maps_.push_back({(const char *)m, map_len_}); }
    static const char empty = 0;
    map_ = map_len_ ? (const char *)m : &empty;
    return true;
  }
  bool next_mapped(Chunk &c) {   // false: this file is through
    const size_t left = map_len_ - map_pos_;
    if (left == 0) { map_ = nullptr; return false; }
    c.p = map_ + map_pos_;
    c.fastq = fastq_;
    for (size_t n = std::min(chunk_, left);; n = std::min(2 * n, std::min(left, MAX_CHUNK))) {
      c.n = n;
      c.final = n == left;
      c.cut = c.final ? n : text_chunk_cut(c.p, n, fastq_);
      if (c.cut > 0) break;
      if (n >= MAX_CHUNK)
        die("a record of " + file_ + " does not fit the largest chunk the device parser takes (1 GiB): classify this input without --device-parse");
    }
    map_pos_ += c.cut;
    return true;
  }
 public:
  explicit TextChunks(const std::vector<std::string> &files) : files_(files) {}
  TextChunks(const TextChunks &) = delete;
  ~TextChunks() { for (const Mapping &m : maps_) munmap((void *)m.p, m.n); }
  bool next(PinnedText &b, Chunk &c) {   // false: the input is exhausted
    for (;;) {
      if (!src_ && !map_ && !open_next()) return false;
      if (map_) {
        if (next_mapped(c)) return true;
        continue;
      }
      size_t n = carry_.size(), want = chunk_;
      b.ensure(n + want, 0);
      memcpy(b.p, carry_.data(), n);
      c.fastq = fastq_;
      for (;;) {
        b.ensure(n + want, n);
        const size_t got = src_->read(b.p + n, want);
        n += got;
        if (got == 0) { c.final = true; c.cut = n; break; }
        c.final = false;
        c.cut = text_chunk_cut(b.p, n, fastq_);
        if (c.cut > 0) break;
        if (n >= MAX_CHUNK)
          die("a record of " + file_ + " does not fit the largest chunk the device parser takes (1 GiB): classify this input without --device-parse");
        want = std::min(std::max(n, chunk_), MAX_CHUNK - n);   // no record ends inside the chunk: twice the bytes
      }
      c.n = n;
      c.p = b.p;
      if (c.final) src_.reset();
      else carry_.assign(b.p + c.cut, n - c.cut);
      if (n > 0) return true;   // (a file that ends on a chunk border leaves an empty last chunk: on to the next file)
    }
  }
};

// classify_stream with the records found on the device: unpaired input, a replicated table, one id column (the command line refuses
// the rest).  A batch is a chunk of text; what comes back fills a FragmentBatch that holds the offsets and the titles only -- the
// titles copied out of the chunk by (position, length) -- and everything downstream of f works on it as on a parsed batch.
template <class F>
void classify_text_stream(DeviceIndex &dev, const std::vector<std::string> &files, int min_hits, const std::vector<double> &thresholds,
                          bool want_hits, F f, bool merged_hits = false) {
  if (dev.sharded) die("internal: classify_text_stream runs on a replicated table");
  TextChunks input(files);
  std::mutex mu_in;
  OrderedHandOver order;
  std::atomic<size_t> total{0}, n_batches{0};
  const int C = (int)thresholds.size();
  struct Lane { slk_index *ix = nullptr; slk_stream *st = nullptr; };
  auto work = [&](const Lane &lane) {
    PinnedText buf;
    std::vector<int32_t> nd, tk;
    std::vector<uint64_t> tpos;
    std::vector<uint32_t> tlen;
    try {
      while (!order.failed()) {
        TextChunks::Chunk c;
        size_t ticket;
        {
          std::lock_guard<std::mutex> lk(mu_in);
          if (!input.next(buf, c)) break;
          ticket = order.next_ticket++;
        }
        n_batches++;
        auto out = new_classified_batch();
        ClassifiedBatch &b = *out;
        b.frags = new_fragment_batch(1);
        b.C = C;
        FragmentBatch &fb = *b.frags;
        if (want_hits) b.reserve_hits(c.n + 1);   // (a span per base at most)
        uint64_t R = 0, consumed = 0;
        size_t rcap = c.n / 64 + 1024;   // records the arrays hold: a guess, and what the call asks for if the guess was short
        for (int attempt = 0;; attempt++) {
          b.taxon.resize((size_t)C * rcap); b.classified.resize((size_t)C * rcap); nd.resize(rcap); tk.resize(rcap);
          fb.offs.resize(rcap + 1); tpos.resize(rcap); tlen.resize(rcap); b.hit_offs.resize(rcap + 1);
          const int32_t rc = slk_classify_text(lane.ix, lane.st, (const uint8_t *)c.p, c.n, c.fastq ? SLK_FORMAT_FASTQ : SLK_FORMAT_FASTA, c.final ? 1 : 0,
                                               min_hits, thresholds.data(), C, b.taxon.data(), b.classified.data(), nd.data(), tk.data(), fb.offs.data(),
                                               tpos.data(), tlen.data(), b.hit_offs.data(), want_hits ? b.hits.get() : nullptr, rcap, c.n + 1, &R, &consumed);
          if (rc == SLK_E_CAPACITY && attempt == 0 && R > rcap) { rcap = R; continue; }
          if (rc != SLK_OK) die(std::string("slk_classify_text: ") + slk_last_error());
          break;
        }
        if (!c.final && consumed != c.cut)
          die("internal: the device parser consumed " + std::to_string(consumed) + " bytes of a chunk that was cut at " + std::to_string(c.cut));
        b.taxon.resize((size_t)C * R); b.classified.resize((size_t)C * R);
        fb.offs.resize(R + 1); b.hit_offs.resize(R + 1);
        fb.title_off.resize(R + 1);
        for (uint64_t r = 0; r < R; r++) fb.title_off[r + 1] = fb.title_off[r] + tlen[r];
        fb.titles.resize(fb.title_off[R]);
        for (uint64_t r = 0; r < R; r++) memcpy(&fb.titles[fb.title_off[r]], c.p + tpos[r], tlen[r]);
        total += R;
        order.deliver(ticket, [&] { f(std::shared_ptr<const ClassifiedBatch>(std::move(out))); });
      }
    } catch (...) {
      order.fail(std::current_exception());
    }
  };
  const char *wenv = getenv("SLK_CLASSIFY_THREADS");
  const size_t per_dev = std::max<size_t>(1, std::min<size_t>(8, wenv ? (size_t)atol(wenv) : 2));
  std::vector<Lane> lanes(per_dev * dev.ixs.size());
  for (size_t i = 0; i < lanes.size(); i++) {
    lanes[i].ix = dev.ixs[i % dev.ixs.size()];
    lanes[i].st = dev.st;
    if (i > 0) SLK_CALL(slk_stream_create(lanes[i].ix, &lanes[i].st));
    SLK_CALL(slk_stream_set_merged_hits(lanes[i].st, merged_hits && want_hits ? 1 : 0));
    SLK_CALL(slk_stream_set_split_long(lanes[i].st, dev.split_long));
    SLK_CALL(slk_stream_set_split_hits(lanes[i].st, dev.split_hits ? 1 : 0));
  }
  std::vector<std::thread> workers;
  for (size_t i = 1; i < lanes.size(); i++) workers.emplace_back([&work, &lanes, i] { work(lanes[i]); });
  work(lanes[0]);
  for (auto &t : workers) t.join();
  for (size_t i = 1; i < lanes.size(); i++) slk_stream_destroy(lanes[i].st);
  (void)slk_stream_set_merged_hits(dev.st, 0);
  (void)slk_stream_set_split_long(dev.st, -1);
  (void)slk_stream_set_split_hits(dev.st, 0);
  order.rethrow_failure();
  if (getenv("SLK_HOST_TIMING")) std::cerr << "host timing: " << n_batches << " chunks parsed on the device by " << lanes.size() << " classify thread(s)" << std::endl;
  std::cerr << total << " fragments" << std::endl;
}

// ---- --device-pairs: the device finds the records of both mate files and pairs them (slk_classify_text_paired) ----------
// Where the next chunk of either file starts is the device's answer -- it depends on how many leading records of the two chunks are
// mates --, so the calls of one file pair follow each other; several file pairs run side by side on different workers.

// The two texts of one file pair.  A plain file is mapped and advanced in place; a compressed file or a pipe goes through ByteSource
// into a pinned buffer, with what the call before left over in front.  A side takes new bytes only while it holds less than its
// target (the chunk size; doubled while a record does not fit), so the side that runs ahead in records does not grow without bound.
class PairedTextChunks {
 public:
  static constexpr size_t MAX_CHUNK = TextChunks::MAX_CHUNK;
  struct Side {
    std::string file;
    bool fastq = false, final = false;
    const char *p = nullptr;   // the chunk of the next call
    size_t n = 0;
   private:
    friend class PairedTextChunks;
    const char *map = nullptr;
    size_t map_len = 0, map_pos = 0, target = 0;
    bool mapped = false, eof = false;
    std::unique_ptr<ByteSource> src;
    PinnedText buf;
    size_t held = 0;   // bytes of buf in use
  };
 private:
  Side side_[2];
  const size_t chunk_ = io_chunk_bytes();

  void open(Side &s, const std::string &file) {
    s.file = file;
    s.fastq = RecordStream::is_fastq_name(file);
    s.target = chunk_;
    if (!TextChunks::plain_file(file)) { s.src = std::make_unique<ByteSource>(file); return; }
    s.mapped = true;
    const int fd = ::open(file.c_str(), O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) die("cannot open " + file);
    s.map_len = (size_t)sb.st_size;
    void *m = s.map_len ? mmap(nullptr, s.map_len, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (s.map_len && m == MAP_FAILED) die("cannot map " + file);
    if (s.map_len) madvise(m, s.map_len, MADV_SEQUENTIAL);
    s.map = (const char *)m;
  }
  void fill(Side &s) {
    if (s.mapped) {
      const size_t left = s.map_len - s.map_pos;
      s.n = std::min(s.target, left);
      s.final = s.n == left;
      static const char empty = 0;
      s.p = s.map ? s.map + s.map_pos : &empty;
      return;
    }
    while (!s.eof && s.held < s.target) {
      s.buf.ensure(s.target, s.held);
      const size_t got = s.src->read(s.buf.p + s.held, s.target - s.held);
      if (got == 0) s.eof = true;
      s.held += got;
    }
    s.buf.ensure(1, 0);
    s.p = s.buf.p;
    s.n = s.held;
    s.final = s.eof;
  }
 public:
  PairedTextChunks(const std::string &file1, const std::string &file2) { open(side_[0], file1); open(side_[1], file2); }
  PairedTextChunks(const PairedTextChunks &) = delete;
  ~PairedTextChunks() { for (Side &s : side_) if (s.map) munmap((void *)s.map, s.map_len); }
  Side &operator[](int i) { return side_[i]; }
  void fill() { fill(side_[0]); fill(side_[1]); }
  // after a call: side i starts `consumed` bytes further on; grow: no record of it fitted its chunk
  void advance(int i, size_t consumed, bool grow) {
    Side &s = side_[i];
    if (grow) {
      if (s.n >= MAX_CHUNK)
        die("a record of " + s.file + " does not fit the largest chunk the device parser takes (1 GiB): classify this input without --device-pairs");
      s.target = std::min(2 * std::max(s.n, chunk_), MAX_CHUNK);
    } else {
      s.target = chunk_;
    }
    if (s.mapped) { s.map_pos += consumed; return; }
    if (consumed) memmove(s.buf.p, s.buf.p + consumed, s.held - consumed);
    s.held -= consumed;
  }
};

// Results are handed on in a fixed rotation over the workers' slots, whichever worker is done first: slot 0's next batch, slot 1's
// next batch, ...; a slot whose file pairs are through leaves the rotation when its turn comes.  The order of the output follows from
// the input alone.
class RotatingHandOver {
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<char> alive_;
  size_t turn_ = 0;
  std::exception_ptr failure_;
  std::atomic<bool> failed_{false};
  void pass_on() {
    for (size_t k = 1; k <= alive_.size(); k++) {
      const size_t t = (turn_ + k) % alive_.size();
      if (alive_[t]) { turn_ = t; break; }
    }
    cv_.notify_all();
  }
 public:
  explicit RotatingHandOver(size_t slots) : alive_(slots, 1) {}
  bool failed() const { return failed_; }
  template <class Hand> void deliver(size_t slot, Hand hand) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return turn_ == slot || failure_; });
    if (!failure_) hand();
    pass_on();
  }
  void retire(size_t slot) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return turn_ == slot || failure_; });
    alive_[slot] = 0;
    pass_on();
  }
  void fail(std::exception_ptr e) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!failure_) failure_ = e;
    failed_ = true;
    cv_.notify_all();
  }
  void rethrow_failure() { if (failure_) std::rethrow_exception(failure_); }
};

// the title of the record that opens at text[at] (its '@' or '>', or a FASTA title at the very start of the text), for messages
inline std::string title_at(const char *text, size_t n, size_t at) {
  size_t a = at < n && (text[at] == '@' || text[at] == '>') ? at + 1 : at, b = a;
  while (b < n && text[b] != ' ' && text[b] != '\n' && text[b] != '\r') b++;
  return std::string(text + a, b - a);
}

// classify_stream for pairs of mate files with the records found and paired on the device: a replicated table, one id column (the
// command line refuses the rest).  A batch is what one call paired; its FragmentBatch holds offsets, mate offsets and the stripped
// titles, no bases.  The device route is the lockstep walk only: mates out of order end the run.
template <class F>
void classify_paired_text_stream(DeviceIndex &dev, const std::vector<std::string> &files, int min_hits, const std::vector<double> &thresholds,
                                 bool want_hits, F f, RepeatedTitles *rep = nullptr, bool merged_hits = false) {
  if (dev.sharded) die("internal: classify_paired_text_stream runs on a replicated table");
  const size_t npairs = files.size() / 2;
  const int C = (int)thresholds.size();
  std::atomic<size_t> total{0}, n_calls{0};
  struct Lane { slk_index *ix = nullptr; slk_stream *st = nullptr; };
  const char *wenv = getenv("SLK_CLASSIFY_THREADS");
  const size_t per_dev = std::max<size_t>(1, std::min<size_t>(8, wenv ? (size_t)atol(wenv) : 2));
  std::vector<Lane> lanes(std::max<size_t>(1, std::min(per_dev * dev.ixs.size(), npairs)));
  RotatingHandOver order(lanes.size());

  // file 2 is through: what file 1 still holds has no partner -- the inner join drops it, and its titles are kept in case one of them
  // is also a fragment's (seqio.hpp: FragmentSource, titles.hpp)
  auto drain_file1 = [&](const Lane &lane, PairedTextChunks &in) {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offs, tpos;
    std::vector<uint32_t> tlen;
    for (;;) {
      in.fill();
      PairedTextChunks::Side &a = in[0];
      if (a.n == 0 && a.final) return;
      uint64_t R = 0, nb = 0, consumed = 0;
      size_t rcap = a.n / 64 + 1024;
      bases.resize(a.n);
      for (int attempt = 0;; attempt++) {
        offs.resize(rcap + 1); tpos.resize(rcap); tlen.resize(rcap);
        const int32_t rc = slk_parse_text(lane.st, (const uint8_t *)a.p, a.n, a.fastq ? SLK_FORMAT_FASTQ : SLK_FORMAT_FASTA, a.final ? 1 : 0, bases.data(),
                                          offs.data(), tpos.data(), tlen.data(), bases.size(), rcap, &R, &nb, &consumed);
        if (rc == SLK_E_CAPACITY && attempt == 0 && R > rcap) { rcap = R; continue; }
        if (rc != SLK_OK) die(std::string("slk_parse_text: ") + slk_last_error());
        break;
      }
      if (rep) for (uint64_t r = 0; r < R; r++) rep->add_unmatched(title_hash(remove_suffix(std::string_view(a.p + tpos[r], tlen[r]), "/1")));
      in.advance(0, consumed, consumed == 0 && !a.final);
    }
  };

  auto one_pair = [&](const Lane &lane, size_t slot, const std::string &file1, const std::string &file2) {
    PairedTextChunks in(file1, file2);
    std::vector<int32_t> nd, tk;
    std::vector<uint64_t> tpos;
    std::vector<uint32_t> tlen;
    uint64_t done = 0;   // pairs of this file pair so far
    while (!order.failed()) {
      in.fill();
      PairedTextChunks::Side &a = in[0], &b2 = in[1];
      if (a.n == 0 && a.final) return;   // file 1 is through: what file 2 still holds is dropped
      if (b2.n == 0 && b2.final) { drain_file1(lane, in); return; }
      n_calls++;
      auto out = new_classified_batch();
      ClassifiedBatch &b = *out;
      b.frags = new_fragment_batch(1);
      b.C = C;
      FragmentBatch &fb = *b.frags;
      fb.paired = true;
      if (want_hits) b.reserve_hits(a.n + b2.n + 1);   // (a span per base at most, and a border per pair)
      slk_pair_record pr{};
      size_t rcap = std::max(a.n, b2.n) / 64 + 1024;   // records the arrays hold: a guess, and what the call asks for if the guess was short
      for (int attempt = 0;; attempt++) {
        b.taxon.resize((size_t)C * rcap); b.classified.resize((size_t)C * rcap); nd.resize(rcap); tk.resize(rcap);
        fb.offs.resize(rcap + 1); fb.mate_offs.resize(rcap + 1); tpos.resize(rcap); tlen.resize(rcap); b.hit_offs.resize(rcap + 1);
        const int32_t rc = slk_classify_text_paired(lane.ix, lane.st, (const uint8_t *)a.p, a.n, a.fastq ? SLK_FORMAT_FASTQ : SLK_FORMAT_FASTA, a.final ? 1 : 0,
                                                    (const uint8_t *)b2.p, b2.n, b2.fastq ? SLK_FORMAT_FASTQ : SLK_FORMAT_FASTA, b2.final ? 1 : 0, min_hits,
                                                    thresholds.data(), C, b.taxon.data(), b.classified.data(), nd.data(), tk.data(), fb.offs.data(),
                                                    fb.mate_offs.data(), tpos.data(), tlen.data(), b.hit_offs.data(), want_hits ? b.hits.get() : nullptr, rcap,
                                                    a.n + b2.n + 1, &pr);
        if (rc == SLK_E_CAPACITY && attempt == 0 && std::max(pr.records1, pr.records2) > rcap) { rcap = std::max(pr.records1, pr.records2); continue; }
        if (rc != SLK_OK) die(std::string("slk_classify_text_paired: ") + slk_last_error());
        break;
      }
      const uint64_t P = pr.pairs;
      if (pr.mismatch)
        die("mates out of order in " + a.file + " and " + b2.file + ": pair " + std::to_string(done + P + 1) + " has the titles '" +
            std::string(a.p + tpos[P], tlen[P]) + "' and '" + std::string(remove_suffix(title_at(b2.p, b2.n, pr.consumed2), "/2")) +
            "'; run without --device-pairs (the host route joins mates that are out of order)");
      if (pr.consumed1 > a.n || pr.consumed2 > b2.n) die("internal: the device consumed more than a chunk holds");
      if (P) {
        b.taxon.resize((size_t)C * P); b.classified.resize((size_t)C * P);
        fb.offs.resize(P + 1); fb.mate_offs.resize(P + 1); b.hit_offs.resize(P + 1);
        fb.title_off.resize(P + 1);
        fb.title_off[0] = 0;
        for (uint64_t r = 0; r < P; r++) fb.title_off[r + 1] = fb.title_off[r] + tlen[r];
        fb.titles.resize(fb.title_off[P]);
        for (uint64_t r = 0; r < P; r++) memcpy(&fb.titles[fb.title_off[r]], a.p + tpos[r], tlen[r]);
        total += P;
        done += P;
        order.deliver(slot, [&] { f(std::shared_ptr<const ClassifiedBatch>(std::move(out))); });
      }
      // a side without a record and without a consumed byte must grow, unless it is final (then it is through: the checks above)
      in.advance(0, pr.consumed1, pr.records1 == 0 && pr.consumed1 == 0 && !a.final);
      in.advance(1, pr.consumed2, pr.records2 == 0 && pr.consumed2 == 0 && !b2.final);
    }
  };
  auto work = [&](size_t slot) {
    try {
      for (size_t k = slot; k < npairs && !order.failed(); k += lanes.size()) one_pair(lanes[slot], slot, files[2 * k], files[2 * k + 1]);
      order.retire(slot);
    } catch (...) {
      order.fail(std::current_exception());
    }
  };
  for (size_t i = 0; i < lanes.size(); i++) {
    lanes[i].ix = dev.ixs[i % dev.ixs.size()];
    lanes[i].st = dev.st;
    if (i > 0) SLK_CALL(slk_stream_create(lanes[i].ix, &lanes[i].st));
    SLK_CALL(slk_stream_set_merged_hits(lanes[i].st, merged_hits && want_hits ? 1 : 0));
    SLK_CALL(slk_stream_set_split_long(lanes[i].st, dev.split_long));
    SLK_CALL(slk_stream_set_split_hits(lanes[i].st, dev.split_hits ? 1 : 0));
  }
  std::vector<std::thread> workers;
  for (size_t i = 1; i < lanes.size(); i++) workers.emplace_back([&work, i] { work(i); });
  work(0);
  for (auto &t : workers) t.join();
  for (size_t i = 1; i < lanes.size(); i++) slk_stream_destroy(lanes[i].st);
  (void)slk_stream_set_merged_hits(dev.st, 0);
  (void)slk_stream_set_split_long(dev.st, -1);
  (void)slk_stream_set_split_hits(dev.st, 0);
  order.rethrow_failure();
  if (getenv("SLK_HOST_TIMING")) std::cerr << "host timing: " << n_calls << " paired calls on " << lanes.size() << " classify thread(s)" << std::endl;
  std::cerr << total << " fragments" << std::endl;
}

}  // namespace slk_host
