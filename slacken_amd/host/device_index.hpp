// device_index.hpp -- the device-side index as the command-line host sees it: the tables of --devices, the library loaded into
// them (KeyValueIndex.load, S/slacken/KeyValueIndex.scala:413-426), and what runs on every replica of them (Bracken weights).
#pragma once
#include <deque>

#include "cli_common.hpp"
#include "library_io.hpp"
#include "output.hpp"
#include "stats.hpp"

namespace slk_host {

// f(i), an slk_* call, for every replica i < n, each on a thread of its own: the code and the text of the first that failed
// (slk_last_error is per thread, so the text is taken where the call was made)
struct ReplicaError { int32_t code = SLK_OK; std::string text; };
template <class F> ReplicaError on_replicas(size_t n, F f) {
  std::vector<ReplicaError> res(n);
  std::vector<std::thread> th;
  for (size_t i = 0; i < n; i++)
    th.emplace_back([&, i] { if ((res[i].code = f(i)) != SLK_OK) res[i].text = slk_last_error(); });
  for (auto &t : th) t.join();
  for (auto &r : res) if (r.code != SLK_OK) return r;
  return {};
}

// The table is REPLICATED on every device of --devices and the reads are shared out between them batch by batch (SURVEY 8e;
// the reference's counterpart is the fan-out of the span rows over the partitions, KeyValueIndex.scala:169-172): there is
// no exchange between devices, only the host-side merge of the per-taxon counts that the report is made of.  The same
// device may be listed more than once (two tables on it): that is how the multi-device path is tested on a one-GPU box.
// --shard-table (BASELINE configs[3]): a library whose table does not fit one GPU is SPREAD over the devices
// instead -- device i keeps the records whose minimizer falls to it (slk_index_set_shard; every device is handed the whole record
// stream and drops the rest), and the batches are classified in rounds of one batch per device by slk_shardset_classify: minimizers
// travel to their owners and taxa back (RCCL, or copies when devices repeat).  The output is byte for byte that of the other mode.
struct DeviceIndex {
  std::vector<slk_index *> ixs;   // one per device of the list
  slk_index *ix = nullptr;        // = ixs[0]
  slk_stream *st = nullptr;       // a stream on ixs[0]
  std::vector<int> devices{0};
  bool sharded = false;
  std::vector<slk_shardset *> sets;   // sharded: the rounds of several host threads overlap, each on a set (streams, buffers) of its own
  std::string last_error;             // of add_sequences
  int64_t split_long = -1;            // classify --split-long: what every classify worker's stream is told (slk_stream_set_split_long)
  bool split_hits = false;            // classify --split-hits: likewise (slk_stream_set_split_hits)
  ~DeviceIndex() { reset(); }
  void reset() {
    for (slk_shardset *s : sets) slk_shardset_destroy(s);
    sets.clear();
    if (st) slk_stream_destroy(st);
    for (slk_index *i : ixs) slk_index_destroy(i);
    ixs.clear(); st = nullptr; ix = nullptr;
  }
  // slk_classify_batch on this library, whichever way it is laid out (single caller: the passes after the stream of batches)
  void classify_one(const uint8_t *bases, const uint64_t *offs, const uint8_t *mb, const uint64_t *mo, uint64_t n, int min_hits,
                    const double *thr, int C, int32_t *taxon, uint8_t *cls, int32_t *nd, int32_t *tk, uint64_t *hit_offs, slk_hit *hits, uint64_t cap) {
    if (!sharded) {
      SLK_CALL(slk_classify_batch(ix, st, bases, offs, mb, mo, n, min_hits, thr, C, taxon, cls, nd, tk, hit_offs, hits, cap));
      return;
    }
    std::vector<slk_shard_batch> round(ixs.size(), slk_shard_batch{});
    round[0] = slk_shard_batch{bases, offs, mb, mo, n, taxon, cls, nd, tk, hit_offs, hits, cap};
    SLK_CALL(slk_shardset_classify(sets[0], round.data(), min_hits, thr, C));
  }
  void create(const IndexParams &ip, const Taxonomy &tax, uint64_t expected_records, int32_t max_taxon) {
    slk_params sp{ip.k, ip.m, ip.spaces, ip.canonical ? 1 : 0, ip.xorMask, (ip.m + 31) / 32, 0};
    // (sharded: a device's share of the records, with room for the hash's unevenness)
    const uint64_t share = sharded ? expected_records / devices.size() + expected_records / (4 * devices.size()) + 4096 : expected_records;
    slk_table_config cfg{share, max_taxon, 0.0f};
    std::vector<int32_t> parents(tax.parents.begin(), tax.parents.end());
    if (max_taxon + 1 > (int32_t)parents.size()) parents.resize(max_taxon + 1, 0);
    for (int d : devices) {
      slk_index *one = nullptr;
      SLK_CALL(slk_index_create(&sp, &cfg, d, &one));
      if (sharded) SLK_CALL(slk_index_set_shard(one, (uint32_t)ixs.size(), (uint32_t)devices.size()));
      ixs.push_back(one);
      SLK_CALL(slk_index_set_taxonomy(one, parents.data(), (int32_t)parents.size()));
    }
    ix = ixs[0];
  }
  void append(const int64_t *keys, const int32_t *taxa, uint64_t n) {
    if (ixs.size() == 1) { SLK_CALL(slk_index_append(ix, keys, taxa, n)); return; }
    const ReplicaError e = on_replicas(ixs.size(), [&](size_t i) { return slk_index_append(ixs[i], keys, taxa, n); });
    if (e.code != SLK_OK) die(e.text);
  }
  // (every replica builds the same records: the result does not depend on insertion order)
  int32_t add_sequences(const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa, uint64_t n) {
    const ReplicaError e = on_replicas(ixs.size(), [&](size_t i) { return slk_index_add_sequences(ixs[i], bases, offsets, taxa, n); });
    if (e.code != SLK_OK) last_error = e.text;
    return e.code;
  }
  void finalize() {
    for (slk_index *i : ixs) SLK_CALL(slk_index_finalize(i));
    SLK_CALL(slk_stream_create(ix, &st));
    if (!sharded) return;
    // Two sets (two host threads whose rounds overlap) where the exchange is copies; ONE where it is RCCL's: several
    // communicators over the same devices, driven by threads that do not agree on an order, are NCCL / RCCL's documented way
    // into a deadlock (the library serialises its grouped calls besides), and no multi-device run has measured a gain from two.
    const char *e = getenv("SLK_SHARD_SETS");
    auto add_set = [&] {
      slk_shardset *s = nullptr;
      SLK_CALL(slk_shardset_create(ixs.data(), (int32_t)ixs.size(), SLK_EXCHANGE_AUTO, &s));
      sets.push_back(s);
    };
    add_set();
    const bool rccl = slk_shardset_exchange_mode(sets[0]) == SLK_EXCHANGE_RCCL;
    const size_t n_sets = std::max<size_t>(1, std::min<size_t>(4, e ? (size_t)atol(e) : (rccl ? 1 : 2)));
    while (sets.size() < n_sets) add_set();
    std::cerr << "table sharded over " << ixs.size() << " device table(s), exchange by " << (rccl ? "RCCL" : "device-to-device copies") << std::endl;
  }
};

// The Parquet table into the device table: bucket files are decoded on several threads (whole files: a bucket file of a standard
// library is ~60 MB) and appended here in file order.  Returns the number of records.
inline uint64_t load_parquet_records(const std::string &location, int W, const IndexParams &ip, const Taxonomy &tax, DeviceIndex &dev) {
  const bool timing = getenv("SLK_HOST_TIMING") != nullptr;
  int64_t mt = -1;
  const double tl0 = wall_seconds();
  const uint64_t n_records = parquet_count_rows(location, W, &mt);
  const double tl1 = wall_seconds();
  int32_t max_taxon = std::max<int32_t>(tax.size() - 1, (int32_t)std::max<int64_t>(mt, 0));
  if (mt < 0)  // no column statistics: one pass over the taxon column
    for_each_record_batch(location, W, [&](const int64_t *, const int32_t *taxa, uint64_t c) { for (uint64_t i = 0; i < c; i++) max_taxon = std::max(max_taxon, taxa[i]); });
  dev.create(ip, tax, n_records, max_taxon);
  if (timing) std::cerr << "host timing: library load: footers of the bucket files " << tl1 - tl0 << " s, device table " << wall_seconds() - tl1 << " s\n";
  struct FileRecords { std::vector<int64_t> keys; std::vector<int32_t> taxa; };
  ThreadPool pool(host_threads());
  std::deque<std::future<FileRecords>> pending;
  double t_wait = 0, t_append = 0;
  auto drain_one = [&]() {
    const double t0 = wall_seconds();
    FileRecords fr = pending.front().get();
    pending.pop_front();
    const double t1 = wall_seconds();
    dev.append(fr.keys.data(), fr.taxa.data(), fr.taxa.size());
    t_wait += t1 - t0; t_append += wall_seconds() - t1;
  };
  for (auto &file : parquet_list_files(location)) {
    pending.push_back(pool.submit([file, W]() {
      FileRecords fr;
      parquet_read_file(file, W, [&](const int64_t *keys, const int32_t *taxa, uint64_t c) {
        fr.keys.insert(fr.keys.end(), keys, keys + c * W);
        fr.taxa.insert(fr.taxa.end(), taxa, taxa + c);
      });
      return fr;
    }));
    while (pending.size() >= 2 * pool.size()) drain_one();
  }
  while (!pending.empty()) drain_one();
  if (timing) std::cerr << "host timing: library load: waiting for decoded bucket files " << t_wait << " s, appending them to the table " << t_append << " s (" << pool.size() << " decoding threads)\n";
  return n_records;
}

// KeyValueIndex.load (KeyValueIndex.scala:413-426): parameters, taxonomy and records into HBM
inline void load_index(const std::string &location, IndexParams &ip, Taxonomy &tax, DeviceIndex &dev) {
  Timer t("Load index " + location);
  ip = read_index_params(location);
  tax = Taxonomy::load(location + "_taxonomy");
  const int W = (ip.m + 31) / 32;   // id columns (KeyValueIndex.scala:49)
  uint64_t n_records = 0;
  if (records_are_parquet(location)) {
    n_records = load_parquet_records(location, W, ip, tax, dev);
  } else {
    RecordFile rec(location, W);
    n_records = rec.n;
    int32_t max_taxon = std::max<int32_t>(tax.size() - 1, (int32_t)rec.max_taxon);
    if (rec.max_taxon == 0)  // an older file without the recorded maximum: one pass over the taxon column
      rec.for_each_chunk(false, [&](const int64_t *, const int32_t *taxa, uint64_t c) { for (uint64_t i = 0; i < c; i++) max_taxon = std::max(max_taxon, taxa[i]); });
    dev.create(ip, tax, rec.n, max_taxon);
    for_each_record_batch(location, W, [&](const int64_t *keys, const int32_t *taxa, uint64_t c) { dev.append(keys, taxa, c); });
  }
  const double tf0 = wall_seconds();
  dev.finalize();
  if (getenv("SLK_HOST_TIMING")) std::cerr << "host timing: library load: finalize " << wall_seconds() - tf0 << " s\n";
  std::cerr << "index: " << n_records << " records, k=" << ip.k << " m=" << ip.m << " spaces=" << ip.spaces << std::endl;
}

// a library loaded onto the devices of a list
struct LoadedIndex {
  IndexParams ip;
  Taxonomy tax;
  DeviceIndex dev;
  LoadedIndex(const std::string &location, const std::vector<int> &devices, bool sharded = false) {
    dev.devices = devices; dev.sharded = sharded; load_index(location, ip, tax, dev);
  }
};

// the (taxon, records) pairs of the resident table, counted on the device
inline TaxonCounts device_taxon_counts(const slk_index *ix) {
  uint64_t n = 0, records = 0;
  SLK_CALL(slk_index_taxon_counts(ix, nullptr, nullptr, 0, &n, &records));
  std::vector<int32_t> taxa(n);
  std::vector<uint64_t> counts(n);
  if (n) SLK_CALL(slk_index_taxon_counts(ix, taxa.data(), counts.data(), n, &n, &records));
  TaxonCounts out(n);
  for (uint64_t i = 0; i < n; i++) out[i] = {taxa[i], counts[i]};
  return out;
}

// ---- Bracken weights (S/slacken/BrackenWeights.scala) for bracken-build and classify2 --bracken-length ----
// Records arrive one by one (add_record) and go to the devices in batches of one engine batch per replica; within a batch, record r
// goes to replica r mod n of --devices, and each replica adds its share on a thread of its own (bracken.hip).  Host memory holds one
// batch at a time.  finish() sums the replicas' triples into the kmer_distrib file.
class BrackenRun {
  std::vector<slk_stream *> st_;
  std::vector<slk_bracken *> b_;
  std::vector<uint8_t> bases_;          // the batch being filled
  std::vector<uint64_t> offsets_{0};
  std::vector<int32_t> taxa_;
  uint64_t n_seq_ = 0, n_bases_ = 0;

  void add(const std::vector<uint8_t> &bases, const std::vector<uint64_t> &offsets, const std::vector<int32_t> &taxa) {
    const size_t n = b_.size();
    const ReplicaError e = on_replicas(n, [&](size_t g) -> int32_t {
      std::vector<uint8_t> bb;
      std::vector<uint64_t> oo(1, 0);
      std::vector<int32_t> tt;
      const uint8_t *base = bases.data();
      const uint64_t *off = offsets.data();
      const int32_t *tx = taxa.data();
      size_t R = taxa.size();
      if (n > 1) {   // this replica's records
        for (size_t r = g; r < taxa.size(); r += n) {
          bb.insert(bb.end(), bases.begin() + offsets[r], bases.begin() + offsets[r + 1]);
          oo.push_back(bb.size());
          tt.push_back(taxa[r]);
        }
        base = bb.data(); off = oo.data(); tx = tt.data(); R = tt.size();
      }
      return R ? slk_bracken_add(b_[g], st_[g], base, off, tx, R) : SLK_OK;
    });
    if (e.code != SLK_OK) die("slk_bracken_add: " + e.text);
  }

 public:
  static constexpr uint64_t BATCH_BYTES = 1ULL << 30;   // per replica: one engine batch (bracken.hip: batch_bytes)
  BrackenRun(DeviceIndex &dev, int read_len) : st_(dev.ixs.size(), nullptr), b_(dev.ixs.size(), nullptr) {
    for (size_t g = 0; g < dev.ixs.size(); g++) {
      SLK_CALL(slk_stream_create(dev.ixs[g], &st_[g]));
      SLK_CALL(slk_bracken_create(dev.ixs[g], read_len, 0, &b_[g]));
    }
  }
  ~BrackenRun() {
    for (slk_bracken *b : b_) slk_bracken_destroy(b);
    for (slk_stream *s : st_) if (s) slk_stream_destroy(s);
  }
  uint64_t sequences() const { return n_seq_; }
  uint64_t bases() const { return n_bases_; }
  // one record, its bases without whitespace (regexp_replace, BrackenWeights.scala:311); a full batch goes to the devices
  void add_record(std::string_view sq, int32_t taxon) {
    for (char ch : sq) if (!isspace((unsigned char)ch)) bases_.push_back((uint8_t)ch);
    n_seq_++; n_bases_ += bases_.size() - offsets_.back();
    offsets_.push_back(bases_.size());
    taxa_.push_back(taxon);
    if (bases_.size() >= BATCH_BYTES * b_.size()) flush();
  }
  void flush() {   // what is left of the last batch: once, after the last record
    add(bases_, offsets_, taxa_);
    bases_.clear(); offsets_.assign(1, 0); taxa_.clear();
  }
  void finish(const std::string &out_file) {
    std::vector<int32_t> d, s;
    std::vector<uint64_t> c;
    for (slk_bracken *b : b_) {
      uint64_t m = 0;
      SLK_CALL(slk_bracken_result(b, &m, nullptr, nullptr, nullptr, 0));
      const size_t at = d.size();
      d.resize(at + m); s.resize(at + m); c.resize(at + m);
      SLK_CALL(slk_bracken_result(b, &m, d.data() + at, s.data() + at, c.data() + at, m));
    }
    open_output(out_file) << kmer_distrib_text(d, s, c);
    std::cerr << "wrote " << out_file << std::endl;
  }
};

}  // namespace slk_host
