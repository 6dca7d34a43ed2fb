// parquet_sink.cpp -- the Parquet half of library_writer.hpp: one snappy-compressed file per bucket, columns id1: int64 and
// taxon: int32, written by a pool of host threads that share the buckets out, through parquet::arrow of the Arrow C++ libraries inside the pyarrow wheel.  Built like parquet_source.cpp: with
// -std=c++20 and only when the Makefile finds those libraries; otherwise the stubs at the bottom are compiled.
#include "library_writer.hpp"

#ifdef SLK_HAVE_PARQUET
#include <arrow/api.h>
#include <arrow/io/file.h>
#include <parquet/arrow/writer.h>
#include <parquet/exception.h>
#include <parquet/properties.h>

#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>

namespace slk_host {

// The buckets' writers are spread over a pool of host threads: bucket b is always served by thread b mod T, so no writer and no
// bucket buffer is shared, and the calls (add_grouped, close) hand every thread its buckets and wait for all of them.
struct ParquetBucketSink::Impl {
  static constexpr uint64_t FLUSH_ROWS = 1ull << 20;   // a bucket's rows become a row group at this many (and at close)
  struct Bucket {
    std::string path;
    std::unique_ptr<parquet::arrow::FileWriter> writer;
    std::vector<int64_t> keys;
    std::vector<int32_t> taxa;
  };
  std::shared_ptr<arrow::Schema> schema = arrow::schema({arrow::field("id1", arrow::int64()), arrow::field("taxon", arrow::int32())});
  std::vector<Bucket> buckets;

  // the pool: run(f) calls f(t) on every thread t and returns when all are done
  std::vector<std::thread> threads;
  std::mutex mu;
  std::condition_variable wake, done;
  const std::function<void(size_t)> *job = nullptr;
  uint64_t generation = 0;
  size_t running = 0;
  bool stop = false;
  std::exception_ptr error;

  size_t n_threads() const { return threads.size() + 1; }
  void serve(size_t t, const std::function<void(size_t)> &f) {   // f(t): thread t's share of a call
    try {
      f(t);
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      if (!error) error = std::current_exception();
    }
  }
  // f(bucket) for every bucket, each on the bucket's own thread
  void run_buckets(const std::function<void(size_t)> &f) {
    run([&](size_t t) { for (size_t b = t; b < buckets.size(); b += n_threads()) f(b); });
  }
  void worker(size_t t) {
    uint64_t seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      wake.wait(lk, [&] { return stop || generation != seen; });
      if (stop) return;
      seen = generation;
      const std::function<void(size_t)> *f = job;
      lk.unlock();
      serve(t, *f);
      lk.lock();
      if (--running == 0) done.notify_all();
    }
  }
  void start(size_t n_threads) {   // (the calling thread is thread 0)
    for (size_t t = 1; t < n_threads; t++) threads.emplace_back([this, t] { worker(t); });
  }
  void run(const std::function<void(size_t)> &f) {
    {
      std::lock_guard<std::mutex> lk(mu);
      job = &f; running = threads.size(); generation++;
    }
    wake.notify_all();
    serve(0, f);
    std::unique_lock<std::mutex> lk(mu);
    done.wait(lk, [&] { return running == 0; });
    job = nullptr;
    if (error) { std::exception_ptr e = error; error = nullptr; std::rethrow_exception(e); }
  }
  ~Impl() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    wake.notify_all();
    for (auto &t : threads) t.join();
  }

  void flush(Bucket &b) {
    if (b.taxa.empty()) return;
    arrow::Int64Builder kb;
    arrow::Int32Builder tb;
    std::shared_ptr<arrow::Array> ka, ta;
    PARQUET_THROW_NOT_OK(kb.AppendValues(b.keys.data(), (int64_t)b.keys.size()));
    PARQUET_THROW_NOT_OK(tb.AppendValues(b.taxa.data(), (int64_t)b.taxa.size()));
    PARQUET_THROW_NOT_OK(kb.Finish(&ka));
    PARQUET_THROW_NOT_OK(tb.Finish(&ta));
    PARQUET_THROW_NOT_OK(b.writer->WriteTable(*arrow::Table::Make(schema, {ka, ta}), (int64_t)b.taxa.size()));
    b.keys.clear();
    b.taxa.clear();
  }
  // a run of rows of one bucket, appended without hashing; row groups of FLUSH_ROWS rows as they fill
  void append(Bucket &b, const int64_t *keys, const int32_t *taxa, uint64_t n) {
    while (n) {
      const uint64_t take = std::min<uint64_t>(n, FLUSH_ROWS - b.taxa.size());
      b.keys.insert(b.keys.end(), keys, keys + take);
      b.taxa.insert(b.taxa.end(), taxa, taxa + take);
      keys += take; taxa += take; n -= take;
      if (b.taxa.size() >= FLUSH_ROWS) flush(b);
    }
  }
};

ParquetBucketSink::ParquetBucketSink(const std::string &dir, int buckets, const std::string &tag, size_t threads) : impl_(new Impl()) {
  const auto props = parquet::WriterProperties::Builder().compression(parquet::Compression::SNAPPY)->build();
  impl_->buckets.resize((size_t)buckets);
  for (int b = 0; b < buckets; b++) {
    char name[64];
    snprintf(name, sizeof name, "_%05d.c000.snappy.parquet", b);   // (Spark reads the bucket from the digits behind the last '_')
    Impl::Bucket &bk = impl_->buckets[(size_t)b];
    bk.path = dir + "/part-00000-" + tag + name;
    PARQUET_ASSIGN_OR_THROW(auto out, arrow::io::FileOutputStream::Open(bk.path));
    PARQUET_ASSIGN_OR_THROW(bk.writer, parquet::arrow::FileWriter::Open(*impl_->schema, arrow::default_memory_pool(), out, props));
  }
  impl_->start(std::max<size_t>(1, std::min<size_t>(threads, (size_t)buckets)));
}

ParquetBucketSink::~ParquetBucketSink() = default;

void ParquetBucketSink::add_grouped(const int64_t *keys, const int32_t *taxa, const uint64_t *group_offsets) {
  impl_->run_buckets([&](size_t b) {
    impl_->append(impl_->buckets[b], keys + group_offsets[b], taxa + group_offsets[b], group_offsets[b + 1] - group_offsets[b]);
  });
}

// rows in any order: dealt into groups here (a stable counting sort by spark_bucket, so a bucket's rows keep their order of arrival;
// the pool's threads take a slice of the rows each),
// then the grouped path
void ParquetBucketSink::add(const int64_t *keys, const int32_t *taxa, uint64_t n) {
  const size_t nb = impl_->buckets.size();
  static const bool serial = getenv("SLK_WRITER_SERIAL") != nullptr && getenv("SLK_WRITER_SERIAL")[0] == '1';
  if (serial) {   // (A/B switch of tools/bench_build.py: rows dealt out one at a time and written on this thread, as it was before add_grouped)
    for (uint64_t i = 0; i < n; i++) {
      Impl::Bucket &b = impl_->buckets[(size_t)spark_bucket(keys[i], (int)nb)];
      b.keys.push_back(keys[i]);
      b.taxa.push_back(taxa[i]);
      if (b.taxa.size() >= Impl::FLUSH_ROWS) impl_->flush(b);
    }
    return;
  }
  // every thread of the pool takes a slice of the rows: the slices' histograms, one prefix sum over (bucket, slice), the scatter
  const size_t T = impl_->n_threads();
  std::unique_ptr<uint32_t[]> group(new uint32_t[n]);
  std::unique_ptr<int64_t[]> gk(new int64_t[n]);
  std::unique_ptr<int32_t[]> gt(new int32_t[n]);
  std::vector<uint64_t> offsets(nb + 1, 0), at(T * nb, 0);
  auto slice = [&](size_t t) { return n * t / T; };
  impl_->run([&](size_t t) {
    uint64_t *mine = at.data() + t * nb;
    for (uint64_t i = slice(t); i < slice(t + 1); i++) mine[group[i] = (uint32_t)spark_bucket(keys[i], (int)nb)]++;
  });
  uint64_t run = 0;
  for (size_t b = 0; b < nb; b++) {
    offsets[b] = run;
    for (size_t t = 0; t < T; t++) { const uint64_t c = at[t * nb + b]; at[t * nb + b] = run; run += c; }
  }
  offsets[nb] = run;
  impl_->run([&](size_t t) {
    uint64_t *mine = at.data() + t * nb;
    for (uint64_t i = slice(t); i < slice(t + 1); i++) {
      const uint64_t slot = mine[group[i]]++;
      gk[slot] = keys[i];
      gt[slot] = taxa[i];
    }
  });
  add_grouped(gk.get(), gt.get(), offsets.data());
}

void ParquetBucketSink::close() {
  impl_->run_buckets([&](size_t i) {
    Impl::Bucket &b = impl_->buckets[i];
    impl_->flush(b);
    PARQUET_THROW_NOT_OK(b.writer->Close());
    b.writer.reset();
  });
}

}  // namespace slk_host

#else

namespace slk_host {
struct ParquetBucketSink::Impl {};
ParquetBucketSink::ParquetBucketSink(const std::string &, int, const std::string &, size_t) { throw std::runtime_error("built without Parquet support"); }
ParquetBucketSink::~ParquetBucketSink() = default;
void ParquetBucketSink::add(const int64_t *, const int32_t *, uint64_t) {}
void ParquetBucketSink::add_grouped(const int64_t *, const int32_t *, const uint64_t *) {}
void ParquetBucketSink::close() {}
}  // namespace slk_host

#endif
