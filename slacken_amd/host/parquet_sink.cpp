// parquet_sink.cpp -- the Parquet half of library_writer.hpp: one snappy-compressed file per bucket, columns id1: int64 and
// taxon: int32, through parquet::arrow of the Arrow C++ libraries inside the pyarrow wheel.  Built like parquet_source.cpp: with
// -std=c++20 and only when the Makefile finds those libraries; otherwise the stubs at the bottom are compiled.
#include "library_writer.hpp"

#ifdef SLK_HAVE_PARQUET
#include <arrow/api.h>
#include <arrow/io/file.h>
#include <parquet/arrow/writer.h>
#include <parquet/exception.h>
#include <parquet/properties.h>

namespace slk_host {

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
};

ParquetBucketSink::ParquetBucketSink(const std::string &dir, int buckets, const std::string &tag) : impl_(new Impl()) {
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
}

ParquetBucketSink::~ParquetBucketSink() = default;

void ParquetBucketSink::add(const int64_t *keys, const int32_t *taxa, uint64_t n) {
  const int nb = (int)impl_->buckets.size();
  for (uint64_t i = 0; i < n; i++) {
    Impl::Bucket &b = impl_->buckets[(size_t)spark_bucket(keys[i], nb)];
    b.keys.push_back(keys[i]);
    b.taxa.push_back(taxa[i]);
    if (b.taxa.size() >= Impl::FLUSH_ROWS) impl_->flush(b);
  }
}

void ParquetBucketSink::close() {
  for (Impl::Bucket &b : impl_->buckets) {
    impl_->flush(b);
    PARQUET_THROW_NOT_OK(b.writer->Close());
    b.writer.reset();
  }
}

}  // namespace slk_host

#else

namespace slk_host {
struct ParquetBucketSink::Impl {};
ParquetBucketSink::ParquetBucketSink(const std::string &, int, const std::string &) { throw std::runtime_error("built without Parquet support"); }
ParquetBucketSink::~ParquetBucketSink() = default;
void ParquetBucketSink::add(const int64_t *, const int32_t *, uint64_t) {}
void ParquetBucketSink::close() {}
}  // namespace slk_host

#endif
