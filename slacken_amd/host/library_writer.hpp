// library_writer.hpp -- a library written to disk in Slacken's layout: what KeyValueIndex.writeRecords (S/slacken/KeyValueIndex.scala:125-139),
// IndexParams.write (S/kmers/IndexParams.scala) with SplitterFormat.write (S/kmers/SplitterFormat.scala:42-64) and Taxonomy.copyToLocation
// leave at a location LOC:
//   LOC.properties   k, m, buckets, version, splitter=randomXOR, XORmask (signed decimal), canonical, minimizerSpaces
//   LOC_taxonomy/    a byte copy of the source library's directory
//   LOC/part-00000-<tag>_<bbbbb>.c000.snappy.parquet   one file per bucket, columns id1: int64, taxon: int32 (parquet_sink.cpp)
//   or LOC.slkrec    the flat form of library_io.hpp, when the build has no Arrow or the caller asks for it
// Host only, no GPU.  Records arrive in chunks (add), in any order.  Everything is written under temporary names and renamed by
// finish(), the properties last, and a library that is at LOC already is kept until then: a writer that dies or is destroyed before finish() returns leaves no LOC.properties, so nothing that
// loads.  Used by `build`, `respace` and `copy-records`.
#pragma once
#include <cstdint>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cli_common.hpp"
#include "parquet_source.hpp"

namespace slk_host {

// Where Spark puts a row of a table CLUSTERED BY (id1) INTO n BUCKETS -- the reference reopens the directory as such a table
// (KeyValueIndex.scala:150-159), so a row's file must be the bucket Spark computes for it: HashPartitioning's
// pmod(Murmur3Hash(id1), n), with Murmur3_x86_32.hashLong(value, seed 42) for a long column.  Spark's public algorithm, restated
// here; UNPINNED: no Spark runs beside this engine.
inline uint32_t spark_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
inline uint32_t spark_mix_k1(uint32_t k1) { k1 *= 0xcc9e2d51u; k1 = spark_rotl32(k1, 15); return k1 * 0x1b873593u; }
inline uint32_t spark_mix_h1(uint32_t h1, uint32_t k1) { h1 ^= k1; h1 = spark_rotl32(h1, 13); return h1 * 5u + 0xe6546b64u; }
inline int32_t spark_hash_long(int64_t v, uint32_t seed) {
  uint32_t h1 = spark_mix_h1(seed, spark_mix_k1((uint32_t)(uint64_t)v));
  h1 = spark_mix_h1(h1, spark_mix_k1((uint32_t)((uint64_t)v >> 32)));
  h1 ^= 8u;   // fmix(h1, length in bytes)
  h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
  return (int32_t)h1;
}
inline int spark_bucket(int64_t id1, int buckets) {
  const int r = spark_hash_long(id1, 42) % buckets;   // pmod
  return r < 0 ? r + buckets : r;
}

struct LibraryProperties {
  int k = 35, m = 31, spaces = 7, buckets = 1;
  uint64_t xorMask = 0;
  bool canonical = true;
};

// The Parquet half (parquet_sink.cpp, built with the flags of parquet_source.cpp): `buckets` files under dir, a row in the file of
// its spark_bucket.  Rows arrive grouped by bucket (add_grouped: group_offsets[0 .. buckets] says where each bucket's run starts, as
// slk_index_export_range leaves them; nothing is hashed) or in any order (add: dealt into groups on the host, then the same path).
// The buckets' writers are spread over `threads` host threads, a bucket always on the same one.  Without Arrow the constructor throws.
class ParquetBucketSink {
  struct Impl;
  std::unique_ptr<Impl> impl_;

 public:
  ParquetBucketSink(const std::string &dir, int buckets, const std::string &tag, size_t threads);
  ~ParquetBucketSink();
  void add(const int64_t *keys, const int32_t *taxa, uint64_t n);
  void add_grouped(const int64_t *keys, const int32_t *taxa, const uint64_t *group_offsets);
  void close();   // footers written, files complete
};

class LibraryWriter {
 public:
  enum Format { AUTO, PARQUET, SLKREC };
  static Format parse_format(const std::string &s) {
    if (s == "parquet") return PARQUET;
    if (s == "slkrec") return SLKREC;
    throw std::runtime_error("--format " + s + ": parquet or slkrec");
  }

  // taxonomy_dir: the directory that is copied to LOC_taxonomy
  LibraryWriter(const std::string &location, const LibraryProperties &props, const std::string &taxonomy_dir, Format format)
      : loc_(location), props_(props), tax_src_(taxonomy_dir), parquet_(format == PARQUET || (format == AUTO && parquet_available())) {
    namespace fs = std::filesystem;
    if (format == PARQUET && !parquet_available()) throw std::runtime_error("--format parquet: this build has no Parquet support");
    if (props_.buckets < 1) throw std::runtime_error("buckets=" + std::to_string(props_.buckets) + " in the properties");
    if (fs::path(loc_).has_parent_path()) fs::create_directories(fs::path(loc_).parent_path());
    tmp_ = loc_ + ".writing";
    fs::remove_all(tmp_);
    fs::remove_all(tmp_ + ".taxa");
    if (parquet_) {
      fs::create_directories(tmp_);
      sink_.reset(new ParquetBucketSink(tmp_, props_.buckets, "slacken-amd", host_threads()));
    } else {
      keys_ = fopen(tmp_.c_str(), "wb");
      taxa_ = fopen((tmp_ + ".taxa").c_str(), "w+b");
      if (!keys_ || !taxa_) throw std::runtime_error("cannot write " + tmp_);
      const char header[24] = {'S', 'L', 'K', 'R', 'E', 'C', '1', 0};   // n and the largest taxon follow in finish()
      put(keys_, header, sizeof header);
    }
  }
  LibraryWriter(const LibraryWriter &) = delete;
  ~LibraryWriter() {
    if (finished_) return;
    std::error_code ec;   // (no exceptions out of a destructor; what cannot be removed holds no properties and does not load)
    sink_.reset();
    if (keys_) fclose(keys_);
    if (taxa_) fclose(taxa_);
    std::filesystem::remove_all(tmp_, ec);
    std::filesystem::remove_all(tmp_ + ".taxa", ec);
  }

  void add(const int64_t *keys, const int32_t *taxa, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) if (taxa[i] > max_taxon_) max_taxon_ = taxa[i];
    n_ += n;
    if (parquet_) { sink_->add(keys, taxa, n); return; }
    put(keys_, keys, n * 8);
    put(taxa_, taxa, n * 4);
  }

  // records grouped by Spark's bucket (slk_index_export_range with n_groups = the properties' buckets): group_offsets[0 .. buckets],
  // group_offsets[buckets] records in all.  The flat form ignores the grouping.
  void add_grouped(const int64_t *keys, const int32_t *taxa, const uint64_t *group_offsets) {
    const uint64_t n = group_offsets[props_.buckets];
    if (!parquet_) { add(keys, taxa, n); return; }
    for (uint64_t i = 0; i < n; i++) if (taxa[i] > max_taxon_) max_taxon_ = taxa[i];
    n_ += n;
    sink_->add_grouped(keys, taxa, group_offsets);
  }
  bool parquet() const { return parquet_; }

  uint64_t records() const { return n_; }

  void finish() {
    namespace fs = std::filesystem;
    // Whatever library is at LOC is left alone until every record is on disk under its temporary name; it stops being one then
    // (its properties go first), its records are replaced, and the new properties come last.
    if (parquet_) {
      sink_->close();
      sink_.reset();
      fs::remove(loc_ + ".properties");
      fs::remove_all(loc_);
      fs::remove(loc_ + ".slkrec");   // (the readers prefer it: a stale one would hide the new records)
      fs::rename(tmp_, loc_);
    } else {
      // taxa behind the keys, then the header's counts
      std::vector<char> buf((size_t)1 << 22);
      if (fflush(taxa_) != 0 || fseeko(taxa_, 0, SEEK_SET) != 0) throw std::runtime_error("cannot write " + tmp_);
      for (size_t got; (got = fread(buf.data(), 1, buf.size(), taxa_)) > 0;) put(keys_, buf.data(), got);
      if (ferror(taxa_)) throw std::runtime_error("cannot read back " + tmp_ + ".taxa");
      const uint32_t W = 1, mt = (uint32_t)max_taxon_;
      if (fseeko(keys_, 8, SEEK_SET) != 0) throw std::runtime_error("cannot write " + tmp_);
      put(keys_, &n_, 8); put(keys_, &W, 4); put(keys_, &mt, 4);
      const bool ok = fclose(keys_) == 0;
      keys_ = nullptr;
      fclose(taxa_);
      taxa_ = nullptr;
      if (!ok) throw std::runtime_error("cannot write " + tmp_);
      fs::remove(tmp_ + ".taxa");
      fs::remove(loc_ + ".properties");
      fs::remove_all(loc_);
      fs::rename(tmp_, loc_ + ".slkrec");
    }
    if (fs::weakly_canonical(tax_src_) != fs::weakly_canonical(loc_ + "_taxonomy")) {
      fs::remove_all(loc_ + "_taxonomy");
      fs::copy(tax_src_, loc_ + "_taxonomy", fs::copy_options::recursive);
    }
    {
      std::ofstream f(loc_ + ".properties.writing");
      f << "#Properties for Slacken\n"
        << "k=" << props_.k << "\nm=" << props_.m << "\nbuckets=" << props_.buckets << "\nversion=1\nsplitter=randomXOR\nXORmask="
        << (int64_t)props_.xorMask << "\ncanonical=" << (props_.canonical ? "true" : "false") << "\nminimizerSpaces=" << props_.spaces << "\n";
      f.close();
      if (!f) throw std::runtime_error("cannot write " + loc_ + ".properties");
    }
    fs::rename(loc_ + ".properties.writing", loc_ + ".properties");
    finished_ = true;
  }

 private:
  void put(FILE *f, const void *p, size_t bytes) {
    if (bytes && fwrite(p, 1, bytes, f) != bytes) throw std::runtime_error("cannot write " + tmp_ + " (disk full?)");
  }
  std::string loc_, tmp_;
  LibraryProperties props_;
  std::string tax_src_;
  bool parquet_, finished_ = false;
  std::unique_ptr<ParquetBucketSink> sink_;
  FILE *keys_ = nullptr, *taxa_ = nullptr;
  uint64_t n_ = 0;
  int32_t max_taxon_ = 0;
};

}  // namespace slk_host
