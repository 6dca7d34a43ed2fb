// library_io.hpp -- a library on disk as the command-line host reads it (S/ = src/main/scala/com/jnpersson/ of the reference):
//   index params     S/kmers/IndexParams.scala:30-47, S/kmers/SplitterFormat.scala:42-64 (<idx>.properties)
//   records          the Parquet table (id1: int64, taxon: int32), read natively (parquet_source.cpp) or, converted once by
//                    tools/parquet_to_slkrec.py, from the flat <idx>.slkrec
//   labels           S/slacken/GenomeLibrary.scala (<library>/seqid2taxid.map)
#pragma once
#include <cstring>
#include <map>

#include "cli_common.hpp"
#include "library_writer.hpp"
#include "parquet_source.hpp"
#include "seqio.hpp"
#include "taxonomy.hpp"

namespace slk_host {

// ---- Java .properties (the subset HDFSUtil.writeProperties produces) ----
inline std::map<std::string, std::string> read_properties(const std::string &path) {
  std::ifstream f = open_input(path);
  std::map<std::string, std::string> p;
  std::string line;
  while (std::getline(f, line)) {
    line = trim(line);
    if (line.empty() || line[0] == '#' || line[0] == '!') continue;
    size_t eq = line.find_first_of("=:");
    if (eq == std::string::npos) continue;
    std::string k = trim(line.substr(0, eq)), v = trim(line.substr(eq + 1));
    std::string u;
    for (size_t i = 0; i < v.size(); i++) { if (v[i] == '\\' && i + 1 < v.size()) i++; u.push_back(v[i]); }
    p[k] = u;
  }
  return p;
}

struct IndexParams { int k, m, spaces; uint64_t xorMask; bool canonical; };
inline IndexParams read_index_params(const std::string &location) {  // IndexParams.read + RandomXORFormat.read + decorate
  auto p = read_properties(location + ".properties");
  auto get = [&](const char *k, const char *def) { auto it = p.find(k); return it == p.end() ? std::string(def ? def : "") : it->second; };
  if (!p.count("k") || !p.count("m") || !p.count("version")) die("Unable to read index parameters for " + location);
  if (std::stoi(get("version", "1")) > 1) die("A newer version of this software is needed to read " + location);
  std::string splitter = get("splitter", "standard");
  if (splitter != "randomXOR") die("splitter '" + splitter + "' is not supported by this engine (randomXOR only)");
  IndexParams ip;
  ip.k = std::stoi(get("k", nullptr));
  ip.m = std::stoi(get("m", nullptr));
  ip.spaces = std::stoi(get("minimizerSpaces", "0"));
  ip.xorMask = p.count("XORmask") ? (uint64_t)std::stoll(get("XORmask", nullptr)) : SLK_DEFAULT_TOGGLE_MASK;  // signed decimal long
  ip.canonical = get("canonical", "true") == "true";
  return ip;
}

// the properties a library derived from `location` is written with (buckets: the source's; a source without the key is one bucket)
inline LibraryProperties writer_properties(const std::string &location, const IndexParams &ip) {
  const auto p = read_properties(location + ".properties");
  LibraryProperties lp;
  lp.k = ip.k; lp.m = ip.m; lp.spaces = ip.spaces; lp.xorMask = ip.xorMask; lp.canonical = ip.canonical;
  lp.buckets = p.count("buckets") ? std::stoi(p.at("buckets")) : 1;
  return lp;
}

// ---- records (<idx>.slkrec written by tools/parquet_to_slkrec.py) ----
// <idx>.slkrec: "SLKREC1\0", u64 n, u32 id columns W, u32 largest taxon (0 = not recorded), int64 keys[n][W], int32 taxa[n].
// Streamed into the device table in chunks: a standard library is ~120 GB of records, which must not need as much host memory.
struct RecordFile {
  FILE *f = nullptr;
  std::string path;
  uint64_t n = 0;
  uint32_t max_taxon = 0, id_columns = 1;
  RecordFile(const std::string &location, int expect_columns) : path(location + ".slkrec") {
    f = fopen(path.c_str(), "rb");
    if (!f) die("cannot open " + path + " (this build reads Parquet " + (parquet_available() ? "natively, but " + location + "/ holds no *.parquet" : "only through tools/parquet_to_slkrec.py " + location) + ")");
    char magic[8];
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "SLKREC1", 8) != 0) die(path + ": bad magic");
    if (fread(&n, 8, 1, f) != 1 || fread(&id_columns, 4, 1, f) != 1 || fread(&max_taxon, 4, 1, f) != 1) die(path + ": truncated header");
    if ((int)id_columns != expect_columns)
      die(path + ": " + std::to_string(id_columns) + " id columns, the index parameters imply " + std::to_string(expect_columns));
  }
  ~RecordFile() { if (f) fclose(f); }
  void read_at(uint64_t off, void *dst, size_t bytes) {
    if (fseeko(f, (off_t)off, SEEK_SET) != 0 || fread(dst, 1, bytes, f) != bytes) die(path + ": truncated");
  }
  static constexpr uint64_t CHUNK = 1ull << 24;
  template <class F> void for_each_chunk(bool with_keys, F fn) {  // fn(keys or null, taxa, count)
    const uint64_t W = id_columns;
    std::vector<int64_t> keys(with_keys ? std::min(n, CHUNK) * W : 0);
    std::vector<int32_t> taxa(std::min(n, CHUNK));
    for (uint64_t o = 0; o < n; o += CHUNK) {
      uint64_t c = std::min(CHUNK, n - o);
      if (with_keys) read_at(24 + o * 8 * W, keys.data(), c * 8 * W);
      read_at(24 + n * 8 * W + o * 4, taxa.data(), c * 4);
      fn(with_keys ? keys.data() : nullptr, taxa.data(), c);
    }
  }
};

// records: the flat <idx>.slkrec if it exists, else Slacken's Parquet table itself
inline bool records_are_parquet(const std::string &location) {
  return !std::filesystem::exists(location + ".slkrec") && parquet_available() && std::filesystem::is_directory(location);
}
template <class F> void for_each_record_batch(const std::string &location, int W, F fn) {  // fn(keys, taxa, count), one chunk in host memory
  if (records_are_parquet(location)) parquet_for_each_batch(location, W, fn);
  else RecordFile(location, W).for_each_chunk(true, fn);
}

// GenomeLibrary.getTaxonLabels: <library>/seqid2taxid.map, TSV header \t taxon, in the file's order (the callers filter)
inline std::vector<std::pair<std::string, Taxon>> read_label_map(const std::string &library) {
  std::ifstream lf = open_input(library + "/seqid2taxid.map");
  std::vector<std::pair<std::string, Taxon>> labels;
  std::string l;
  while (std::getline(lf, l)) {
    size_t tab = l.find('\t');
    if (tab == std::string::npos) continue;
    labels.emplace_back(l.substr(0, tab), (Taxon)std::stoi(l.substr(tab + 1)));
  }
  return labels;
}

}  // namespace slk_host
