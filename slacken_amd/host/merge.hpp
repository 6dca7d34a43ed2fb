// merge.hpp -- libraries united: the host side of `merge` and of `build --base`.  A record's taxon is the LCA of the
// taxa of all sequences that hold its minimizer (KeyValueIndex.makeRecords, S/slacken/KeyValueIndex.scala:85-93), and LCA is
// associative, commutative and idempotent: the records of two libraries under one taxonomy, merged per key by LCA
// (slk_index_merge_records), are the records of the library built from both sets of genomes.  Here: the translation of a source's
// taxa into the destination's taxonomy, what is refused from the .properties files alone, and the stream of a library's records
// from disk into a resident table.
#pragma once
#include "device_index.hpp"

namespace slk_host {

// For every node t that src defines: dst.primary[t] (dst's merged.dmp honoured) if dst defines that node, else 0 -- the table
// slk_index_set_merge_remap takes.  identity: every node of src is itself in dst, and no remap is needed.
struct TaxonRemap {
  std::vector<int32_t> map;   // src.size() entries
  bool identity = true;
};
inline TaxonRemap taxon_remap(const Taxonomy &src, const Taxonomy &dst) {
  TaxonRemap r;
  r.map.assign((size_t)src.size(), 0);
  for (Taxon t = 1; t < src.size(); t++) {
    if (!src.isDefined(t)) continue;
    Taxon p = t < dst.size() ? dst.primary[t] : NONE;
    if (p < 0 || p >= dst.size() || !dst.isDefined(p)) p = NONE;
    r.map[t] = p;
    if (p != t) r.identity = false;
  }
  return r;
}

// the splitter field in which two libraries differ, or null: what must agree before their records can share a table
inline const char *differing_splitter_field(const IndexParams &a, const IndexParams &b) {
  if (a.k != b.k) return "k";
  if (a.m != b.m) return "m";
  if (a.spaces != b.spaces) return "minimizerSpaces";
  if (a.xorMask != b.xorMask) return "XORmask";
  if (a.canonical != b.canonical) return "canonical";
  return nullptr;
}

// What `merge` refuses from the .properties files alone, before a device is opened and with nothing written; the sources' common
// parameters otherwise.
inline IndexParams check_merge_sources(const std::string &out, const std::vector<std::string> &sources) {
  namespace fs = std::filesystem;
  if (sources.size() < 2) die("merge needs two libraries at least");
  for (const std::string &s : sources)
    if (fs::weakly_canonical(s) == fs::weakly_canonical(out)) die("merge: OUT is the source " + s);
  const IndexParams ip = read_index_params(sources[0]);
  for (size_t i = 1; i < sources.size(); i++)
    if (const char *field = differing_splitter_field(ip, read_index_params(sources[i])))
      die("merge: " + sources[0] + " and " + sources[i] + " differ in " + field + ": their minimizers are not comparable");
  if (ip.m > 32) die("merge supports minimizers of up to 32 nt (these libraries have m=" + std::to_string(ip.m) + ")");
  return ip;
}

// the record count of a library where that is cheap to know (the Parquet footers, the flat file's header)
inline uint64_t library_record_count(const std::string &location, int W) {
  if (records_are_parquet(location)) { int64_t mt = -1; return parquet_count_rows(location, W, &mt); }
  return RecordFile(location, W).n;
}

// The records of the library at `location` merged into the table, their taxa translated from the library's own taxonomy
// (location_taxonomy) into dst_tax.  A taxon dst_tax lacks ends the run with the library's message.  Returns the records read.
inline uint64_t merge_library_into(DeviceIndex &dev, const std::string &location, const Taxonomy &dst_tax) {
  const Taxonomy src_tax = Taxonomy::load(location + "_taxonomy");
  const TaxonRemap remap = taxon_remap(src_tax, dst_tax);
  if (remap.identity) SLK_CALL(slk_index_set_merge_remap(dev.ix, nullptr, 0));
  else SLK_CALL(slk_index_set_merge_remap(dev.ix, remap.map.data(), (int32_t)remap.map.size()));
  uint64_t n = 0;
  for_each_record_batch(location, 1, [&](const int64_t *keys, const int32_t *taxa, uint64_t c) {
    if (slk_index_merge_records(dev.ix, keys, taxa, c) != SLK_OK) die(location + ": " + slk_last_error());
    n += c;
  });
  SLK_CALL(slk_index_set_merge_remap(dev.ix, nullptr, 0));
  return n;
}

}  // namespace slk_host
