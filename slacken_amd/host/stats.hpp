// stats.hpp -- what `stats` and `inspect` print without a genome library, from the (taxon, records) pairs of an index
// (slk_index_taxon_counts) and its taxonomy: KeyValueIndex.showIndexStats(None) (S/slacken/KeyValueIndex.scala:240-251),
// kmerDepthHistogram / taxonDepthHistogram (:326-336) as Dataset.show() prints them, and report(labels, output, None) (:274-306).
// Header only, no GPU: `stats` and `inspect` feed it the device's pairs, `stats-report` a text file.  The only place that formats.
#pragma once
#include <cstdint>
#include <map>
#include <ostream>
#include <set>
#include <string>
#include <vector>

#include "taxonomy.hpp"

namespace slk_host {

using TaxonCounts = std::vector<std::pair<Taxon, uint64_t>>;   // distinct taxa, ascending

// Dataset.show() (Dataset.showString with numRows = 20, truncate = 20): right-aligned cells as wide as the column's widest entry
// (at least 3), rules above the header, below it and after the last row, and the empty line show()'s println leaves.  The caller
// has at most 20 rows (and no cell beyond 20 characters), so show()'s cuts never apply.
inline std::string show_table(const std::vector<std::string> &head, const std::vector<std::vector<std::string>> &rows) {
  std::vector<size_t> width(head.size());
  for (size_t c = 0; c < head.size(); c++) {
    width[c] = std::max<size_t>(3, head[c].size());
    for (auto &r : rows) width[c] = std::max(width[c], r[c].size());
  }
  std::string rule = "+";
  for (size_t w : width) rule += std::string(w, '-') + "+";
  rule += "\n";
  auto line = [&](const std::vector<std::string> &r) {
    std::string s = "|";
    for (size_t c = 0; c < head.size(); c++) s += std::string(width[c] - r[c].size(), ' ') + r[c] + "|";
    return s + "\n";
  };
  std::string out = rule + line(head) + rule;
  for (auto &r : rows) out += line(r);
  return out + rule + "\n";
}

// formatPerc (S/kmers/package.scala:60): "%.2f%%".format(d * 100), Java's rounding (taxonomy.hpp); 0.0 / 0 prints as Java's NaN
inline std::string format_perc(double num, double den) {
  if (den == 0) return "NaN%";
  const std::string s = java_format_6_2f(num / den * 100);
  return s.substr(s.find_first_not_of(' ')) + "%";
}

// An id outside the taxonomy's arrays (the reference would throw) is a leaf without ancestors, of depth -1.
inline bool stats_is_leaf(const Taxonomy &tax, Taxon t) { return t < 0 || t >= tax.size() || tax.children()[t].empty(); }   // Taxonomy.isLeafNode :171

// Taxonomy.countDistinctTaxaWithAncestors (:295, taxaWithAncestors :307-311): every path stops at the first taxon already seen
inline uint64_t stats_tree_size(const Taxonomy &tax, const TaxonCounts &counts) {
  std::set<Taxon> seen;
  for (auto &tc : counts)
    for (Taxon t = tc.first; t != NONE && seen.insert(t).second;) t = (t > 0 && t < tax.size()) ? tax.parents[t] : NONE;
  return seen.size();
}

// showIndexStats(None) :240-251
inline std::string index_stats_text(const Taxonomy &tax, const TaxonCounts &counts, int m) {
  uint64_t leaves = 0, records = 0, leaf_records = 0;
  for (auto &tc : counts) {
    records += tc.second;
    if (stats_is_leaf(tax, tc.first)) { leaves++; leaf_records += tc.second; }
  }
  return "Tree size: " + std::to_string(stats_tree_size(tax, counts)) + " taxa, stored taxa: " + std::to_string(counts.size()) +
         ", of which " + std::to_string(leaves) + " leaf taxa (" + format_perc((double)leaves, (double)counts.size()) + ")\n" +
         "Total " + std::to_string(m) + "-minimizers: " + std::to_string(records) + ", of which leaf records: " +
         std::to_string(leaf_records) + " (" + format_perc((double)leaf_records, (double)records) + ")\n";
}

// kmerDepthHistogram (by_records) / taxonDepthHistogram :326-336: depth, rank, count sorted by depth.  Depths are -1 .. 8: at most
// 10 rows, so show()'s cut at 20 rows never applies.  numericalRankToStrUdf (GenomeLibrary.scala:63-65) looks the depth up among
// root .. species only: -1 (a taxon without a ranked ancestor) is "???", not "unclassified".
inline std::string depth_histogram_text(const Taxonomy &tax, const TaxonCounts &counts, bool by_records) {
  std::map<int, uint64_t> hist;
  for (auto &tc : counts) hist[tax.depth(tc.first)] += by_records ? tc.second : 1;
  std::vector<std::vector<std::string>> rows;
  for (auto &e : hist)
    rows.push_back({std::to_string(e.first), e.first >= 0 && e.first <= 8 ? rank_titles(e.first + 1) : "???", std::to_string(e.second)});
  return show_table({"depth", "rank", "count"}, rows);
}

// what `stats` prints after the splitter lines (Slacken.scala:304-312)
inline std::string stats_text(const Taxonomy &tax, const TaxonCounts &counts, int m, bool histogram) {
  if (!histogram) return index_stats_text(tax, counts, m);
  return "Minimizer depth histogram\n" + depth_histogram_text(tax, counts, true) + "Taxon depth histogram\n" +
         depth_histogram_text(tax, counts, false);
}

// new KrakenReport(taxonomy, counts).print.  Without counts the reference divides 0 by 0 and Java prints the root's share as NaN.
inline void stats_print_report(const Taxonomy &tax, const std::vector<std::pair<Taxon, long>> &counts, std::ostream &out) {
  if (counts.empty()) {
    out << "#Perc\tAggregate\tIn taxon\tRank\tTaxon\tName\n   NaN\t0\t0\tR\t1\t" << (tax.has_name[ROOT] ? tax.names[ROOT] : "") << '\n';
    return;
  }
  KrakenReport(tax, counts).print(out);
}

// report(labels, output, None) :274-306: records per taxon, and one "genome" per stored taxon
inline void write_min_report(const Taxonomy &tax, const TaxonCounts &counts, std::ostream &out) {
  std::vector<std::pair<Taxon, long>> c;
  for (auto &tc : counts) c.emplace_back(tc.first, (long)tc.second);
  stats_print_report(tax, c, out);
}
inline void write_genome_report(const Taxonomy &tax, const TaxonCounts &counts, std::ostream &out) {
  std::vector<std::pair<Taxon, long>> c;
  for (auto &tc : counts) c.emplace_back(tc.first, 1L);
  stats_print_report(tax, c, out);
}

// GenomeLibrary.getTaxonLabels (GenomeLibrary.scala:74-78): seqid \t taxon lines; the distinct taxa.  A line whose second column is
// no number is skipped (Spark's cast gives null there).
inline std::set<Taxon> read_label_taxa(std::istream &in) {
  std::set<Taxon> taxa;
  std::string line;
  while (std::getline(in, line)) {
    const size_t tab = line.find('\t');
    if (tab == std::string::npos) continue;
    const std::string f = trim(line.substr(tab + 1, line.find('\t', tab + 1) - tab - 1));
    char *end = nullptr;
    const long v = strtol(f.c_str(), &end, 10);
    if (f.empty() || *end != '\0' || v < 0 || v > INT32_MAX) continue;
    taxa.insert((Taxon)v);
  }
  return taxa;
}
// the label taxa that are not stored, one each (:297-304)
inline void write_missing_report(const Taxonomy &tax, const TaxonCounts &counts, const std::set<Taxon> &label_taxa, std::ostream &out) {
  std::set<Taxon> present;
  for (auto &tc : counts) present.insert(tc.first);
  std::vector<std::pair<Taxon, long>> c;
  for (Taxon t : label_taxa) if (!present.count(t)) c.emplace_back(t, 1L);
  stats_print_report(tax, c, out);
}

}  // namespace slk_host
