// coverage.hpp -- the `coverage` command: a genome library's minimizers counted against a resident index (slk_coverage_*), and what
// is written from the counts.  Mirrors (S/ = src/main/scala/com/jnpersson/ in the reference):
//   IndexStatistics.showTaxonFullCoverageStats     S/slacken/IndexStatistics.scala:86-111  (the two coverage files, written as
//                                                  Dynamic.reportDynamicIndexSupport writes them, S/slacken/Dynamic.scala:230-241)
//   IndexStatistics.totalKmerCountReport           :38-52
//   TotalKmerCountReport, TotalKmerSizeAggregator  :114-222
// The formatting is host only (`coverage-report` feeds it text files); the counting is the device's.
#pragma once
#include <cmath>
#include <map>
#include <ostream>
#include <string>
#include <unordered_map>
#include <vector>

#include "cli_common.hpp"
#include "device_index.hpp"
#include "library_io.hpp"
#include "stats.hpp"
#include "taxonomy.hpp"

namespace slk_host {

// TotalKmerSizeAggregator (:130-222): the same tree walk, the same order of additions.  genomeSizes: k-mers per source taxon, one
// entry per labelled taxon (also those without a k-mer, and those the taxonomy lacks: nobody asks for them).
struct TotalKmerSizeAggregator {
  const Taxonomy &tax;
  std::map<Taxon, long> genomeSizes;
  std::vector<std::pair<long, long>> tree;   // computedTreeMap: (sum of genome sizes, genomes) in the subtree

  TotalKmerSizeAggregator(const Taxonomy &t, const std::vector<std::pair<Taxon, uint64_t>> &sizes) : tax(t), tree(t.parents.size(), {0, 0}) {
    for (auto &s : sizes) genomeSizes[s.first] = (long)s.second;
    // computeLeafAggAndCounts(ROOT) :193-219 without the recursion: children before their parent
    std::vector<Taxon> order{ROOT};
    for (size_t i = 0; i < order.size(); i++)
      for (Taxon c : tax.children()[order[i]]) order.push_back(c);
    for (size_t i = order.size(); i-- > 0;) {
      const Taxon x = order[i];
      long size = 0, count = 0;
      auto own = genomeSizes.find(x);
      if (own != genomeSizes.end()) { size += own->second; count += 1; }
      for (Taxon c : tax.children()[x]) { size += tree[c].first; count += tree[c].second; }
      tree[x] = {size, count};
    }
  }
  const std::vector<Taxon> &children(Taxon t) const { return tax.children()[t]; }

  double s1(Taxon t) const {   // totKmerAverageS1 :140-148
    std::pair<long, long> agg = tree[t];
    if (!children(t).empty()) {
      agg = {0, 0};
      for (Taxon c : children(t)) { agg.first += tree[c].first; agg.second += tree[c].second; }
    }
    auto own = genomeSizes.find(t);
    if (own != genomeSizes.end()) { agg.first += own->second; agg.second += 1; }
    return (double)agg.first / (double)agg.second;
  }
  double s2(Taxon t) const {   // totKmerAverageS2 :156-167
    if (children(t).empty()) return tree[t].second == 0 ? 0.0 : (double)tree[t].first / (double)tree[t].second;
    double sum = 0.0;   // (List.sum: from the left, the taxon's own genome first)
    size_t n = 0;
    auto own = genomeSizes.find(t);
    if (own != genomeSizes.end()) { sum += (double)own->second; n++; }
    for (Taxon c : children(t))
      if (tree[c].second > 0) { sum += (double)tree[c].first / (double)tree[c].second; n++; }
    return sum / (double)n;
  }
  double s3(Taxon t) const {   // totKmerAverageS3 :175-185
    std::pair<long, long> agg{0, 0};
    size_t nonzero = 0;
    for (Taxon c : children(t))
      if (tree[c].second > 0) { agg.first += tree[c].first; agg.second += tree[c].second; nonzero++; }
    if (nonzero == 0) agg = tree[t];
    const double nz = (double)nonzero;
    if ((double)agg.second + nz == 0) return 0.0;
    return ((s1(t) * (double)agg.second) + (s2(t) * nz)) / ((double)agg.second + nz);
  }
};

// java.lang.Math.round(double): floor(x + 1/2) computed exactly, NaN -> 0
inline long java_round(double x) {
  if (std::isnan(x)) return 0;
  const double f = std::floor(x);
  return (long)f + (x - f >= 0.5 ? 1 : 0);
}

// OUTPUT_min_report.txt of `coverage`: new TotalKmerCountReport(taxonomy, records per taxon, k-mers per source).print (:114-128)
inline void write_total_kmer_count_report(const Taxonomy &tax, const TaxonCounts &records, const std::vector<std::pair<Taxon, uint64_t>> &sizes,
                                          std::ostream &out) {
  const TotalKmerSizeAggregator agg(tax, sizes);
  std::vector<std::pair<Taxon, long>> c;
  for (auto &tc : records) c.emplace_back(tc.first, (long)tc.second);
  KrakenReport rep(tax, c);
  rep.extraHeaders = "\tTKC1-LeafOnly\tTKC2-FirstChildren\tTKC3-AllChildren";
  rep.extraColumns = [&agg](Taxon t) {
    return "\t" + std::to_string(java_round(agg.s1(t))) + "\t" + std::to_string(java_round(agg.s2(t))) + "\t" + std::to_string(java_round(agg.s3(t)));
  };
  rep.print(out);
}

struct CoverageRow { int32_t source, depth; uint64_t all, distinct; };

// OUTPUT_support_report_minimizerCoverage.txt / ..DistinctCoverage.txt (Dynamic.scala:233-241): "<taxon>  <d>:<c>|<d>:<c>..", one line
// per source that has a row.  Spark leaves the order of the lines and of collect_list's entries (:104-106) unspecified; sources
// ascending and depths ascending is this engine's choice.  rows: sorted by source then depth (slk_coverage_result).
inline void write_coverage_lines(const std::vector<CoverageRow> &rows, std::ostream &all, std::ostream &distinct) {
  for (size_t i = 0; i < rows.size();) {
    size_t j = i;
    all << rows[i].source << "  ";
    distinct << rows[i].source << "  ";
    for (; j < rows.size() && rows[j].source == rows[i].source; j++) {
      all << (j > i ? "|" : "") << rows[j].depth << ':' << rows[j].all;
      distinct << (j > i ? "|" : "") << rows[j].depth << ':' << rows[j].distinct;
    }
    all << '\n';
    distinct << '\n';
    i = j;
  }
}

inline void write_coverage_files(const Taxonomy &tax, const TaxonCounts &records, const std::vector<std::pair<Taxon, uint64_t>> &sizes,
                                 const std::vector<CoverageRow> &rows, const std::string &output) {
  std::ofstream f1 = open_output(output + "_support_report_minimizerCoverage.txt");
  std::ofstream f2 = open_output(output + "_support_report_minimizerDistinctCoverage.txt");
  write_coverage_lines(rows, f1, f2);
  std::ofstream f3 = open_output(output + "_min_report.txt");
  write_total_kmer_count_report(tax, records, sizes, f3);
}

struct CoverageOptions {
  std::string index, library, output;
  std::vector<int> devices{0};
};

// The sources in groups whose (minimizer, source) pairs fit the budget together: ascending, filled greedily.  need: windows per
// source taxon, max(0, length - k + 1) summed over its sequences -- a bound on its pairs.
inline std::unordered_map<Taxon, int> coverage_groups(const std::map<Taxon, uint64_t> &need, uint64_t budget, int *n_groups) {
  std::unordered_map<Taxon, int> group_of;
  int g = 0;
  uint64_t used = 0;
  for (auto &e : need) {
    if (e.second > budget)
      die("coverage: taxon " + std::to_string(e.first) + " alone needs " + std::to_string(e.second) + " (minimizer, source) pairs, the budget is " +
          std::to_string(budget) + " (SLK_COVERAGE_MAX_PAIRS, or the device's free memory)");
    if (used + e.second > budget) { g++; used = 0; }
    used += e.second;
    group_of[e.first] = g;
  }
  *n_groups = need.empty() ? 1 : g + 1;
  return group_of;
}

// walk(fn): every labelled sequence of the library, fn(sequence, taxon), in the same order every time
template <class Walk>
int coverage_run(const CoverageOptions &o, Walk walk) {
  const double t0 = wall_seconds();
  const IndexParams ip0 = read_index_params(o.index);
  // planning pass, host only: what every source taxon can need
  std::map<Taxon, uint64_t> need;
  walk([&](std::string_view sq, Taxon taxon) {
    if (taxon == NONE) return;
    need[taxon] += sq.size() >= (size_t)ip0.k ? sq.size() - ip0.k + 1 : 0;
  });
  const long env_pairs = getenv("SLK_COVERAGE_MAX_PAIRS") ? atol(getenv("SLK_COVERAGE_MAX_PAIRS")) : 0;
  int n_groups = 1;
  if (env_pairs > 0) (void)coverage_groups(need, (uint64_t)env_pairs, &n_groups);   // (a source too large stops the run before the library is loaded)

  LoadedIndex lib(o.index, o.devices);
  std::vector<int32_t> depths(lib.tax.size());
  for (Taxon t = 0; t < lib.tax.size(); t++) depths[t] = lib.tax.depth(t);
  slk_coverage *cv = nullptr;
  SLK_CALL(slk_coverage_create(lib.dev.ix, depths.data(), (int32_t)depths.size(), env_pairs > 0 ? (uint64_t)env_pairs : 0, &cv));
  const std::unordered_map<Taxon, int> group_of = coverage_groups(need, slk_coverage_budget(cv), &n_groups);

  // One pass over the library per group, in batches of whole sequences as `build` takes them; a pass hands over the sequences of its
  // group's sources only.  Every labelled sequence belongs to one group, so it goes through slk_coverage_add exactly once and the
  // per-source totals are complete after the last pass: no pass needs to see the others' sequences for them.
  const long env_batch = getenv("SLK_BUILD_BATCH_BASES") ? atol(getenv("SLK_BUILD_BATCH_BASES")) : 0;
  const uint64_t batch_bases = env_batch > 0 ? (uint64_t)env_batch : (uint64_t)1 << 30;
  struct Batch {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets{0};
    std::vector<int32_t> taxa;
    void clear() { bases.clear(); offsets.assign(1, 0); taxa.clear(); }
  } b;
  uint64_t n_seq = 0;
  auto submit = [&] {
    if (b.taxa.empty()) return;
    SLK_CALL(slk_coverage_add(cv, lib.dev.st, b.bases.data(), b.offsets.data(), b.taxa.data(), b.taxa.size()));
    b.clear();
  };
  for (int g = 0; g < n_groups; g++) {
    walk([&](std::string_view sq, Taxon taxon) {
      if (taxon == NONE || group_of.at(taxon) != g) return;
      n_seq++;
      if (!b.taxa.empty() && b.bases.size() + sq.size() > batch_bases) submit();
      b.bases.insert(b.bases.end(), sq.begin(), sq.end());
      b.offsets.push_back(b.bases.size());
      b.taxa.push_back(taxon);
    });
    submit();
    SLK_CALL(slk_coverage_fold(cv, lib.dev.st));
  }

  uint64_t n = 0, ns = 0;
  SLK_CALL(slk_coverage_result(cv, &n, nullptr, nullptr, nullptr, nullptr, 0));
  std::vector<int32_t> source(n), depth(n), tsource;
  std::vector<uint64_t> all(n), distinct(n), kmers, supermers;
  if (n) SLK_CALL(slk_coverage_result(cv, &n, source.data(), depth.data(), all.data(), distinct.data(), n));
  SLK_CALL(slk_coverage_totals(cv, &ns, nullptr, nullptr, nullptr, 0));
  tsource.resize(ns); kmers.resize(ns); supermers.resize(ns);
  if (ns) SLK_CALL(slk_coverage_totals(cv, &ns, tsource.data(), kmers.data(), supermers.data(), ns));
  slk_coverage_destroy(cv);

  std::vector<CoverageRow> rows(n);
  uint64_t matched = 0, total_kmers = 0, total_supermers = 0;
  for (uint64_t i = 0; i < n; i++) { rows[i] = {source[i], depth[i], all[i], distinct[i]}; matched += all[i]; }
  std::vector<std::pair<Taxon, uint64_t>> sizes(ns);
  for (uint64_t i = 0; i < ns; i++) { sizes[i] = {tsource[i], kmers[i]}; total_kmers += kmers[i]; total_supermers += supermers[i]; }
  write_coverage_files(lib.tax, device_taxon_counts(lib.dev.ix), sizes, rows, o.output);
  std::cout << "coverage: " << n_seq << " sequences, " << ns << " source taxa, " << total_kmers << " k-mers, " << total_supermers
            << " super-mers, " << matched << " matched super-mers, " << n_groups << " groups, " << wall_seconds() - t0 << " s" << std::endl;
  return 0;
}

}  // namespace slk_host
