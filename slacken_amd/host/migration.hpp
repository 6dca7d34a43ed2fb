// migration.hpp -- what MinimizerMigration.run (S/slacken/analysis/MinimizerMigration.scala:68-84) makes of the (t1, t2, steps)
// triples: the histogram of steps as Dataset.show() prints it, and the Kraken report of the taxa whose minimizers went to ROOT or
// "cellular organisms".  Header only, no GPU: `compare-index` feeds it the device's triples, `migration-report` a text file.
#pragma once
#include <cstdint>
#include <map>
#include <ostream>
#include <string>
#include <vector>

#include "taxonomy.hpp"

namespace slk_host {

constexpr Taxon CELLULAR_ORGANISMS = 131567;   // MinimizerMigration.scala:74

// steps of one pair (:51-64); depth = Taxonomy.depth of the REFERENCE's taxonomy (bcTax, :42), -1 for ids it does not have
inline int32_t migration_steps(const Taxonomy &reference, Taxon t1, Taxon t2) {
  const int l1 = reference.depth(t1), l2 = reference.depth(t2);
  return l1 == -1 ? -100 : l2 == -1 ? -200 : l1 - l2;
}

// groupBy("steps").agg(count("steps")).sort("steps").show() (:70-72): right-aligned cells as wide as the column's widest entry (at
// least 3), rules above the header, below it and after the last row, and the empty line show()'s println leaves.  At most 19 step
// values exist, so show()'s cut at 20 rows never applies.
inline std::string steps_histogram_text(const std::vector<int32_t> &steps, const std::vector<uint64_t> &count) {
  std::map<int32_t, uint64_t> hist;
  for (size_t i = 0; i < steps.size(); i++) hist[steps[i]] += count[i];
  const std::string head[2] = {"steps", "count(steps)"};
  std::vector<std::string> cells[2];
  size_t width[2] = {std::max<size_t>(3, head[0].size()), std::max<size_t>(3, head[1].size())};
  for (auto &e : hist) {
    cells[0].push_back(std::to_string(e.first));
    cells[1].push_back(std::to_string(e.second));
    for (int c = 0; c < 2; c++) width[c] = std::max(width[c], cells[c].back().size());
  }
  const std::string rule = "+" + std::string(width[0], '-') + "+" + std::string(width[1], '-') + "+\n";
  auto row = [&](const std::string &a, const std::string &b) {
    return "|" + std::string(width[0] - a.size(), ' ') + a + "|" + std::string(width[1] - b.size(), ' ') + b + "|\n";
  };
  std::string out = rule + row(head[0], head[1]) + rule;
  for (size_t i = 0; i < cells[0].size(); i++) out += row(cells[0][i], cells[1][i]);
  return out + rule + "\n";
}

// t1 -> records of the pairs that moved into {ROOT, cellular organisms} from outside it (:77-79)
inline std::vector<std::pair<Taxon, long>> taxa_to_root(const std::vector<int32_t> &t1, const std::vector<int32_t> &t2,
                                                        const std::vector<uint64_t> &count) {
  auto top = [](Taxon t) { return t == ROOT || t == CELLULAR_ORGANISMS; };
  std::map<Taxon, long> sum;
  for (size_t i = 0; i < t1.size(); i++)
    if (top(t2[i]) && !top(t1[i])) sum[t1[i]] += (long)count[i];
  return std::vector<std::pair<Taxon, long>>(sum.begin(), sum.end());
}

// run (:68-84): the table to `table`, the report with the SUBJECT's taxonomy (index.bcTaxonomy, :82) to `report`
inline void write_migration(const Taxonomy &subject, const std::vector<int32_t> &t1, const std::vector<int32_t> &t2,
                            const std::vector<int32_t> &steps, const std::vector<uint64_t> &count, std::ostream &table,
                            std::ostream &report) {
  table << steps_histogram_text(steps, count);
  KrakenReport(subject, taxa_to_root(t1, t2, count)).print(report);
}

}  // namespace slk_host
