// migration.hpp -- what MinimizerMigration.run (S/slacken/analysis/MinimizerMigration.scala:68-84) makes of the (t1, t2, steps)
// triples: the histogram of steps as Dataset.show() prints it, and the Kraken report of the taxa whose minimizers went to ROOT or
// "cellular organisms".  Header only, no GPU: `compare-index` feeds it the device's triples, `migration-report` a text file.
#pragma once
#include <cstdint>
#include <map>
#include <ostream>
#include <string>
#include <vector>

#include "stats.hpp"
#include "taxonomy.hpp"

namespace slk_host {

constexpr Taxon CELLULAR_ORGANISMS = 131567;   // MinimizerMigration.scala:74

// steps of one pair (:51-64); depth = Taxonomy.depth of the REFERENCE's taxonomy (bcTax, :42), -1 for ids it does not have
inline int32_t migration_steps(const Taxonomy &reference, Taxon t1, Taxon t2) {
  const int l1 = reference.depth(t1), l2 = reference.depth(t2);
  return l1 == -1 ? -100 : l2 == -1 ? -200 : l1 - l2;
}

// groupBy("steps").agg(count("steps")).sort("steps").show() (:70-72) in show()'s layout (stats.hpp: show_table).  At most 19 step
// values exist, so show()'s cut at 20 rows never applies.
inline std::string steps_histogram_text(const std::vector<int32_t> &steps, const std::vector<uint64_t> &count) {
  std::map<int32_t, uint64_t> hist;
  for (size_t i = 0; i < steps.size(); i++) hist[steps[i]] += count[i];
  std::vector<std::vector<std::string>> rows;
  for (auto &e : hist) rows.push_back({std::to_string(e.first), std::to_string(e.second)});
  return show_table({"steps", "count(steps)"}, rows);
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
