// support.hpp -- the `support` command and the counts behind `classify2 -C` / `-D`: a sample's minimizers counted per taxon against a
// resident index (slk_support_*), and what is written from the counts.  Mirrors (S/ = src/main/scala/com/jnpersson/ in the reference):
//   Dynamic.minimizersInSubjects, totalMinimizersPerTaxon, distinctMinimizersPerTaxon   S/slacken/Dynamic.scala:95-117
//   Dynamic.multiStatsPerTaxon                                                           :152-180
//   Dynamic.reportDynamicIndexSupport, the four KrakenReports                            :210-228
// The options, the views of a batch's reads and the reports are host only; the counting is the device's.
#pragma once
#include <future>
#include <ostream>
#include <string>
#include <vector>

#include "classify_stream.hpp"
#include "cli_common.hpp"
#include "device_index.hpp"
#include "seqio.hpp"
#include "taxonomy.hpp"

namespace slk_host {

inline const char *SUPPORT_USAGE = "usage: support -i INDEX -o OUTPUT [--rank RANK (species)] [--min-hits N] [-p] [--devices D] FILES...";

struct SupportOptions {
  std::string index, output, rank = "species";
  int min_hits = 2, rank_depth = 8;
  bool paired = false;
  std::vector<int> devices{0};
  std::vector<std::string> files;
};

// the command line of `support`; every usage error ends the program here, before a library is read or a device is opened
inline SupportOptions parse_support_options(int argc, char **argv) {
  SupportOptions o;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") o.index = a.next();
    else if (a == "-o" || a == "--output") o.output = a.next();
    else if (a == "--rank") o.rank = a.next();
    else if (a == "--min-hits") o.min_hits = std::stoi(a.next());
    else if (a == "-p" || a == "--paired") o.paired = true;
    else if (a == "--devices") o.devices = parse_device_list(a.next());
    else if (a == "--shard-table") refuse_shard_table("support", "the library's table must fit one GPU", SUPPORT_USAGE);
    else if (a.opt.size() > 1 && a.opt[0] == '@') {
      std::ifstream lf(a.opt.substr(1));
      std::string l;
      while (std::getline(lf, l)) if (!trim(l).empty()) o.files.push_back(trim(l));
    }
    else if (!a.opt.empty() && a.opt[0] == '-') die("unknown option " + a.opt + "\n" + SUPPORT_USAGE);
    else o.files.push_back(a.opt);
  }
  if (o.index.empty() || o.output.empty() || o.files.empty()) die(SUPPORT_USAGE);
  const int rank = rank_index(o.rank);   // Taxonomy.rankOrNull
  if (rank == NO_RANK) die("unknown rank " + o.rank);
  o.rank_depth = rank - 1;
  if (o.paired && o.files.size() % 2 != 0)
    die("For paired end mode, please supply pairs of files (even number). " + std::to_string(o.files.size()) + " files were supplied");
  return o;
}

// The pass counts on ONE device: `distinct` does not add up across replicas (a minimizer seen by two of them would count twice), and
// a replica's cell positions are its own.  The pass is bound by parsing on the host, not by the device (classify_stream.hpp).
inline void note_one_support_device(const std::vector<int> &devices) {
  if (devices.size() > 1)
    std::cerr << "the support pass counts on one device: device " << devices[0] << ", the first of the " << devices.size() << " named by --devices" << std::endl;
}

// A batch's reads as slk_support_add takes them: the first mates, and the second mates as sequences of their own.
struct SequenceSet { const uint8_t *bases; const uint64_t *offsets; uint64_t n; };
inline std::vector<SequenceSet> support_sequence_sets(const FragmentBatch &fb) {
  std::vector<SequenceSet> sets{{fb.bases.data(), fb.offs.data(), (uint64_t)fb.offs.size() - 1}};
  if (fb.paired) sets.push_back({fb.mate_bases.data(), fb.mate_offs.data(), (uint64_t)fb.mate_offs.size() - 1});
  return sets;
}

struct SupportRow { Taxon taxon; uint64_t kmers, minimizers, distinct; };
struct SupportCounts {
  std::vector<SupportRow> rows;   // ascending by taxon
  uint64_t sequences = 0, supermers = 0, matched = 0, kept = 0;
};

// One pass over the reads (ambiguous regions kept, as classify2 takes them) on dev's first table: the batches are parsed ahead by
// the input's own threads, and the next one is taken while the last is counted -- two batches in host memory, as `build` holds them.
inline SupportCounts support_pass(DeviceIndex &dev, const Taxonomy &tax, const std::vector<std::string> &files, bool paired, int rank_depth,
                                  bool want_distinct) {
  std::vector<int32_t> depths((size_t)tax.size());
  for (Taxon t = 0; t < tax.size(); t++) depths[t] = tax.depth(t);
  slk_support *sup = nullptr;
  SLK_CALL(slk_support_create(dev.ix, depths.data(), (int32_t)depths.size(), rank_depth, want_distinct ? 1 : 0, &sup));
  {
    InputRotation input(files, paired, nullptr);
    FragmentBatchPtr counting;   // the batch the device is reading
    std::future<std::pair<int32_t, std::string>> adding;
    auto wait_for_add = [&] {
      if (!adding.valid()) return;
      const auto r = adding.get();
      if (r.first != SLK_OK) die("slk_support_add: " + r.second);
    };
    while (FragmentBatchPtr fb = input.next()) {
      wait_for_add();   // (the batch before this one is free from here on)
      counting = std::move(fb);
      adding = std::async(std::launch::async, [sup, &dev, &counting] {
        for (const SequenceSet &s : support_sequence_sets(*counting)) {
          const int32_t rc = slk_support_add(sup, dev.st, s.bases, s.offsets, s.n);
          if (rc != SLK_OK) return std::make_pair(rc, std::string(slk_last_error()));
        }
        return std::make_pair((int32_t)SLK_OK, std::string());
      });
    }
    wait_for_add();
  }
  SupportCounts c;
  uint64_t n = 0;
  SLK_CALL(slk_support_result(sup, &n, nullptr, nullptr, nullptr, nullptr, 0));
  std::vector<int32_t> taxa(n);
  std::vector<uint64_t> kmers(n), minimizers(n), distinct(n);
  if (n) SLK_CALL(slk_support_result(sup, &n, taxa.data(), kmers.data(), minimizers.data(), distinct.data(), n));
  SLK_CALL(slk_support_totals(sup, &c.sequences, &c.supermers, &c.matched, &c.kept));
  slk_support_destroy(sup);
  c.rows.resize(n);
  for (uint64_t i = 0; i < n; i++) c.rows[i] = {taxa[i], kmers[i], minimizers[i], distinct[i]};
  return c;
}

// one column of the rows as the (taxon, value) pairs a KrakenReport is made of
inline std::vector<std::pair<Taxon, long>> support_column(const std::vector<SupportRow> &rows, uint64_t SupportRow::*column) {
  std::vector<std::pair<Taxon, long>> out;
  out.reserve(rows.size());
  for (const SupportRow &r : rows) out.emplace_back(r.taxon, (long)(r.*column));
  return out;
}

inline void write_support_report(const Taxonomy &tax, const std::vector<std::pair<Taxon, long>> &counts, std::ostream &out) {
  KrakenReport(tax, counts).print(out);
}

// the four files of Dynamic.reportDynamicIndexSupport (:212-228); classified: reads per taxon of Classifier.classify at confidence 0
inline void write_support_files(const Taxonomy &tax, const std::vector<SupportRow> &rows, const std::vector<std::pair<Taxon, long>> &classified,
                                const std::string &output) {
  const std::pair<const char *, std::vector<std::pair<Taxon, long>>> files[] = {
      {"totalKmerCount", support_column(rows, &SupportRow::kmers)},
      {"distinctMinimizerCount", support_column(rows, &SupportRow::distinct)},
      {"totalMinimizerCount", support_column(rows, &SupportRow::minimizers)},
      {"classifiedReadCount", classified}};
  for (auto &f : files) {
    std::ofstream out = open_output(output + "_support_report_" + f.first + ".txt");
    write_support_report(tax, f.second, out);
  }
}

}  // namespace slk_host
