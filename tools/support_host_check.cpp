// support_host_check.cpp -- drives the host-only parts of slacken_amd/host/support.hpp without a GPU, for a run under the host
// sanitizers: the option parsing, the views of a batch's reads that slk_support_add is given, and the four reports from rows.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o support_host_check tools/support_host_check.cpp
//       -Lslacken_amd/lib -lslacken_amd -lz -ldl -lpthread -Wl,-rpath,$PWD/slacken_amd/lib          (one command line)
//   ./support_host_check TAXONOMY_DIR ROWS_TSV CLASSIFIED_TSV OUTPUT
//
// ROWS_TSV: "taxon kmers minimizers distinct" lines, CLASSIFIED_TSV: "taxon reads" lines (tests/support_model.py gives both); the four
// OUTPUT_support_report_*.txt files are what `support` would write from them.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>

#include "../slacken_amd/host/support.hpp"

using namespace slk_host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "support_host_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static SupportOptions parse(std::vector<std::string> args) {
  std::vector<char *> argv;
  for (std::string &a : args) argv.push_back(a.data());
  return parse_support_options((int)argv.size(), argv.data());
}

int main(int argc, char **argv) {
  if (argc != 5) die("usage: support_host_check TAXONOMY_DIR ROWS_TSV CLASSIFIED_TSV OUTPUT");
  // options
  SupportOptions o = parse({"-i", "lib", "-o", "out", "a.fq"});
  CHECK(o.index == "lib" && o.output == "out" && o.rank_depth == 8 && o.min_hits == 2 && !o.paired && o.devices == std::vector<int>{0});
  CHECK(o.files == std::vector<std::string>{"a.fq"});
  o = parse({"--index", "lib", "--output", "out", "--rank", "genus", "--min-hits", "3", "-p", "--devices", "0,2,1", "a_1.fq", "a_2.fq", "b_1.fq", "b_2.fq"});
  CHECK(o.rank_depth == 7 && o.min_hits == 3 && o.paired && o.files.size() == 4 && (o.devices == std::vector<int>{0, 2, 1}));
  const std::string list = std::string(argv[4]) + "_files.txt";
  { std::ofstream f = open_output(list); f << "x.fq\n\n  y.fq.gz  \n"; }
  o = parse({"-i", "lib", "-o", "out", "--rank", "superkingdom", "@" + list, "z.fa"});
  CHECK(o.rank_depth == 1 && (o.files == std::vector<std::string>{"x.fq", "y.fq.gz", "z.fa"}));

  // a batch's reads as (bases, offsets, n): unpaired, paired, with empty reads, and an empty batch
  FragmentBatch fb;
  fb.add("r1", "ACGTNACGT", nullptr);
  fb.add("r2", "", nullptr);
  fb.add("r3", "TTTT", nullptr);
  std::vector<SequenceSet> sets = support_sequence_sets(fb);
  CHECK(sets.size() == 1 && sets[0].n == 3 && sets[0].offsets[0] == 0 && sets[0].offsets[1] == 9 && sets[0].offsets[2] == 9 && sets[0].offsets[3] == 13);
  CHECK(std::string((const char *)sets[0].bases, sets[0].offsets[3]) == "ACGTNACGTTTTT");
  FragmentBatch pb;
  pb.paired = true;
  const std::string_view m1 = "GGGGG", m2 = "";
  pb.add("p1", "ACGT", &m1);
  pb.add("p2", "CC", &m2);
  sets = support_sequence_sets(pb);
  CHECK(sets.size() == 2 && sets[0].n == 2 && sets[1].n == 2 && sets[1].offsets[1] == 5 && sets[1].offsets[2] == 5);
  CHECK(std::string((const char *)sets[1].bases, sets[1].offsets[2]) == "GGGGG" && sets[0].offsets[2] == 6);
  FragmentBatch none;
  sets = support_sequence_sets(none);
  CHECK(sets.size() == 1 && sets[0].n == 0 && sets[0].offsets[0] == 0);

  // the reports
  const Taxonomy tax = Taxonomy::load(argv[1]);
  std::vector<SupportRow> rows;
  long long t;
  unsigned long long k, m, d;
  std::ifstream f1 = open_input(argv[2]);
  while (f1 >> t >> k >> m >> d) rows.push_back({(Taxon)t, k, m, d});
  std::vector<std::pair<Taxon, long>> classified;
  std::ifstream f2 = open_input(argv[3]);
  while (f2 >> t >> k) classified.emplace_back((Taxon)t, (long)k);
  CHECK(support_column(rows, &SupportRow::kmers).size() == rows.size());
  if (!rows.empty()) CHECK(support_column(rows, &SupportRow::distinct)[0].second == (long)rows[0].distinct);
  write_support_files(tax, rows, classified, argv[4]);
  std::printf("support_host_check: %zu rows, %zu classified taxa\n", rows.size(), classified.size());
  return 0;
}
