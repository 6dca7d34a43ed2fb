// slacken_cli.cpp -- `slacken-amd`: the subcommands of the host above the C ABI (include/slacken_amd.h), mirroring the reference's CLI
// surface (S/ = src/main/scala/com/jnpersson/ of the reference; flags: S/slacken/Slacken.scala:66-100,186-196 -- classify: -i, -o,
// --min-hits, -p, --[no]unclassified, --[no]detailed, -c, --sample-regex, files, @list).  The library on disk is read by library_io.hpp,
// held on the devices by device_index.hpp and classified against by classify_stream.hpp; repeated_titles.hpp settles the titles that
// occur more than once; taxonomy.hpp, output.hpp, migration.hpp and stats.hpp make the outputs.  Each cites what it mirrors.
// Host-only subcommands (`report`, `parse`, `props`) exist so that this layer can be tested without a GPU.
#include <future>
#include <set>
#include <sstream>

#include "classify_stream.hpp"
#include "compare.hpp"
#include "coverage.hpp"
#include "mask.hpp"
#include "merge.hpp"
#include "migration.hpp"
#include "repeated_titles.hpp"
#include "support.hpp"

using namespace slk_host;
namespace fs = std::filesystem;

static std::vector<std::pair<Taxon, long>> read_counts_tsv(const char *path) {   // taxon \t count
  std::ifstream f(path);
  std::vector<std::pair<Taxon, long>> counts;
  Taxon t; long c;
  while (f >> t >> c) counts.emplace_back(t, c);
  return counts;
}
// CountFilter (Dynamic.scala:174-185): keys at depth >= rank whose clade total reaches the threshold
static std::vector<Taxon> count_filter(const Taxonomy &tax, const std::vector<std::pair<Taxon, long>> &counts, int rank_depth, long threshold) {
  KrakenReport agg(tax, counts);
  std::vector<Taxon> keep;
  for (auto &kv : agg.taxonCounts)
    if (tax.depth(kv.first) >= rank_depth && agg.clade(kv.first) >= threshold) keep.push_back(kv.first);
  return keep;
}
static int cmd_report(int argc, char **argv) {  // report <taxonomy dir> <counts.tsv>
  if (argc < 2) die("usage: report TAXONOMY_DIR COUNTS_TSV");
  Taxonomy tax = Taxonomy::load(argv[0]);
  KrakenReport(tax, read_counts_tsv(argv[1])).print(std::cout);
  return 0;
}
// taxonomy <taxonomy dir> <rank> <threshold> <counts.tsv>: the dynamic library's taxon selection on its own (Dynamic.scala
// CountFilter :174-185 + Taxonomy.taxaWithDescendants :304-311): line 1 = the kept taxa, line 2 = with descendants
static int cmd_taxonomy(int argc, char **argv) {
  if (argc < 4) die("usage: taxonomy TAXONOMY_DIR RANK THRESHOLD COUNTS_TSV");
  Taxonomy tax = Taxonomy::load(argv[0]);
  int rank = rank_index(argv[1]);
  if (rank == NO_RANK) die(std::string("unknown rank ") + argv[1]);
  const std::vector<Taxon> keep = count_filter(tax, read_counts_tsv(argv[3]), rank - 1, std::stol(argv[2]));
  for (Taxon k : keep) std::cout << k << ' ';
  std::cout << '\n';
  auto in = tax.withDescendants(keep);
  for (Taxon i = 0; i < tax.size(); i++) if (in[i]) std::cout << i << ' ';
  std::cout << '\n';
  return 0;
}
// gunzip FILE: the file's bytes as the input layer sees them (ByteSource: zlib, libbz2 or the parallel inflate of pargz.hpp)
static int cmd_gunzip(int argc, char **argv) {
  if (argc < 1) die("usage: gunzip FILE");
  ByteSource src(argv[0]);
  std::vector<char> buf((size_t)4 << 20);
  uint64_t total = 0;
  const double t0 = wall_seconds();
  const bool quiet = argc >= 2 && std::string(argv[1]) == "--count";
  while (size_t n = src.read(buf.data(), buf.size())) {
    if (!quiet && fwrite(buf.data(), 1, n, stdout) != n) die("write error");
    total += n;
  }
  if (quiet) {
    const double dt = wall_seconds() - t0;
    std::cout << total << " bytes, " << dt << " s, " << total / dt / 1e9 << " GB/s\n";
  }
  return 0;
}
// parse --device FILE: the same lines with the records found on the device (slk_parse_text) -- the file's bytes, inflated if need be, go
// up chunk by chunk out of pinned memory, the rest of a chunk that `consumed` leaves is carried over to the next
static int parse_on_device(int argc, char **argv) {
  if (argc != 1) die("usage: parse --device FILE");
  const std::vector<std::string> files{argv[0]};
  const slk_params sp{35, 31, 7, 1, SLK_DEFAULT_TOGGLE_MASK, 1, 0};   // (a stream belongs to an index: an empty one of the default shape)
  const slk_table_config cfg{1024, 0, 0.0f};
  slk_index *ix = nullptr;
  slk_stream *st = nullptr;
  SLK_CALL(slk_index_create(&sp, &cfg, 0, &ix));
  SLK_CALL(slk_stream_create(ix, &st));
  {
    TextChunks input(files);
    PinnedText buf;
    TextChunks::Chunk c;
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offs, tpos;
    std::vector<uint32_t> tlen;
    std::string out;
    while (input.next(buf, c)) {
      uint64_t R = 0, nb = 0, consumed = 0;
      size_t rcap = c.n / 64 + 1024;
      bases.resize(c.n);
      for (int attempt = 0;; attempt++) {
        offs.resize(rcap + 1); tpos.resize(rcap); tlen.resize(rcap);
        const int32_t rc = slk_parse_text(st, (const uint8_t *)c.p, c.n, c.fastq ? SLK_FORMAT_FASTQ : SLK_FORMAT_FASTA, c.final ? 1 : 0, bases.data(),
                                          offs.data(), tpos.data(), tlen.data(), bases.size(), rcap, &R, &nb, &consumed);
        if (rc == SLK_E_CAPACITY && attempt == 0 && R > rcap) { rcap = R; continue; }
        if (rc != SLK_OK) die(std::string("slk_parse_text: ") + slk_last_error());
        break;
      }
      if (!c.final && consumed != c.cut)
        die("internal: the device parser consumed " + std::to_string(consumed) + " bytes of a chunk that was cut at " + std::to_string(c.cut));
      out.clear();
      for (uint64_t r = 0; r < R; r++) {
        out.append(c.p + tpos[r], tlen[r]);
        out += '\t';
        out.append((const char *)bases.data() + offs[r], offs[r + 1] - offs[r]);
        out += '\n';
      }
      std::cout << out;
    }
  }
  slk_stream_destroy(st);
  slk_index_destroy(ix);
  return 0;
}
static int cmd_parse(int argc, char **argv) {  // parse <file> [<file2>]: header \t nucleotides [\t nucleotides2]
  if (argc < 1) die("usage: parse [--count] FILE [MATE_FILE] | parse --device FILE");
  if (std::string(argv[0]) == "--device") return parse_on_device(argc - 1, argv + 1);
  if (std::string(argv[0]) == "--count") {  // read through the batch reader only: fragments, bases, a checksum, seconds
    std::vector<std::string> files(argv + 1, argv + std::min(argc, 3));
    const double t0 = wall_seconds();
    BatchPrefetcher pf(files, files.size() >= 2);
    uint64_t n = 0, nb = 0, sum = 0;
    while (auto b = pf.next()) {
      n += b->size();
      nb += b->bases.size() + b->mate_bases.size();
      for (size_t i = 0; i < b->size(); i += 97) sum = sum * 31 + std::hash<std::string_view>()(b->title(i)) + b->seq(i).size();
    }
    const double dt = wall_seconds() - t0;
    std::cout << n << " fragments, " << nb << " bases, checksum " << sum << ", " << dt << " s\n";
    return 0;
  }
  std::vector<std::string> files(argv, argv + std::min(argc, 2));
  FragmentSource src(files, argc >= 2);
  for_each_fragment_batch(src, 4096, (size_t)64 << 20, [](const FragmentBatch &b) {
    for (size_t i = 0; i < b.size(); i++) {
      std::cout << b.title(i) << '\t' << b.seq(i);
      if (b.paired) std::cout << '\t' << b.mate(i);
      std::cout << '\n';
    }
  });
  return 0;
}
// records <idx>: how many records the library holds and a checksum of them, from the Parquet files (native reader) and
// from <idx>.slkrec when present -- lets the readers be tested without a GPU
static int cmd_records(int argc, char **argv) {
  if (argc < 1) die("usage: records INDEX_LOCATION");
  std::string location = argv[0];
  const int W = (read_index_params(location).m + 31) / 32;
  struct Digest {
    int W;
    uint64_t n = 0, kx = 0; int64_t ts = 0; int32_t mt = 0;
    void operator()(const int64_t *k, const int32_t *t, uint64_t c) {
      for (uint64_t i = 0; i < c; i++) { ts += t[i]; mt = std::max(mt, t[i]); }
      for (uint64_t i = 0; i < c * W; i++) kx ^= ((uint64_t)k[i] + i % W) * 0x9E3779B97F4A7C15ull;
      n += c;
    }
    void print(const char *src) const { std::cout << src << " n=" << n << " key_xor=" << kx << " taxon_sum=" << ts << " max_taxon=" << mt << '\n'; }
  };
  if (parquet_available() && fs::is_directory(location)) {
    Digest d{W};
    int64_t stat_max = -1;
    uint64_t rows = parquet_count_rows(location, W, &stat_max);
    parquet_for_each_batch(location, W, std::ref(d));
    if (rows != d.n) die("row count of the footers differs from the rows read");
    if (stat_max >= 0 && stat_max != d.mt) die("column statistics disagree with the data");
    d.print("parquet");
  }
  if (fs::exists(location + ".slkrec")) {
    Digest d{W};
    RecordFile(location, W).for_each_chunk(true, std::ref(d));
    d.print("slkrec");
  }
  return 0;
}

// the titles of a batch into the set of those seen; the ones seen before go to rep
static void track_titles(const FragmentBatch &fb, ConcurrentTitleSet &seen, RepeatedTitles &rep) {
  std::vector<uint64_t> hs(fb.size()), again;
  for (size_t i = 0; i < fb.size(); i++) hs[i] = title_hash(fb.title(i));
  seen.insert_many(hs, again);
  rep.add(again);
}

// repeated [-p] FILES: the read titles the classify command would regroup (titles.hpp) -- those that occur more than once among the
// fragments, and for paired input those whose header repeats inside one file of a pair -- one per line, sorted.  Host only: lets
// the detection be tested without a GPU (every fragment is taken to produce a row).
static int cmd_repeated(int argc, char **argv) {
  bool paired = false;
  std::vector<std::string> files;
  for (int i = 0; i < argc; i++) {
    if (std::string(argv[i]) == "-p") paired = true;
    else files.push_back(argv[i]);
  }
  if (files.empty() || (paired && files.size() % 2)) die("usage: repeated [-p] FILES...");
  RepeatedTitles rep;
  ConcurrentTitleSet titles;
  const size_t unit = paired ? 2 : 1;
  for (size_t u = 0; u + unit <= files.size(); u += unit) {
    FragmentSource src(std::vector<std::string>(files.begin() + u, files.begin() + u + unit), paired, &rep);
    for_each_fragment_batch(src, 4096, (size_t)64 << 20, [&](const FragmentBatch &b) { track_titles(b, titles, rep); });
  }
  rep.settle_unmatched([&](uint64_t h) { return titles.contains(h); });
  const FlatHashSet<0> D = rep.to_set();
  std::set<std::string> out;
  for (size_t i = 0; i < files.size(); i++)
    for_each_repeated_record(files[i], !paired ? "" : i % 2 == 0 ? "/1" : "/2", D, [&](std::string_view h, std::string_view) { out.insert(std::string(h)); });
  for (const std::string &t : out) std::cout << t << "\n";
  return 0;
}

static int cmd_props(int argc, char **argv) {
  if (argc < 1) die("usage: props INDEX_LOCATION");
  IndexParams ip = read_index_params(argv[0]);
  std::cout << "k=" << ip.k << " m=" << ip.m << " spaces=" << ip.spaces << " xorMask=" << (long long)ip.xorMask << " canonical=" << ip.canonical << '\n';
  return 0;
}

// ---- options shared by classify and classify2 (ClassifyCommand, Slacken.scala:66-100) ----
struct ClassifyOpts {
  std::string index, output, sample_regex;
  int min_hits = 2;
  bool paired = false, with_unclassified = true, detailed = true;
  std::vector<double> thresholds;
  std::vector<std::string> files;
  std::vector<int> devices{0};  // --devices: the GPUs that share the reads (table replicated on each)
  bool shard_table = false;     // --shard-table: the table is spread over the devices instead (a library beyond one GPU's memory)
  bool device_parse = false;    // --device-parse: the raw text goes to the device, which finds the records (classify_text_stream)
  bool device_pairs = false;    // --device-pairs: both mate files' text goes to the device, which finds and pairs the records (classify_paired_text_stream)
  long long split_long = -1;    // --split-long LEN: unpaired sequences of at least LEN bases are split over many waves (slk_stream_set_split_long)
  bool split_hits = false;      // --split-hits: ... and so are they when per-read lines (hit lists) are written (slk_stream_set_split_hits)
  // classify2 (Slacken.scala:199-260)
  std::string library, rank = "species";
  int min_count = -1, min_distinct = -1, reads = -1;
  double init_confidence = 0.15;
  // GoldSetOptions (Dynamic.scala:62): a user-supplied taxon set to compare the detected set with, or to build the library from
  std::string gold_set, promote_rank;
  bool classify_with_gold = false;
  int bracken_length = 0;       // --bracken-length (Slacken.scala:220,259): Bracken weights for the dynamic library as well
};

static void refuse_wide(const char *cmd, const IndexParams &ip) {
  if (ip.m > 32) die(std::string(cmd) + " supports minimizers of up to 32 nt (this library has m=" + std::to_string(ip.m) + ")");
}

static ClassifyOpts parse_classify_opts(int argc, char **argv, bool two_step) {
  ClassifyOpts o;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") o.index = a.next();
    else if (a == "-o" || a == "--output") o.output = a.next();
    else if (a == "--min-hits") o.min_hits = std::stoi(a.next());
    else if (a == "-p" || a == "--paired") o.paired = true;
    else if (a == "--unclassified") o.with_unclassified = true;
    else if (a == "--nounclassified") o.with_unclassified = false;
    else if (a == "--detailed") o.detailed = true;
    else if (a == "--nodetailed") o.detailed = false;
    else if (a == "-c" || a == "--confidence") { while (a.peek() && (isdigit(a.peek()[0]) || a.peek()[0] == '.')) o.thresholds.push_back(std::stod(a.next())); }
    else if (a == "--sample-regex") o.sample_regex = a.next();
    else if (a == "--devices") o.devices = parse_device_list(a.next());
    else if (a == "--shard-table") { if (two_step) die("--shard-table is for classify (the dynamic library of classify2 is small)"); o.shard_table = true; }
    else if (a == "--device-parse") {
      if (two_step) die("--device-parse is for classify (classify2 reads its input through the host parser)");
      o.device_parse = true;
    }
    else if (a == "--device-pairs") {
      if (two_step) die("--device-pairs is for classify (classify2 reads its input through the host parser)");
      o.device_pairs = true;
    }
    else if (a == "--split-long") {
      if (two_step) die("--split-long is for classify (classify2 classifies reads against a small dynamic library)");
      o.split_long = std::stoll(a.next());
      if (o.split_long < 0) die("--split-long takes a number of bases (0: never split)");
    }
    else if (a == "--split-hits") {
      if (two_step) die("--split-hits is for classify (classify2 classifies reads against a small dynamic library: nothing there to split)");
      o.split_hits = true;
    }
    else if (two_step && (a == "-l" || a == "--library")) o.library = a.next();
    else if (two_step && a == "--rank") o.rank = a.next();
    else if (two_step && (a == "-C" || a == "--min-count")) o.min_count = std::stoi(a.next());
    else if (two_step && (a == "-D" || a == "--min-distinct")) o.min_distinct = std::stoi(a.next());
    else if (two_step && (a == "-R" || a == "--reads")) o.reads = std::stoi(a.next());
    else if (two_step && a == "--init-confidence") o.init_confidence = std::stod(a.next());
    else if (two_step && (a == "-g" || a == "--gold-set")) o.gold_set = a.next();
    else if (two_step && a == "--classify-with-gold") o.classify_with_gold = true;
    else if (two_step && a == "--promote-gold-set") o.promote_rank = a.next();
    else if (two_step && a == "--bracken-length") {
      o.bracken_length = std::stoi(a.next());
      if (o.bracken_length < 1) die("--bracken-length must be a positive number of bases");
    }
    else if (two_step && a == "--index-reports")
      die(a.opt + " is not supported by this engine (index reports are outside the classify path: `coverage` and `support` write them)");
    else if (a.opt[0] == '@') { std::ifstream lf(a.opt.substr(1)); std::string l; while (std::getline(lf, l)) if (!trim(l).empty()) o.files.push_back(trim(l)); }
    else if (a.opt[0] == '-') die("unknown option " + a.opt);
    else o.files.push_back(a.opt);
  }
  if (o.index.empty() || o.output.empty() || o.files.empty() || (two_step && o.library.empty()))
    die(two_step ? "usage: classify2 -i INDEX -o OUTPUT --library DIR [--rank R] [-R N | -C N | -D N] [--init-confidence X] [classify options] FILES"
                 : "usage: classify -i INDEX -o OUTPUT [-p] [-c T...] [--min-hits N] [--sample-regex RE] FILES");
  if (two_step && o.gold_set.empty() && (o.classify_with_gold || !o.promote_rank.empty()))
    die("--classify-with-gold and --promote-gold-set qualify a gold set: give one with -g FILE");
  if (o.device_pairs && o.device_parse) die("--device-pairs and --device-parse exclude each other: --device-pairs is the device route for paired input (-p), --device-parse the one for unpaired input");
  if (o.device_pairs && !o.paired) die("--device-pairs pairs the records of two mate files: give -p and pairs of files (--device-parse is the device route for unpaired input)");
  if (o.device_pairs && o.shard_table) die("--device-pairs needs the whole table on the device that parses (not --shard-table)");
  if (o.split_long >= 0 && o.paired) die("--split-long splits unpaired sequences (contigs, assemblies): not with -p");
  if (o.split_long >= 0 && o.shard_table) die("--split-long needs the whole table on the device that classifies (not --shard-table)");
  if (o.split_hits && o.split_long <= 0) die("--split-hits extends --split-long LEN to runs that write per-read lines: give --split-long with LEN > 0");
  if (o.device_parse && o.paired) die("--device-parse takes unpaired input (the mates of paired reads are joined by title, on the host)");
  if (o.device_parse && o.shard_table) die("--device-parse needs the whole table on the device that parses (not --shard-table)");
  if (o.thresholds.empty()) o.thresholds.push_back(0.0);
  for (double t : o.thresholds) if (t < 0 || t > 1) die("confidence must be in [0, 1]");
  if (o.paired && o.files.size() % 2 != 0)
    die("For paired end mode, please supply pairs of files (even number). " + std::to_string(o.files.size()) + " files were supplied");
  if ((o.min_count >= 0) + (o.min_distinct >= 0) + (o.reads >= 0) > 1) die("--min-count, --min-distinct and --reads are mutually exclusive");
  if (o.init_confidence < 0 || o.init_confidence > 1) die("--read-confidence must be >=0 and <= 1");
  return o;
}

static void resolve_repeated_titles(DeviceIndex &dev, const IndexParams &ip, const ClassifyOpts &o, OutputSink &sink) {
  Timer t("Regroup repeated titles");
  const FlatHashSet<0> D = sink.repeated().to_set();
  const int C = (int)o.thresholds.size();
  const Regrouped g = regroup_repeated_titles(dev, o.files, o.paired, o.min_hits, o.thresholds, D, [&](const std::string &title, const RepeatResult &r) {
    if (r.hits.empty()) return;  // no span, no row
    const std::string sample = sink.sample_of(title);
    for (int c = 0; c < C; c++)
      if (r.classified[c] || o.with_unclassified) sink.adjust_count(c, sample, r.taxon[c], -1);
  });
  const size_t R = g.titles.size();
  if (R == 0) return;
  std::map<std::pair<int, std::string>, std::string> extra;
  for (size_t r = 0; r < R; r++) {
    const size_t n = g.moffs[r + 1] - g.moffs[r];
    if (n == 0) continue;   // none of the fragments had a span: no row
    const std::string sample = sink.sample_of(g.titles[r]);
    for (int c = 0; c < C; c++) {
      const bool classified = g.mcls[(size_t)c * R + r] != 0;
      if (!classified && !o.with_unclassified) continue;
      const int32_t tx = g.mtaxon[(size_t)c * R + r];
      sink.adjust_count(c, sample, tx, +1);
      if (o.detailed) OutputSink::append_output_line(extra[{c, sample}], classified, g.titles[r], tx, g.mhits.data() + g.moffs[r], n, ip.k, true);
    }
  }
  std::unordered_map<std::string_view, bool> drop;
  for (const std::string &title : g.titles) drop[title] = true;
  sink.replace_rows([&](std::string_view title) { return drop.count(title) != 0; }, extra);
}

// Classifier.classifyHitsAndWrite / writePerSampleOutput (Classifier.scala:156-227): per-read lines and Kraken reports
static void classify_and_write(DeviceIndex &dev, const IndexParams &ip, const Taxonomy &tax, const ClassifyOpts &o) {
  OutputOptions oo;
  oo.output = o.output; oo.sample_regex = o.sample_regex; oo.thresholds = o.thresholds;
  oo.with_unclassified = o.with_unclassified; oo.detailed = o.detailed; oo.k = ip.k;
  Timer t("Classify reads");
  OutputSink sink(oo, tax, host_threads());
  if (o.device_pairs)
    classify_paired_text_stream(dev, o.files, o.min_hits, o.thresholds, o.detailed, [&](std::shared_ptr<const ClassifiedBatch> b) { sink.submit(std::move(b)); },
                                &sink.repeated(), true);
  else if (o.device_parse)
    classify_text_stream(dev, o.files, o.min_hits, o.thresholds, o.detailed, [&](std::shared_ptr<const ClassifiedBatch> b) { sink.submit(std::move(b)); }, true);
  else
    classify_stream(dev, o.files, o.paired, o.min_hits, o.thresholds, false, o.detailed,   // (hit lists only feed the per-read lines)
                    [&](std::shared_ptr<const ClassifiedBatch> b) { sink.submit(std::move(b)); }, &sink.repeated(), nullptr, true);
  sink.drain();
  sink.repeated().settle_unmatched([&](uint64_t h) { return sink.has_title(h); });
  if (!sink.repeated().empty()) resolve_repeated_titles(dev, ip, o, sink);
  sink.finish();
}

static int cmd_classify(int argc, char **argv) {
  ClassifyOpts o = parse_classify_opts(argc, argv, false);
  if (o.device_parse && read_index_params(o.index).m > 32)
    die("--device-parse supports minimizers of up to 32 nt (this library has m=" + std::to_string(read_index_params(o.index).m) + ")");
  if (o.device_pairs && read_index_params(o.index).m > 32)
    die("--device-pairs supports minimizers of up to 32 nt (this library has m=" + std::to_string(read_index_params(o.index).m) + ")");
  if (o.split_long >= 0 && read_index_params(o.index).m > 32)
    die("--split-long supports minimizers of up to 32 nt (this library has m=" + std::to_string(read_index_params(o.index).m) + ")");
  if (o.split_long > 0 && o.detailed && !o.split_hits)
    std::cerr << "note: --split-long has no effect on this run: per-read lines need hit lists, which keep the other routes (give --nodetailed)" << std::endl;
  LoadedIndex lib(o.index, o.devices, o.shard_table);
  lib.dev.split_long = o.split_long;
  lib.dev.split_hits = o.split_hits;
  classify_and_write(lib.dev, lib.ip, lib.tax, o);
  return 0;
}

// ---- classify2: two-step classification with a dynamic library (Dynamic.scala; Slacken.scala:199-260) ----
// the .fna files under DIR/library (HDFSUtil.findFiles(location + "/library", ".fna")), sorted
static std::vector<std::string> library_fna_files(const std::string &library) {
  const fs::path dir = fs::path(library) / "library";
  if (!fs::exists(dir)) die("no such directory: " + dir.string());
  std::vector<std::string> fna;
  for (auto &e : fs::recursive_directory_iterator(dir))
    if (e.is_regular_file() && ends_with(e.path().string(), ".fna")) fna.push_back(e.path().string());
  std::sort(fna.begin(), fna.end());
  return fna;
}
// every sequence of those files, in the order of the sorted files: fn(sequence id, sequence)
template <class Fn>
static void for_each_library_sequence(const std::string &library, Fn fn) {
  for (auto &file : library_fna_files(library)) {
    AsyncRecordStream rs(file);  // (plain .fna files are parsed on several threads)
    std::string_view h, sq;
    while (rs.next(h, sq)) fn(h, sq);
  }
}
// the sequences whose header carries a label: fn(sequence, taxon)
template <class Fn>
static void for_each_labelled_sequence(const std::string &library, const std::unordered_map<std::string, Taxon> &labels, Fn fn) {
  for_each_library_sequence(library, [&](std::string_view h, std::string_view sq) {
    auto it = labels.find(std::string(h));
    if (it != labels.end()) fn(sq, it->second);
  });
}

// "%.2f%%".format(d * 100) (Helpers.formatPerc, S/kmers/package.scala:60) with java.util.Formatter's rounding
static std::string format_perc(double d) {
  if (std::isnan(d)) return "NaN%";
  std::string v = java_format_6_2f(d * 100);
  return v.substr(v.find_first_not_of(' ')) + "%";
}
static std::string rank_name(int rank_index_) {   // a Rank's toString: the case object's name (Taxonomy.scala:39-48)
  if (rank_index_ == NO_RANK) return "null";
  std::string t = rank_titles(rank_index_);
  if (!t.empty()) t[0] = (char)toupper((unsigned char)t[0]);
  return t;
}

// Dynamic.readGoldSet (Dynamic.scala:284-310): the taxa of the file (one per line, first CSV column; secondary ids mapped to their
// primaries by merged.dmp), those without sequence in the library replaced by -- in the reference's words "promoted to" -- their
// nearest ancestor that has, everything filtered at the reclassification rank; the promoted ones are kept down to
// --promote-gold-set RANK if that is given.  in_library: GenomeLibrary.taxonSet (:35-44), the labelled taxa with their ancestors.
// The messages are the reference's (println: standard output).
static std::vector<Taxon> read_gold_set(const Taxonomy &tax, const std::string &file, const std::string &promote_rank, int rank_depth,
                                        const std::string &rank_title, const std::vector<uint8_t> &in_library) {
  std::ifstream f(file);
  if (!f) die("cannot open the gold set " + file);
  std::set<Taxon> gold;
  std::string l;
  while (std::getline(f, l)) {
    if (!l.empty() && l.back() == '\r') l.pop_back();
    if (l.empty()) continue;   // (spark.read.csv drops empty lines)
    std::string c0 = l.substr(0, l.find(','));
    if (c0.size() >= 2 && c0.front() == '"' && c0.back() == '"') c0 = c0.substr(1, c0.size() - 2);
    size_t used = 0;
    int t = 0;
    try { t = std::stoi(c0, &used); } catch (...) { used = 0; }
    if (used != c0.size() || c0.empty()) die("gold set " + file + ": not a taxon id: " + l);   // (x.getString(0).toInt throws)
    if (t < 0 || t >= (int)tax.primary.size()) die("gold set " + file + ": taxon " + c0 + " is outside the taxonomy");
    gold.insert(tax.primary[t]);
  }
  std::cout << "Gold set contained " << gold.size() << " taxa" << std::endl;
  auto in_lib = [&](Taxon t) { return t >= 0 && t < (Taxon)in_library.size() && in_library[t]; };
  std::set<Taxon> not_found, promoted;
  for (Taxon t : gold) if (!in_lib(t)) not_found.insert(t);
  for (Taxon t : not_found)
    for (Taxon p = t; p != NONE; p = (p >= 0 && p < tax.size()) ? tax.parents[p] : NONE)   // Taxonomy.pathToRoot :204-215
      if (in_lib(p)) { promoted.insert(p); break; }
  std::cout << not_found.size() << " taxa from gold set not found in library, promoted to " << promoted.size() << " taxa." << std::endl;
  {
    std::map<int, int> by_depth;   // (depth -> taxa; Rank orders by depth)
    for (Taxon t : promoted) by_depth[tax.depth(t)]++;
    std::cout << "Promoted to levels: ArrayBuffer(";
    bool first = true;
    for (auto &kv : by_depth) {
      std::cout << (first ? "" : ", ") << "(" << rank_name(kv.first >= 0 && kv.first <= 8 ? kv.first + 1 : NO_RANK) << "," << kv.second << ")";
      first = false;
    }
    std::cout << ")" << std::endl;
  }
  std::set<Taxon> kept;
  if (!promote_rank.empty()) {
    const int pr = rank_index(promote_rank);
    if (pr == NO_RANK) die("unknown rank " + promote_rank);
    for (Taxon t : promoted) if (tax.depth(t) >= pr - 1) kept.insert(t);
    std::cout << "Keeping " << kept.size() << " taxa at rank " << rank_name(pr) << " and below from promoted set" << std::endl;
  }
  std::set<Taxon> total = gold;
  total.insert(promoted.begin(), promoted.end());
  std::set<Taxon> filtered = kept;
  for (Taxon t : total) if (tax.depth(t) >= rank_depth) filtered.insert(t);
  std::cout << "Initial adjusted gold set size " << total.size() << ", filtered at " << rank_title << " to " << filtered.size() << std::endl;
  return std::vector<Taxon>(filtered.begin(), filtered.end());
}

// step 1 of classify2: per-taxon support in the sample (Dynamic.findTaxonSet :213-243), by one of three strategies
using TaxonSupport = std::map<Taxon, long>;
// -C: MinimizerTotalCount, -D: MinimizerDistinctCount -- the hits with a true taxon at depth >= rank (minimizersInSubjects :95-107)
// grouped by taxon and counted, with repetitions or distinct (:111-117), on the device (support.hpp; one device: the first)
static TaxonSupport support_by_minimizers(DeviceIndex &base, const ClassifyOpts &o, const Taxonomy &tax, int rank_depth, bool distinct) {
  note_one_support_device(o.devices);
  const SupportCounts c = support_pass(base, tax, o.files, o.paired, rank_depth, distinct);
  std::cerr << c.sequences << " sequences" << std::endl;
  TaxonSupport m;
  for (const SupportRow &r : c.rows) m[r.taxon] = (long)(distinct ? r.distinct : r.minimizers);
  return m;
}
// -R: ClassifiedReadCount(threshold, confidence): classified reads per taxon (classifiedReadsPerTaxon :133-141).  That count goes
// through Classifier.classify, which regroups the hits by title (Classifier.scala:92): fragments that share a title are one
// read here too -- the titles are tracked on the way, and those that repeat are settled as in the final classification.
static TaxonSupport support_by_classified_reads(DeviceIndex &base, const ClassifyOpts &o) {
  TaxonSupport m;
  ConcurrentTitleSet seen;
  RepeatedTitles rep;
  classify_stream(base, o.files, o.paired, o.min_hits, {o.init_confidence}, false, false, [&](std::shared_ptr<const ClassifiedBatch> b) {
    for (size_t i = 0; i < b->frags->size(); i++)
      if (b->hit_offs[i + 1] > b->hit_offs[i] && b->classified[i]) m[b->taxon[i]] += 1;
  }, &rep, [&](const FragmentBatch &fb) { track_titles(fb, seen, rep); });
  rep.settle_unmatched([&](uint64_t h) { return seen.contains(h); });
  if (rep.empty()) return m;
  const std::vector<double> thr{o.init_confidence};
  const Regrouped g = regroup_repeated_titles(base, o.files, o.paired, o.min_hits, thr, rep.to_set(), [&](const std::string &, const RepeatResult &r) {
    if (!r.hits.empty() && r.classified[0]) m[r.taxon[0]] -= 1;
  });
  for (size_t r = 0; r < g.titles.size(); r++)
    if (g.moffs[r + 1] > g.moffs[r] && g.mcls[r]) m[g.mtaxon[r]] += 1;
  for (auto it = m.begin(); it != m.end();) it = it->second == 0 ? m.erase(it) : std::next(it);
  return m;
}

// What classify2 carries from step to step
struct TwoStep {
  ClassifyOpts o;
  int rank = NO_RANK, rank_depth = 0;
  IndexParams ip;
  Taxonomy tax;
  int32_t max_taxon = 0;
  std::vector<std::pair<std::string, Taxon>> all_labels;   // GenomeLibrary.getTaxonLabels
  std::vector<Taxon> gold;   // readGoldSet's result, if a gold set was given
  bool with_gold = false;    // makeRecords :366-369: the library is built from the gold set, nothing is detected
  std::vector<uint8_t> bases;   // the sequences of the dynamic library
  std::vector<uint64_t> offsets{0};
  std::vector<int32_t> taxa;
};

// The base index in device memory for as long as this runs: the gold set (which needs the taxonomy) and the detection pass
// (inputs: getInputFragments(withAmbiguous = true), Dynamic.scala:323)
static std::vector<std::pair<Taxon, long>> detect_taxon_support(TwoStep &s) {
  const ClassifyOpts &o = s.o;
  DeviceIndex base;
  base.devices = o.devices;
  load_index(o.index, s.ip, s.tax, base);
  if (o.bracken_length > 0 && o.bracken_length < s.ip.k)
    die("--bracken-length " + std::to_string(o.bracken_length) + " is shorter than k = " + std::to_string(s.ip.k));
  slk_index_info info;
  SLK_CALL(slk_index_get_info(base.ix, &info));
  s.max_taxon = info.taxonomy_size - 1;
  if (!o.gold_set.empty()) {
    // GenomeLibrary.taxonSet (:35-44): the labelled taxa and their ancestors (Taxonomy.taxaWithAncestors :306-310)
    std::vector<uint8_t> in_library((size_t)s.tax.size(), 0);
    for (auto &lb : s.all_labels)
      for (Taxon p = lb.second; p > 0 && p < s.tax.size() && !in_library[p]; p = s.tax.parents[p]) in_library[p] = 1;
    s.gold = read_gold_set(s.tax, o.gold_set, o.promote_rank, s.rank_depth, rank_name(s.rank), in_library);
  }
  TaxonSupport m;
  if (s.with_gold) {}   // (no detection pass)
  else if (o.min_count >= 0) m = support_by_minimizers(base, o, s.tax, s.rank_depth, false);
  else if (o.min_distinct >= 0) m = support_by_minimizers(base, o, s.tax, s.rank_depth, true);
  else m = support_by_classified_reads(base, o);
  return std::vector<std::pair<Taxon, long>>(m.begin(), m.end());
}

// The taxon set of the dynamic library, with descendants: the count filter, OUTPUT_taxonSet.txt, the comparison with the gold set
static std::vector<uint8_t> select_taxon_set(const TwoStep &s, const std::vector<std::pair<Taxon, long>> &counts) {
  const ClassifyOpts &o = s.o;
  const long threshold = o.min_count >= 0 ? o.min_count : o.min_distinct >= 0 ? o.min_distinct : o.reads >= 0 ? o.reads : 100;
  std::vector<Taxon> keep = count_filter(s.tax, counts, s.rank_depth, threshold);
  if (s.with_gold) {
    keep = s.gold;   // Dynamic.makeRecords :366-369: taxonomy.taxaWithDescendants(goldSet); no _taxonSet.txt, nothing was detected
  } else {
    std::ofstream ts(o.output + "_taxonSet.txt");  // HDFSUtil.writeTextLines, Dynamic.scala:224-225 (BitSet order = ascending)
    for (Taxon t : keep) ts << t << "\n";
  }
  if (!o.gold_set.empty() && !s.with_gold) {
    // findTaxonSet :262-274: the detected set against the gold set
    std::set<Taxon> g(s.gold.begin(), s.gold.end());
    size_t tp = 0;
    for (Taxon t : keep) tp += g.count(t);
    const size_t fp = keep.size() - tp, fn = g.size() - tp;
    std::cout << "Comparing detected set with supplied gold set. True Positives: " << tp << ", False Positives: " << fp << ", False Negatives: " << fn
              << ", Precision: " << format_perc((double)tp / (double)(tp + fp)) << ", Recall: " << format_perc((double)tp / (double)g.size()) << std::endl;
  }
  std::vector<uint8_t> in_set = s.tax.withDescendants(keep);
  size_t n_set = 0;
  for (uint8_t b : in_set) n_set += b;
  if (s.with_gold) std::cerr << "Gold set: " << keep.size() << " taxa at rank " << o.rank << ", expanded with descendants to " << n_set << std::endl;
  else std::cerr << "Detected set: initial scan produced " << keep.size() << " taxa at rank " << o.rank << ", expanded with descendants to " << n_set << std::endl;
  return in_set;
}

// step 2: KeyValueIndex.makeRecords(library, Some(taxonSet)) :100-122 -- the sequences whose label is in the set, into a table
static void build_dynamic_index(TwoStep &s, const std::vector<uint8_t> &in_set, DeviceIndex &dyn) {
  std::unordered_map<std::string, Taxon> labels;
  for (auto &lb : s.all_labels) {
    const Taxon t = lb.second;
    if (t >= 0 && t < s.tax.size() && in_set[t] && s.tax.isDefined(t)) labels[lb.first] = t;
  }
  for_each_labelled_sequence(s.o.library, labels, [&](std::string_view sq, Taxon t) {
    s.bases.insert(s.bases.end(), sq.begin(), sq.end());
    s.offsets.push_back(s.bases.size());
    s.taxa.push_back(t);
  });
  std::cerr << "Construct dynamic records from: " << s.taxa.size() << " sequences, " << s.bases.size() << " bases" << std::endl;
  // distinct minimizers <= super-mers: about 2/(w+1) per k-mer window on random sequence, at most one per window
  const int w = s.ip.k - s.ip.m + 1;
  uint64_t expected = (uint64_t)((double)s.bases.size() * std::min(1.0, 2.5 / (w + 1))) + 1024;
  dyn.devices = s.o.devices;
  for (int attempt = 0;; attempt++) {
    dyn.create(s.ip, s.tax, expected, s.max_taxon);
    int32_t rc = dyn.add_sequences(s.bases.data(), s.offsets.data(), s.taxa.data(), s.taxa.size());
    if (rc == SLK_OK) break;
    if (rc != SLK_E_CAPACITY || attempt == 1) die("slk_index_add_sequences: " + dyn.last_error);
    dyn.reset();  // low-complexity sequence: retry with one record per base
    expected = s.bases.size() + 1024;
  }
  dyn.finalize();
  slk_index_info info;
  SLK_CALL(slk_index_get_info(dyn.ix, &info));
  std::cerr << "dynamic index: " << info.records << " records" << std::endl;
}

// Dynamic.scala:339-344: the dynamic library's genomes against the dynamic index
static void bracken_of_dynamic_library(const TwoStep &s, DeviceIndex &dyn) {
  Timer t("Bracken weights");
  BrackenRun br(dyn, s.o.bracken_length);
  for (size_t r = 0; r < s.taxa.size(); r++)
    br.add_record(std::string_view((const char *)s.bases.data() + s.offsets[r], s.offsets[r + 1] - s.offsets[r]), s.taxa[r]);
  br.flush();
  br.finish(s.o.output + "/database" + std::to_string(s.o.bracken_length) + "mers.kmer_distrib");
}

static int cmd_classify2(int argc, char **argv) {
  TwoStep s;
  s.o = parse_classify_opts(argc, argv, true);
  s.rank = rank_index(s.o.rank);  // Taxonomy.rankOrNull
  if (s.rank == NO_RANK) die("unknown rank " + s.o.rank);
  s.rank_depth = s.rank - 1;
  s.all_labels = read_label_map(s.o.library);
  s.with_gold = !s.o.gold_set.empty() && s.o.classify_with_gold;
  const auto counts = detect_taxon_support(s);   // (the base index has left HBM when this returns)
  const std::vector<uint8_t> in_set = select_taxon_set(s, counts);
  DeviceIndex dyn;
  build_dynamic_index(s, in_set, dyn);
  classify_and_write(dyn, s.ip, s.tax, s.o);
  if (s.o.bracken_length > 0) bracken_of_dynamic_library(s, dyn);
  return 0;
}

// bracken-build (Slacken.scala:264-279): BrackenWeights.buildAndWriteWeights over the whole library, taxa = GenomeLibrary.taxonSet
// (GenomeLibrary.scala:35-44: the labelled taxa with their ancestors; a label outside the taxonomy is dropped)
static int cmd_bracken_build(int argc, char **argv) {
  std::string index, library;
  int read_len = 100;
  std::vector<int> devices{0};
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") index = a.next();
    else if (a == "-l" || a == "--library") library = a.next();
    else if (a == "--read-len") read_len = std::stoi(a.next());
    else if (a == "--devices") devices = parse_device_list(a.next());
    else if (a == "--shard-table") die("--shard-table is not supported by bracken-build: the library is replicated on each device");
    else die("unknown option " + a.opt);
  }
  if (index.empty() || library.empty()) die("usage: bracken-build -i INDEX --library DIR [--read-len L (100)] [--devices LIST]");
  if (read_len < 1) die("--read-len must be a positive number of bases");
  LoadedIndex lib(index, devices);
  if (read_len < lib.ip.k) die("--read-len " + std::to_string(read_len) + " is shorter than k = " + std::to_string(lib.ip.k));
  std::unordered_map<std::string, Taxon> labels;
  for (auto &lb : read_label_map(library))
    if (lb.second > 0 && lb.second < lib.tax.size()) labels[lb.first] = lb.second;
  // the records stream through: one batch per replica in host memory at a time
  Timer t("Bracken weights");
  BrackenRun br(lib.dev, read_len);
  for_each_labelled_sequence(library, labels, [&](std::string_view sq, Taxon t) { br.add_record(sq, t); });
  br.flush();
  std::cerr << "Bracken weights of " << br.sequences() << " sequences, " << br.bases() << " bases, read length " << read_len << std::endl;
  br.finish(index + "_bracken/database" + std::to_string(read_len) + "mers.kmer_distrib");
  return 0;
}

template <class Fn> static void for_each_triple(const char *path, Fn fn) {   // "a \t b \t count" lines: fn(a, b, count)
  std::ifstream f = open_input(path);
  long long a, b;
  unsigned long long n;
  while (f >> a >> b >> n) fn(a, b, (uint64_t)n);
}
// kmer-distrib TRIPLES_TSV: the kmer_distrib text of "dest \t source \t count" lines (host only: the file format without a GPU)
static int cmd_kmer_distrib(int argc, char **argv) {
  if (argc < 1) die("usage: kmer-distrib TRIPLES_TSV");
  std::vector<int32_t> d, s;
  std::vector<uint64_t> c;
  for_each_triple(argv[0], [&](long long a, long long b, uint64_t n) { d.push_back((int32_t)a); s.push_back((int32_t)b); c.push_back(n); });
  std::cout << kmer_distrib_text(d, s, c);
  return 0;
}

// ---- compare-index (Slacken.scala:332-341): MinimizerMigration(subject, reference).run(output) ----
// The table on stdout, OUTPUT_taxaToRoot_report.txt beside it (MinimizerMigration.scala:68-84)
static void write_migration_files(const Taxonomy &subject_tax, const std::vector<int32_t> &t1, const std::vector<int32_t> &t2,
                                  const std::vector<int32_t> &steps, const std::vector<uint64_t> &count, const std::string &output) {
  std::ofstream rep = open_output(output + "_taxaToRoot_report.txt");
  write_migration(subject_tax, t1, t2, steps, count, std::cout, rep);
  std::cout.flush();
}

// migration-report SUBJECT_TAXONOMY_DIR REFERENCE_TAXONOMY_DIR PAIRS_TSV OUTPUT: what compare-index writes, from "t1 \t t2 \t count"
// lines (host only: the outputs without a GPU)
static int cmd_migration_report(int argc, char **argv) {
  if (argc < 4) die("usage: migration-report SUBJECT_TAXONOMY_DIR REFERENCE_TAXONOMY_DIR PAIRS_TSV OUTPUT");
  const Taxonomy subject_tax = Taxonomy::load(argv[0]), reference_tax = Taxonomy::load(argv[1]);
  std::vector<int32_t> t1, t2, steps;
  std::vector<uint64_t> count;
  for_each_triple(argv[2], [&](long long a, long long b, uint64_t n) {
    t1.push_back((int32_t)a); t2.push_back((int32_t)b); count.push_back(n);
    steps.push_back(migration_steps(reference_tax, (Taxon)a, (Taxon)b));
  });
  write_migration_files(subject_tax, t1, t2, steps, count, argv[3]);
  return 0;
}

static int cmd_compare_index(int argc, char **argv) {
  const char *usage = "usage: compare-index -i SUBJECT -r REFERENCE -o OUTPUT [--devices D]", *why_one = "the reference's table must fit one GPU";
  std::string subject, reference, output;
  std::vector<int> devices{0};
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") subject = a.next();
    else if (a == "-r" || a == "--reference") reference = a.next();
    else if (a == "-o" || a == "--output") output = a.next();
    else if (a == "--devices") devices = parse_single_device(a.next(), "compare-index", why_one);
    else if (a == "--shard-table") refuse_shard_table("compare-index", why_one, usage);
    else die("unknown option " + a.opt);
  }
  if (subject.empty() || reference.empty() || output.empty()) die(usage);
  // "They must use the same minimizer scheme for the comparison to be meaningful" (MinimizerMigration.scala:31): checked here
  const IndexParams sp = read_index_params(subject), rp0 = read_index_params(reference);
  if (sp.k != rp0.k || sp.m != rp0.m || sp.spaces != rp0.spaces || sp.xorMask != rp0.xorMask || sp.canonical != rp0.canonical)
    die("the two libraries do not share a minimizer scheme (k, m, minimizerSpaces, XORmask, canonical of " + subject + ".properties and " +
        reference + ".properties differ): their minimizers cannot be compared");
  const Taxonomy subject_tax = Taxonomy::load(subject + "_taxonomy");
  LoadedIndex ref(reference, devices);
  const Taxonomy &reference_tax = ref.tax;
  const double t0 = wall_seconds();
  std::vector<int32_t> depths(reference_tax.size());
  for (Taxon t = 0; t < reference_tax.size(); t++) depths[t] = reference_tax.depth(t);
  slk_migration *mg = nullptr;
  SLK_CALL(slk_migration_create(ref.dev.ix, depths.data(), (int32_t)depths.size(), &mg));
  // the subject's records stream through: one chunk in host memory, no second table
  const int W = (sp.m + 31) / 32;
  uint64_t n_read = 0;
  for_each_record_batch(subject, W, [&](const int64_t *keys, const int32_t *taxa, uint64_t c) {
    n_read += c;
    SLK_CALL(slk_migration_add(mg, ref.dev.st, keys, taxa, c));
  });
  uint64_t n = 0, matched = 0, unmatched = 0;
  SLK_CALL(slk_migration_result(mg, &n, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
  std::vector<int32_t> t1(n), t2(n), steps(n);
  std::vector<uint64_t> count(n);
  if (n) SLK_CALL(slk_migration_result(mg, &n, t1.data(), t2.data(), steps.data(), count.data(), n, &matched, &unmatched));
  else SLK_CALL(slk_migration_result(mg, &n, nullptr, nullptr, nullptr, nullptr, 0, &matched, &unmatched));
  slk_migration_destroy(mg);
  write_migration_files(subject_tax, t1, t2, steps, count, output);
  std::cerr << "compare-index: " << n_read << " records read, " << matched << " matched, " << unmatched << " unmatched, " << n
            << " distinct pairs, " << wall_seconds() - t0 << " s" << std::endl;
  return 0;
}

// ---- stats (Slacken.scala:281-315) and inspect (:317-330) without --library: functions of the records per taxon ----
static const char *STATS_USAGE = "usage: stats -i INDEX [--histogram] [--devices D]";
static const char *INSPECT_USAGE = "usage: inspect -i INDEX -o OUTPUT [--labels FILE] [--devices D]";

// OUTPUT_min_report.txt, OUTPUT_genome_report.txt and, with a label file, OUTPUT_missing_report.txt (KeyValueIndex.scala:274-306)
static void write_inspect_files(const Taxonomy &tax, const TaxonCounts &counts, const std::string &output, const std::string &labels) {
  std::set<Taxon> label_taxa;
  if (!labels.empty()) {
    std::ifstream lf = open_input(labels);
    label_taxa = read_label_taxa(lf);
  }
  std::ofstream f1 = open_output(output + "_min_report.txt");
  write_min_report(tax, counts, f1);
  std::ofstream f2 = open_output(output + "_genome_report.txt");
  write_genome_report(tax, counts, f2);
  if (labels.empty()) return;
  std::ofstream f3 = open_output(output + "_missing_report.txt");
  write_missing_report(tax, counts, label_taxa, f3);
}

// stats-report TAXONOMY_DIR COUNTS_TSV M [--histogram] [-o OUTPUT [--labels FILE]]: what `stats` prints after the splitter lines,
// or with -o what `inspect` writes, from "taxon \t count" lines (host only: the outputs without a GPU)
static int cmd_stats_report(int argc, char **argv) {
  const char *usage = "usage: stats-report TAXONOMY_DIR COUNTS_TSV M [--histogram] [-o OUTPUT [--labels FILE]]";
  std::vector<std::string> pos;
  std::string output, labels;
  bool histogram = false;
  for (Args a(argc, argv); a.take();) {
    if (a == "--histogram") histogram = true;
    else if (a == "-o" || a == "--output") output = a.next();
    else if (a == "--labels") labels = a.next();
    else if (a.opt.size() > 1 && a.opt[0] == '-') die("unknown option " + a.opt + "\n" + usage);
    else pos.push_back(a.opt);
  }
  if (pos.size() != 3 || (!labels.empty() && output.empty())) die(usage);
  const Taxonomy tax = Taxonomy::load(pos[0]);
  std::ifstream f = open_input(pos[1]);
  std::map<Taxon, uint64_t> sum;   // (any order, a taxon may repeat)
  long long t;
  unsigned long long c;
  while (f >> t >> c) sum[(Taxon)t] += c;
  const TaxonCounts counts(sum.begin(), sum.end());
  if (output.empty()) std::cout << stats_text(tax, counts, std::stoi(pos[2]), histogram);
  else write_inspect_files(tax, counts, output, labels);
  return 0;
}

// the options stats and inspect share; what neither supports is refused on the command line and the properties alone, before any
// library is read
struct StatsOptions {
  std::string index, output, labels;
  bool histogram = false;
  std::vector<int> devices{0};
};
static StatsOptions parse_stats_options(const char *cmd, const char *usage, bool inspect, int argc, char **argv) {
  StatsOptions o;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") o.index = a.next();
    else if (inspect && (a == "-o" || a == "--output")) o.output = a.next();
    else if (inspect && a == "--labels") o.labels = a.next();
    else if (!inspect && a == "--histogram") o.histogram = true;
    else if (a == "-l" || a == "--library")
      die(std::string("--library is not supported by ") + cmd + ": genome coverage (IndexStatistics) is not part of this engine\n" + usage);
    else if (a == "--devices") o.devices = parse_single_device(a.next(), cmd, "the library's table must fit one GPU");
    else if (a == "--shard-table") refuse_shard_table(cmd, "the library's table must fit one GPU", usage);
    else die("unknown option " + a.opt + "\n" + usage);
  }
  if (o.index.empty() || (inspect && o.output.empty())) die(usage);
  refuse_wide(cmd, read_index_params(o.index));
  return o;
}

static std::string java_binary_string(uint64_t x) {   // java.lang.Long.toBinaryString: no leading zeros
  std::string s;
  for (; x; x >>= 1) s.insert(s.begin(), (char)('0' + (x & 1)));
  return s.empty() ? "0" : s;
}

// The splitter lines of Slacken.scala:291-302.  The masks are one word (m <= 32, which the count needs anyway): SpacedSeed.spaceMask
// (MinimizerPriorities.scala:287-300) and RandomXOR.mask (:146-160), both left aligned.  The reference's third line is the toString
// of a Scala object; this one names the parameters in the engine's words.
static void print_splitter_lines(const IndexParams &ip) {
  if (ip.spaces > 0) {
    const int r = ip.m % 32;
    uint64_t sm = r == 0 ? ~0ULL : ~0ULL << ((32 - r) * 2);
    const uint64_t final_bits = 3ULL << ((64 - r * 2) & 63);
    for (int i = 0; i < ip.spaces; i++) sm = (sm << 4) | final_bits;
    std::cout << "Spaced mask (left aligned) " << java_binary_string(sm) << "\n";
    std::cout << "Toggle mask (left aligned) " << java_binary_string(r == 0 ? ip.xorMask : ip.xorMask << (64 - r * 2)) << "\n";
    std::cout << "Inner splitter randomXOR m=" << ip.m << " XORmask=" << (int64_t)ip.xorMask << " canonical=" << (ip.canonical ? "true" : "false") << "\n";
  } else {
    std::cout << "Splitter randomXOR k=" << ip.k << " m=" << ip.m << " XORmask=" << (int64_t)ip.xorMask << " canonical="
              << (ip.canonical ? "true" : "false") << "\n";
  }
}

static int stats_or_inspect(bool inspect, int argc, char **argv) {
  const StatsOptions o = parse_stats_options(inspect ? "inspect" : "stats", inspect ? INSPECT_USAGE : STATS_USAGE, inspect, argc, argv);
  LoadedIndex lib(o.index, o.devices);
  if (inspect) { write_inspect_files(lib.tax, device_taxon_counts(lib.dev.ix), o.output, o.labels); return 0; }
  print_splitter_lines(lib.ip);
  std::cout << stats_text(lib.tax, device_taxon_counts(lib.dev.ix), lib.ip.m, o.histogram);
  std::cout.flush();
  return 0;
}
static int cmd_stats(int argc, char **argv) { return stats_or_inspect(false, argc, argv); }
static int cmd_inspect(int argc, char **argv) { return stats_or_inspect(true, argc, argv); }

// ---- respace (Slacken.scala:173-184, KeyValueIndex.respaceMultiple :390-404) and copy-records: the library writer's two users ----
static const char *RESPACE_USAGE = "usage: respace -i INDEX -o OUTPUT --spaces S [S ...] [--format parquet|slkrec] [--devices D]";
static const char *COPY_RECORDS_USAGE = "usage: copy-records -i INDEX -o OUTPUT [--format parquet|slkrec]";

// copy-records -i INDEX -o OUTPUT [--format parquet|slkrec]: a library's records read with the readers and written with the
// writer, with its properties and taxonomy (host only: the writer without a GPU)
static int cmd_copy_records(int argc, char **argv) {
  std::string index, output;
  LibraryWriter::Format format = LibraryWriter::AUTO;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") index = a.next();
    else if (a == "-o" || a == "--output") output = a.next();
    else if (a == "--format") format = LibraryWriter::parse_format(a.next());
    else die("unknown option " + a.opt + "\n" + COPY_RECORDS_USAGE);
  }
  if (index.empty() || output.empty()) die(COPY_RECORDS_USAGE);
  if (fs::weakly_canonical(index) == fs::weakly_canonical(output)) die("copy-records: OUTPUT is INDEX");
  const IndexParams ip = read_index_params(index);
  refuse_wide("copy-records", ip);
  LibraryWriter w(output, writer_properties(index, ip), index + "_taxonomy", format);
  for_each_record_batch(index, 1, [&](const int64_t *keys, const int32_t *taxa, uint64_t c) { w.add(keys, taxa, c); });
  w.finish();
  std::cerr << "copy-records: " << w.records() << " records written to " << output << std::endl;
  return 0;
}

// the first match of _s[0-9]+ in s (respaceMultiple's regex): its position and length, or false
static bool find_spaces_tag(const std::string &s, size_t *pos, size_t *len) {
  for (size_t at = s.find("_s"); at != std::string::npos; at = s.find("_s", at + 1)) {
    size_t e = at + 2;
    while (e < s.size() && s[e] >= '0' && s[e] <= '9') e++;
    if (e > at + 2) { *pos = at; *len = e - at; return true; }
  }
  return false;
}

// A resident table onto disk, piece by piece: slk_index_export_range over SLK_EXPORT_PIECE_BUCKETS table buckets at a time (default
// 2^23: 6.7e7 cells, a few tens of millions of records at the loads the table is sized for), grouped by Spark's bucket for the
// Parquet form so that the writer appends runs (n_groups 0 for .slkrec, which has no buckets).  Two pinned host buffers: a piece is
// written on a second thread while the next is exported.  Host memory is two pieces, whatever the table holds.
struct ExportTimes { double export_s = 0, write_wait_s = 0; uint64_t pieces = 0; };
static void export_to_writer(const slk_index *ix, LibraryWriter &w, int buckets, ExportTimes *times) {
  slk_index_info info;
  SLK_CALL(slk_index_get_info(ix, &info));
  const long env_piece = getenv("SLK_EXPORT_PIECE_BUCKETS") ? atol(getenv("SLK_EXPORT_PIECE_BUCKETS")) : 0;
  const uint64_t piece = std::min<uint64_t>(std::max<uint64_t>(info.buckets, 1), env_piece > 0 ? (uint64_t)env_piece : (uint64_t)1 << 23);
  const uint64_t cap = piece * (uint64_t)info.bucket_cells;   // an upper bound on a piece's records: never SLK_E_CAPACITY
  // (SLK_EXPORT_GROUPED=0: A/B switch of tools/bench_build.py -- pieces in any order, dealt into buckets by the writer on the host)
  const bool on_device = !(getenv("SLK_EXPORT_GROUPED") && getenv("SLK_EXPORT_GROUPED")[0] == '0');
  const int n_groups = w.parquet() && on_device ? buckets : 0;
  struct Piece {
    void *keys = nullptr, *taxa = nullptr;
    std::vector<uint64_t> offsets;
    uint64_t n = 0;
    ~Piece() { if (keys) slk_host_free(keys); if (taxa) slk_host_free(taxa); }
  } buf[2];
  for (Piece &p : buf) {
    SLK_CALL(slk_host_alloc(cap * 8, &p.keys));
    SLK_CALL(slk_host_alloc(cap * 4, &p.taxa));
    p.offsets.assign((size_t)n_groups + 1, 0);
  }
  std::future<void> writing;
  int at = 0;
  for (uint64_t b0 = 0; b0 < info.buckets; b0 += piece, at ^= 1) {
    Piece &p = buf[at];   // (its last write was waited for before the other buffer's began)
    const double t0 = wall_seconds();
    SLK_CALL(slk_index_export_range(ix, b0, std::min<uint64_t>(info.buckets, b0 + piece), n_groups, (int64_t *)p.keys, (int32_t *)p.taxa, cap,
                                    n_groups ? p.offsets.data() : nullptr, &p.n));
    const double t1 = wall_seconds();
    if (writing.valid()) writing.get();
    const double t2 = wall_seconds();
    if (times) { times->export_s += t1 - t0; times->write_wait_s += t2 - t1; times->pieces++; }
    writing = std::async(std::launch::async, [&w, &p, n_groups] {
      if (n_groups) w.add_grouped((const int64_t *)p.keys, (const int32_t *)p.taxa, p.offsets.data());
      else w.add((const int64_t *)p.keys, (const int32_t *)p.taxa, p.n);
    });
  }
  const double t2 = wall_seconds();
  if (writing.valid()) writing.get();
  if (times) times->write_wait_s += wall_seconds() - t2;
}

// ---- build (Slacken.scala:123-171): a library from the genomes of LIBRARY_DIR and the labels of LIBRARY_DIR/seqid2taxid.map ----
static const char *BUILD_USAGE =
    "usage: [--partitions N] build -i INDEX -t TAXONOMY_DIR -l LIBRARY_DIR [-k 35] [-m 31] [-s|--spaces 7] [--check] [--format parquet|slkrec] "
    "[--expected-records N] [--mask] [--base LIB] [--devices D]";
static int g_partitions = 200;          // --partitions, the reference's global option: `buckets` of a library that `build` writes
constexpr int BUILD_MAX_WINDOW = 28;    // m-mers per window the library builder takes (slk_index_add_sequences)

static bool is_nucleotide(char c) {     // what the scan takes for a base (BitRepresentation.charToTwobit: A C G T U, either case)
  switch (c) { case 'A': case 'C': case 'G': case 'T': case 'U': case 'a': case 'c': case 'g': case 't': case 'u': return true; default: return false; }
}

// KeyValueIndex.checkInput (KeyValueIndex.scala:57-76), host only: a sequence has a super-mer, so a minimizer, exactly when it has
// a window, a run of k valid bases; the counts of the records that share an id are summed, as the reference's groupBy does.
static int check_build_input(const std::string &library, int k) {
  std::map<std::string, bool> has_minimizer;
  for_each_library_sequence(library, [&](std::string_view h, std::string_view sq) {
    bool found = false;
    size_t run = 0;
    for (char c : sq) {
      run = is_nucleotide(c) ? run + 1 : 0;
      if (run >= (size_t)k) { found = true; break; }
    }
    bool &slot = has_minimizer[std::string(h)];
    slot = slot || found;
  });
  std::vector<std::vector<std::string>> rows;
  size_t none = 0;
  for (auto &e : has_minimizer) {
    if (e.second) continue;
    none++;
    // (Dataset.show(): the first 20 rows, cells cut to 20 characters)
    if (rows.size() < 20) rows.push_back({e.first.size() > 20 ? e.first.substr(0, 17) + "..." : e.first, "0"});
  }
  if (none) {
    std::cout << "Some input sequences had no minimizers (total " << none << "): \n" << show_table({"seqId", "sum"}, rows);
    if (none > 20) std::cout << "only showing top 20 rows\n\n";
  } else {
    std::cout << "Input sequences checked, all had minimizers.\n";
  }
  std::cout.flush();
  return 0;
}

// GenomeLibrary.inputStats (GenomeLibrary.scala:81-107) for the label file.  A label outside the taxonomy's arrays (the reference
// would throw) counts as undefined.
static std::string input_stats_text(const std::string &label_file, const std::vector<std::pair<std::string, Taxon>> &labels, const Taxonomy &tax) {
  std::set<Taxon> labelled;
  for (auto &lb : labels) labelled.insert(lb.second);
  auto defined = [&](Taxon t) { return t >= 0 && t < tax.size() && tax.isDefined(t); };
  std::vector<Taxon> invalid, valid;
  size_t non_leaf = 0;
  for (Taxon t : labelled) {
    (defined(t) ? valid : invalid).push_back(t);
    if (!stats_is_leaf(tax, t)) non_leaf++;
  }
  std::ostringstream o;
  if (!invalid.empty()) {
    o << invalid.size() << " unknown genomes in " << label_file << " were not indexed (missing from the taxonomy):\nList(";
    for (size_t i = 0; i < invalid.size(); i++) o << (i ? ", " : "") << invalid[i];
    o << ")\n";
  }
  if (non_leaf) o << non_leaf << " non-leaf genomes in " << label_file << "\n";
  TaxonCounts as_counts;
  for (Taxon t : valid) as_counts.emplace_back(t, 1);
  o << valid.size() << " valid taxa in input sequences described by " << label_file << " (maximal implied tree size "
    << stats_tree_size(tax, as_counts) << ")\n";
  o << "Max leaf nodes in resulting database: " << (long)valid.size() - (long)non_leaf << "\n";
  std::map<int, uint64_t> missing;
  for (Taxon t : valid) for (int level : tax.missingStepsToRoot(t)) missing[level]++;
  std::vector<std::vector<std::string>> rows;
  for (auto &e : missing) rows.push_back({std::to_string(e.first), std::to_string(e.second), rank_titles(e.first + 1)});
  o << show_table({"missingLevel", "count(missingLevel)", "label"}, rows);
  return o.str();
}

static int cmd_build(int argc, char **argv) {
  const char *why_one = "the library's table must fit one GPU";
  std::string index, taxonomy, library, ordering = "xor", base;
  int k = 35, m = 31, spaces = 7;
  bool check = false, mask = false, k_given = false, m_given = false, spaces_given = false;
  uint64_t expected = 0;
  std::vector<int> devices{0};
  LibraryWriter::Format format = LibraryWriter::AUTO;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") index = a.next();
    else if (a == "-t" || a == "--taxonomy") taxonomy = a.next();
    else if (a == "-l" || a == "--library") library = a.next();
    else if (a == "-k") { k = std::stoi(a.next()); k_given = true; }
    else if (a == "-m" || a == "--minimizer-width") { m = std::stoi(a.next()); m_given = true; }
    else if (a == "-s" || a == "--spaces") { spaces = std::stoi(a.next()); spaces_given = true; }
    else if (a == "--base") base = a.next();
    else if (a == "--ordering") ordering = a.next();
    else if (a == "--check") check = true;
    else if (a == "--mask") mask = true;
    else if (a == "--format") format = LibraryWriter::parse_format(a.next());
    else if (a == "--expected-records") expected = std::stoull(a.next());
    else if (a == "--devices") devices = parse_single_device(a.next(), "build", why_one);
    else if (a == "--shard-table") refuse_shard_table("build", why_one, BUILD_USAGE);
    else die("unknown option " + a.opt + "\n" + BUILD_USAGE);
  }
  if (index.empty() || taxonomy.empty() || library.empty()) die(BUILD_USAGE);
  // --base LIB: the splitter is LIB's (its records and the genomes' minimizers must be comparable); -k / -m / -s may repeat it
  if (!base.empty()) {
    const IndexParams bp = read_index_params(base);
    refuse_wide("build --base", bp);
    auto same = [&](const char *opt, bool given, int &mine, int theirs) {
      if (given && mine != theirs) die(std::string("build --base: ") + opt + " " + std::to_string(mine) + ", but " + base + " has " + std::to_string(theirs));
      mine = theirs;
    };
    same("-k", k_given, k, bp.k);
    same("-m", m_given, m, bp.m);
    same("-s", spaces_given, spaces, bp.spaces);
    if (bp.xorMask != SLK_DEFAULT_TOGGLE_MASK || !bp.canonical)
      die("build --base: " + base + " has another XORmask or is not canonical: build writes the default splitter only");
    if (fs::weakly_canonical(base) == fs::weakly_canonical(index)) die("build --base: INDEX is the base library");
  }
  // what this engine does not build is refused on the command line alone, before any file is read
  if (ordering != "xor" && ordering != "random")
    die("--ordering " + ordering + " is not supported by this engine (randomXOR only: xor or random)");
  if (m > k) die("-m must be <= -k");
  if (k < 1 || m < 1) die("-k and -m must be positive");
  if (m > 32) die("build supports minimizers of up to 32 nt (-m " + std::to_string(m) + ")");
  if (k - m + 1 > BUILD_MAX_WINDOW)
    die("build supports windows of up to " + std::to_string(BUILD_MAX_WINDOW) + " m-mers (k - m + 1 = " + std::to_string(k - m + 1) + ")");
  if (spaces < 0 || spaces > m / 2) die(std::to_string(spaces) + " spaces in minimizers of " + std::to_string(m) + " nt: at most " + std::to_string(m / 2));
  if (g_partitions < 1) die("--partitions must be positive");
  if (format == LibraryWriter::PARQUET && !parquet_available()) die("--format parquet: this build has no Parquet support");

  IndexParams ip{k, m, spaces, SLK_DEFAULT_TOGGLE_MASK, true};
  // (the reference prints the toString of a Scala object here; this line names the parameters in the engine's words)
  std::cout << "Splitter randomXOR k=" << ip.k << " m=" << ip.m << " XORmask=" << (int64_t)ip.xorMask << " canonical=true minimizerSpaces=" << ip.spaces << std::endl;
  if (check) return check_build_input(library, k);

  const Taxonomy tax = Taxonomy::load(taxonomy);
  const std::string label_file = library + "/seqid2taxid.map";
  const auto all_labels = read_label_map(library);
  std::unordered_map<std::string, Taxon> labels;   // KeyValueIndex.makeRecords :118-120: only defined taxa are indexed
  for (auto &lb : all_labels)
    if (lb.second >= 0 && lb.second < tax.size() && tax.isDefined(lb.second)) labels[lb.first] = lb.second;

  // the table: --expected-records, or classify2's estimate from the size of the genome files (distinct minimizers <= super-mers:
  // about 2 / (w + 1) per window on random sequence); it grows by itself when that proves too low
  const int w = k - m + 1;
  if (expected == 0) {
    uint64_t bytes = 0;
    for (auto &f : library_fna_files(library)) bytes += (uint64_t)fs::file_size(f);
    expected = (uint64_t)((double)bytes * std::min(1.0, 2.5 / (w + 1))) + 1024;
    if (!base.empty()) expected += library_record_count(base, 1);
  }
  DeviceIndex dev;
  dev.devices = devices;
  dev.create(ip, tax, expected, std::max<int32_t>(tax.size() - 1, 1));
  // --base: the base library's records first, translated into the taxonomy of -t; the genomes' minimizers merge into them by LCA
  if (!base.empty()) {
    Timer t("Merge base library " + base);
    const uint64_t n = merge_library_into(dev, base, tax);
    std::cerr << "build: --base " << base << ": " << n << " records merged into the table" << std::endl;
  }

  // the walk: batches of whole sequences of about SLK_BUILD_BATCH_BASES bases (a longer sequence is a batch of its own); the next
  // batch is read and parsed while slk_index_add_sequences runs on the last.  Host memory: two batches.
  const long env_batch = getenv("SLK_BUILD_BATCH_BASES") ? atol(getenv("SLK_BUILD_BATCH_BASES")) : 0;
  const uint64_t batch_bases = env_batch > 0 ? (uint64_t)env_batch : (uint64_t)1 << 30;
  struct Batch {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets{0};
    std::vector<int32_t> taxa;
    void clear() { bases.clear(); offsets.assign(1, 0); taxa.clear(); }
  } batch[2];
  int fill = 0;
  // --mask: every batch is uploaded once, masked where it lies with the defaults of `mask` (window 64, threshold 20) and scanned where
  // it lies; the files are not touched
  slk_stream *mask_st = nullptr;
  std::atomic<uint64_t> n_masked{0};
  if (mask) SLK_CALL(slk_stream_create(dev.ix, &mask_st));
  uint64_t n_seq = 0, n_bases = 0, n_batches = 0;
  double t_add = 0, t_wait = 0;
  std::future<std::pair<int32_t, std::string>> adding;
  auto wait_for_add = [&] {
    if (!adding.valid()) return;
    const double t0 = wall_seconds();
    const auto r = adding.get();
    t_wait += wall_seconds() - t0;
    if (r.first != SLK_OK) die("slk_index_add_sequences: " + r.second);
  };
  auto submit = [&] {
    Batch &b = batch[fill];
    if (b.taxa.empty()) return;
    wait_for_add();   // (the other buffer is free from here on)
    n_batches++;
    adding = std::async(std::launch::async, [&dev, &b, &t_add, mask_st, &n_masked] {
      const double t0 = wall_seconds();
      uint64_t masked = 0;
      const slk_mask_config mask_cfg{64, 20, (uint8_t)'x'};
      const int32_t rc = mask_st ? slk_index_add_sequences_masked(dev.ix, mask_st, b.bases.data(), b.offsets.data(), b.taxa.data(), b.taxa.size(), &mask_cfg, &masked)
                                 : slk_index_add_sequences(dev.ix, b.bases.data(), b.offsets.data(), b.taxa.data(), b.taxa.size());
      n_masked += masked;
      t_add += wall_seconds() - t0;   // (one add at a time: nobody else writes this)
      return std::make_pair(rc, std::string(rc == SLK_OK ? "" : slk_last_error()));
    });
    fill ^= 1;
    batch[fill].clear();
  };
  const double t_walk0 = wall_seconds();
  {
    Timer t("Build records");
    for_each_labelled_sequence(library, labels, [&](std::string_view sq, Taxon taxon) {
      if (!batch[fill].taxa.empty() && batch[fill].bases.size() + sq.size() > batch_bases) submit();
      Batch &b = batch[fill];
      b.bases.insert(b.bases.end(), sq.begin(), sq.end());
      b.offsets.push_back(b.bases.size());
      b.taxa.push_back(taxon);
      n_seq++; n_bases += sq.size();
    });
    submit();
    wait_for_add();
    if (mask_st) slk_stream_destroy(mask_st);
    SLK_CALL(slk_index_finalize(dev.ix));
  }
  const double t_walk = wall_seconds() - t_walk0;
  slk_index_info info;
  SLK_CALL(slk_index_get_info(dev.ix, &info));

  // writeRecords (KeyValueIndex.scala:125-139), IndexParams.write, Taxonomy.copyToLocation.  The writer keeps whatever library is at
  // INDEX until finish(): a failed build leaves nothing that loads, and an existing library is replaced only by a finished one.
  LibraryProperties lp;
  lp.k = k; lp.m = m; lp.spaces = spaces; lp.buckets = g_partitions; lp.xorMask = ip.xorMask; lp.canonical = true;
  ExportTimes et;
  const double t_write0 = wall_seconds();
  {
    Timer t("Write records to " + index);
    LibraryWriter wr(index, lp, taxonomy, format);
    export_to_writer(dev.ix, wr, lp.buckets, &et);
    wr.finish();
  }
  const double t_write = wall_seconds() - t_write0;
  if (mask) std::cerr << "build: --mask: " << n_masked.load() << " low-complexity letters masked on the device" << std::endl;
  std::cerr << "build: " << n_seq << " sequences, " << n_bases << " bases in " << n_batches << " batches, " << info.records << " records (table grown "
            << info.grown << " times); read and parse " << t_walk - t_wait << " s beside add_sequences " << t_add << " s (waited for it " << t_wait
            << " s); export " << et.export_s << " s in " << et.pieces << " pieces beside the writer (waited for it " << et.write_wait_s << " s), "
            << t_write << " s in all" << std::endl;
  // showIndexStats(None) and GenomeLibrary.inputStats (Slacken.scala:166-168)
  std::cout << index_stats_text(tax, device_taxon_counts(dev.ix), m) << input_stats_text(label_file, all_labels, tax);
  std::cout.flush();
  return 0;
}

// ---- merge: libraries united by LCA (merge.hpp).  The reference has no such command. ----
static const char *MERGE_USAGE =
    "usage: [--partitions N] merge -i OUT [-t TAXONOMY_DIR] [--format parquet|slkrec] [--expected-records N] [--devices D] LIB LIB [LIB ...]";

static int cmd_merge(int argc, char **argv) {
  const char *why_one = "the merged library's table must fit one GPU";
  std::string out, taxonomy;
  std::vector<std::string> sources;
  uint64_t expected = 0;
  std::vector<int> devices{0};
  LibraryWriter::Format format = LibraryWriter::AUTO;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") out = a.next();
    else if (a == "-t" || a == "--taxonomy") taxonomy = a.next();
    else if (a == "--format") format = LibraryWriter::parse_format(a.next());
    else if (a == "--expected-records") expected = std::stoull(a.next());
    else if (a == "--devices") devices = parse_single_device(a.next(), "merge", why_one);
    else if (a == "--shard-table") refuse_shard_table("merge", why_one, MERGE_USAGE);
    else if (a.opt.size() > 1 && a.opt[0] == '-') die("unknown option " + a.opt + "\n" + MERGE_USAGE);
    else sources.push_back(a.opt);
  }
  if (out.empty() || sources.empty()) die(MERGE_USAGE);
  if (g_partitions < 1) die("--partitions must be positive");
  if (format == LibraryWriter::PARQUET && !parquet_available()) die("--format parquet: this build has no Parquet support");
  const IndexParams ip = check_merge_sources(out, sources);   // (from the .properties files alone)

  if (taxonomy.empty()) taxonomy = sources[0] + "_taxonomy";
  const Taxonomy tax = Taxonomy::load(taxonomy);
  if (expected == 0)
    for (const std::string &s : sources) expected += library_record_count(s, 1);
  DeviceIndex dev;
  dev.devices = devices;
  dev.create(ip, tax, std::max<uint64_t>(expected, 1024), std::max<int32_t>(tax.size() - 1, 1));

  std::ostringstream per_source;
  const double t0 = wall_seconds();
  {
    Timer t("Merge records");
    for (const std::string &s : sources) per_source << (per_source.tellp() > 0 ? ", " : "") << s << " " << merge_library_into(dev, s, tax);
    SLK_CALL(slk_index_finalize(dev.ix));
  }
  const double t_merge = wall_seconds() - t0;
  slk_index_info info;
  SLK_CALL(slk_index_get_info(dev.ix, &info));

  // written as `build` writes: whatever library is at OUT is replaced only by a finished one
  LibraryProperties lp = writer_properties(sources[0], ip);
  lp.buckets = g_partitions;
  ExportTimes et;
  const double t_write0 = wall_seconds();
  {
    Timer t("Write records to " + out);
    LibraryWriter wr(out, lp, taxonomy, format);
    export_to_writer(dev.ix, wr, lp.buckets, &et);
    wr.finish();
  }
  std::cerr << "merge: records read: " << per_source.str() << "; " << info.records << " records out (table grown " << info.grown << " times); merge "
            << t_merge << " s; export " << et.export_s << " s in " << et.pieces << " pieces beside the writer (waited for it " << et.write_wait_s
            << " s), " << wall_seconds() - t_write0 << " s in all" << std::endl;
  std::cout << index_stats_text(tax, device_taxon_counts(dev.ix), ip.m);
  std::cout.flush();
  return 0;
}

// ---- mask: low-complexity masking of genome files before `build` (scripts/k2/mask_low_complexity.sh of the reference, which runs
// `k2mask -r x` over every .fna) ----
static const char *MASK_USAGE =
    "usage: mask [-l LIBRARY_DIR | FILES...] [--window 64] [--threshold 20] [--replace x | --soft] [--host] [--devices D]";

static int cmd_mask(int argc, char **argv) {
  const char *why_one = "masking runs on one GPU";
  std::vector<std::string> targets;
  slk_mask_config cfg{64, 20, (uint8_t)'x'};
  bool host = false;
  std::vector<int> devices{0};
  for (Args a(argc, argv); a.take();) {
    if (a == "-l" || a == "--library") targets.push_back(a.next());
    else if (a == "--window") cfg.window = (uint32_t)std::stoul(a.next());
    else if (a == "--threshold") cfg.threshold = (uint32_t)std::stoul(a.next());
    else if (a == "--replace") {
      const std::string v = a.next();
      if (v.size() != 1 || mask_code((uint8_t)v[0]) <= 3 || v[0] == '\n' || v[0] == '\r' || v[0] == '>')
        die("--replace takes one character that is no nucleotide letter\n" + std::string(MASK_USAGE));
      cfg.replacement = (uint8_t)v[0];
    }
    else if (a == "--soft") cfg.replacement = 0;
    else if (a == "--host") host = true;
    else if (a == "--devices") devices = parse_device_list(a.next());   // (one device: the first of the list)
    else if (a == "--shard-table") refuse_shard_table("mask", why_one, MASK_USAGE);
    else if (a.opt.size() > 1 && a.opt[0] == '-') die("unknown option " + a.opt + "\n" + MASK_USAGE);
    else targets.push_back(a.opt);
  }
  if (targets.empty()) die(MASK_USAGE);
  if (!mask_config_ok(cfg)) die("--window takes 8..64 and --threshold 1..255 (tenths, as k2mask -T)\n" + std::string(MASK_USAGE));
  // a directory: every *.fna below it; a file: itself
  std::vector<std::string> files;
  for (auto &t : targets) {
    if (fs::is_directory(t)) {
      std::vector<std::string> fna;
      for (auto &e : fs::recursive_directory_iterator(t))
        if (e.is_regular_file() && ends_with(e.path().string(), ".fna")) fna.push_back(e.path().string());
      std::sort(fna.begin(), fna.end());
      files.insert(files.end(), fna.begin(), fna.end());
    } else if (fs::is_regular_file(t)) {
      files.push_back(t);
    } else {
      die("Target " + t + " must be directory or regular file, aborting masking");
    }
  }
  slk_index *ix = nullptr;
  slk_stream *st = nullptr;
  if (!host) {
    const slk_params sp{35, 31, 7, 1, SLK_DEFAULT_TOGGLE_MASK, 1, 0};   // (a stream belongs to an index: an empty one of the default shape)
    const slk_table_config tc{1024, 0, 0.0f};
    SLK_CALL(slk_index_create(&sp, &tc, devices[0], &ix));
    SLK_CALL(slk_stream_create(ix, &st));
  }
  // pieces of whole records of about SLK_MASK_BATCH_BASES bytes of text (a longer record is a piece of its own): the next piece is read
  // while the last one is masked.  Host memory: two pieces.
  const long env_batch = getenv("SLK_MASK_BATCH_BASES") ? atol(getenv("SLK_MASK_BATCH_BASES")) : 0;
  const size_t piece_bytes = env_batch > 0 ? (size_t)env_batch : (size_t)1 << 28;
  const size_t threads = host_threads();
  MaskTotals totals;
  uint64_t skipped = 0, done = 0;
  const double t0 = wall_seconds();
  int status = 0;
  for (auto &f : files) {
    if (fs::exists(f + ".masked")) { skipped++; continue; }
    std::string error;
    const bool ok = mask_file(f, piece_bytes, [&](uint8_t *bases, const uint64_t *offsets, uint64_t n) -> uint64_t {
      if (host) return mask_sequences_host(bases, offsets, n, cfg, threads);
      uint64_t masked = 0;
      if (slk_mask_sequences(st, bases, offsets, n, &cfg, &masked) != SLK_OK) {
        remove((f + ".tmp").c_str());   // (the file itself is as it was)
        die(std::string("slk_mask_sequences: ") + slk_last_error());
      }
      return masked;
    }, &totals, &error);
    if (!ok) { std::cerr << "slacken-amd: mask: " << error << std::endl; status = 2; break; }
    done++;
  }
  if (st) slk_stream_destroy(st);
  if (ix) slk_index_destroy(ix);
  std::cout << "mask: " << done << " files, " << totals.letters << " letters read, " << totals.masked << " letters masked, " << skipped
            << " files skipped (already masked), " << wall_seconds() - t0 << " s" << (host ? " on the host" : "") << std::endl;
  return status;
}

// ---- compare (Slacken.scala:343-366): MappingComparison.processFiles / processDirectories.  compare.hpp has the contract; here are
// the options, the readers and the joiner on the device ----
static const char *COMPARE_USAGE =
    "usage: compare -t TAXONOMY_DIR -r REFERENCE -o OUTPUT [--id-col 2] [-T|--taxon-col 3] [--header] (--test-files F... | --multi-dirs D...) "
    "[--devices D] [--host]";

// the join of slk_compare_*: one small empty index and a stream own the handle
class DeviceJoin : public CompareJoiner {
  slk_index *ix_ = nullptr;
  slk_stream *st_ = nullptr;
  slk_compare *h_ = nullptr;

  size_t done(int32_t rc, const char *call, uint64_t consumed) {
    if (rc == SLK_OK) return (size_t)consumed;
    uint64_t at = 0;
    int32_t kind = SLK_COMPARE_NO_ERROR;
    if (rc == SLK_E_INVALID && slk_compare_error(h_, &at, &kind) == SLK_OK && kind != SLK_COMPARE_NO_ERROR) throw CompareTextError{at, kind};
    die(std::string(call) + ": " + slk_last_error());
  }

 public:
  explicit DeviceJoin(int device) {
    const slk_params sp{35, 31, 7, 1, SLK_DEFAULT_TOGGLE_MASK, 1, 0};   // (a stream belongs to an index: an empty one of the default shape)
    const slk_table_config tc{1024, 0, 0.0f};
    SLK_CALL(slk_index_create(&sp, &tc, device, &ix_));
    SLK_CALL(slk_stream_create(ix_, &st_));
    SLK_CALL(slk_compare_create(st_, &h_));
  }
  ~DeviceJoin() override {
    slk_compare_destroy(h_);
    slk_stream_destroy(st_);
    slk_index_destroy(ix_);
  }
  size_t add_reference(const char *p, size_t n, int id_col, int taxon_col, bool final) override {
    uint64_t consumed = 0;
    const int32_t rc = slk_compare_add_reference(h_, st_, (const uint8_t *)p, n, id_col, taxon_col, final ? 1 : 0, &consumed);
    return done(rc, "slk_compare_add_reference", consumed);   // (the call first: it writes `consumed`)
  }
  void begin_test() override { SLK_CALL(slk_compare_begin_test(h_)); }
  size_t add_test(const char *p, size_t n, bool final) override {
    uint64_t consumed = 0;
    const int32_t rc = slk_compare_add_test(h_, st_, (const uint8_t *)p, n, final ? 1 : 0, &consumed);
    return done(rc, "slk_compare_add_test", consumed);
  }
  CompareCounts counts() override {
    CompareCounts c;
    uint64_t n = 0;
    SLK_CALL(slk_compare_pairs(h_, &n, nullptr, nullptr, nullptr, 0));
    std::vector<int32_t> a(n), b(n);
    std::vector<uint64_t> rows(n);
    if (n) SLK_CALL(slk_compare_pairs(h_, &n, a.data(), b.data(), rows.data(), n));
    for (uint64_t i = 0; i < n; i++) c.pairs.push_back({a[i], b[i], rows[i]});
    SLK_CALL(slk_compare_reference_taxa(h_, &n, nullptr, nullptr, 0));
    a.resize(n); rows.resize(n);
    if (n) SLK_CALL(slk_compare_reference_taxa(h_, &n, a.data(), rows.data(), n));
    for (uint64_t i = 0; i < n; i++) c.ref_taxa.emplace_back(a[i], rows[i]);
    SLK_CALL(slk_compare_totals(h_, &c.reference_rows, &c.dropped_second, &c.kept_ids, &c.test_rows, &c.joined_rows));
    return c;
  }
};

static int cmd_compare(int argc, char **argv) {
  const char *why_one = "the reference mapping is joined on one GPU";
  std::string taxonomy_dir, reference, output;
  std::vector<std::string> test_files, multi_dirs;
  int id_col = 2, taxon_col = 3;
  bool header = false, host = false, have_files = false, have_dirs = false;
  std::vector<int> devices{0};
  for (Args a(argc, argv); a.take();) {
    auto list = [&](std::vector<std::string> &into) {
      while (a.peek() && a.peek()[0] != '-') into.push_back(a.next());
    };
    if (a == "-t" || a == "--taxonomy") taxonomy_dir = a.next();
    else if (a == "-r" || a == "--reference") reference = a.next();
    else if (a == "-o" || a == "--output") output = a.next();
    else if (a == "--id-col") id_col = std::stoi(a.next());
    else if (a == "-T" || a == "--taxon-col") taxon_col = std::stoi(a.next());
    else if (a == "--header") header = true;
    else if (a == "--noheader") header = false;
    else if (a == "--test-files") { have_files = true; list(test_files); }
    else if (a == "--multi-dirs") { have_dirs = true; list(multi_dirs); }
    else if (a == "--host") host = true;
    else if (a == "--devices") devices = parse_single_device(a.next(), "compare", why_one);
    else if (a == "--shard-table") refuse_shard_table("compare", why_one, COMPARE_USAGE);
    else die("unknown option " + a.opt + "\n" + COMPARE_USAGE);
  }
  if (taxonomy_dir.empty() || reference.empty() || output.empty()) die(COMPARE_USAGE);
  if (have_files == have_dirs) die("compare takes exactly one of --test-files and --multi-dirs\n" + std::string(COMPARE_USAGE));
  if ((have_files ? test_files : multi_dirs).empty()) die(std::string(have_files ? "--test-files" : "--multi-dirs") + " names nothing\n" + COMPARE_USAGE);
  if (id_col < 1 || taxon_col < 1 || id_col == taxon_col) die("--id-col and --taxon-col are two columns, counted from 1\n" + std::string(COMPARE_USAGE));
  const Taxonomy tax = Taxonomy::load(taxonomy_dir);
  std::vector<std::pair<std::string, std::string>> locations;   // (test location, its reference mapping)
  if (have_files) for (auto &f : test_files) locations.emplace_back(f, reference);
  else {
    for (auto &d : multi_dirs) if (!fs::is_directory(d)) die(d + " is no directory");
    locations = compare_multi_locations(multi_dirs, reference);
  }
  const long env_chunk = getenv("SLK_COMPARE_CHUNK") ? atol(getenv("SLK_COMPARE_CHUNK")) : 0;
  const size_t chunk = env_chunk > 0 ? (size_t)env_chunk : (size_t)64 << 20;
  const char *kinds[] = {"", "too few columns, an empty id or taxon field, or a taxon that is no non-negative int", "this id occurs twice among the kept reference rows",
                         "this id occurs twice among the test rows that have a reference row"};
  // where in which file a joiner's offset lies, and the run ends
  auto text_error = [&](const CompareTextError &e, const std::vector<std::pair<std::string, uint64_t>> &files, int idc, int txc) {
    size_t fi = 0;
    while (fi + 1 < files.size() && files[fi + 1].second <= e.offset) fi++;
    ByteSource src(files[fi].first);
    std::string text;
    const uint64_t line = locate_line([&](char *dst, size_t cap) { return src.read(dst, cap); }, e.offset - files[fi].second, text);
    std::string_view id;
    int32_t taxon = 0;
    std::string what = kinds[e.kind];
    if (e.kind != COMPARE_BAD_LINE && compare_fields(text.data(), text.size(), idc - 1, txc - 1, id, taxon)) what += " (" + std::string(id) + ")";
    die("compare: " + files[fi].first + " line " + std::to_string(line) + ": " + what);
  };
  std::map<std::string, std::unique_ptr<CompareJoiner>> resident;   // by reference mapping: uploaded once
  std::vector<std::string> rows{compare_metrics_header()}, late;
  const double t0 = wall_seconds();
  double t_reference = 0, t_tests = 0;
  for (auto &loc : locations) {
    std::unique_ptr<CompareJoiner> &join = resident[loc.second];
    if (!join) {
      const double t1 = wall_seconds();
      if (host) join = std::make_unique<HostJoin>();
      else join = std::make_unique<DeviceJoin>(devices[0]);
      uint64_t skipped = 0;   // (the header's bytes are not given to the joiner: its offsets lie that much lower)
      try {
        ByteSource src(loc.second);
        feed_text([&](char *dst, size_t cap) { return src.read(dst, cap); }, chunk, header,
                  [&](const char *p, size_t n, bool final) { return join->add_reference(p, n, id_col, taxon_col, final); }, &skipped);
      } catch (CompareTextError &e) {
        e.offset += skipped;
        text_error(e, {{loc.second, 0}}, id_col, taxon_col);
      }
      t_reference += wall_seconds() - t1;
    }
    const double t1 = wall_seconds();
    join->begin_test();
    std::vector<std::pair<std::string, uint64_t>> files;
    uint64_t base = 0;
    try {
      for (auto &f : compare_location_files(loc.first)) {
        files.emplace_back(f, base);
        ByteSource src(f);
        feed_text([&](char *dst, size_t cap) { return src.read(dst, cap); }, chunk, false, [&](const char *p, size_t n, bool final) {
          const size_t used = join->add_test(p, n, final);
          base += used;
          return used;
        });
      }
    } catch (const CompareTextError &e) {
      text_error(e, files, 2, 3);
    }
    LocationMetrics m;
    std::cout << location_report(tax, join->counts(), loc.first, have_dirs, m) << std::flush;
    for (int ri = 0; ri < 2; ri++) {
      std::string row;
      (metrics_row(m, ri, row) ? rows : late).push_back(row);
    }
    t_tests += wall_seconds() - t1;
  }
  for (auto &l : late) std::cout << l << "\n";
  std::ofstream out = open_output(output + "_metrics.tsv");
  for (auto &r : rows) out << r << "\n";
  out.close();
  if (!out) die("cannot write " + output + "_metrics.tsv");
  std::cerr << "compare: " << locations.size() << " locations, " << resident.size() << " reference mappings (" << t_reference << " s), tests "
            << t_tests << " s, " << wall_seconds() - t0 << " s in all" << (host ? " on the host" : "") << std::endl;
  return 0;
}

// ---- coverage: the genome coverage of IndexStatistics (S/slacken/IndexStatistics.scala:38-52, 86-111), behind a command of its own.
// The reference reaches it through `stats --library`, `inspect --library` and `classify2 --index-reports`; those stay refused here.
static const char *COVERAGE_USAGE = "usage: coverage -i INDEX -l LIBRARY_DIR -o OUTPUT [--devices D]";

static int cmd_coverage(int argc, char **argv) {
  const char *why_one = "the library's table must fit one GPU";
  CoverageOptions o;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") o.index = a.next();
    else if (a == "-l" || a == "--library") o.library = a.next();
    else if (a == "-o" || a == "--output") o.output = a.next();
    else if (a == "--devices") o.devices = parse_single_device(a.next(), "coverage", why_one);
    else if (a == "--shard-table") refuse_shard_table("coverage", why_one, COVERAGE_USAGE);
    else die("unknown option " + a.opt + "\n" + COVERAGE_USAGE);
  }
  if (o.index.empty() || o.library.empty() || o.output.empty()) die(COVERAGE_USAGE);
  const IndexParams ip = read_index_params(o.index);
  refuse_wide("coverage", ip);
  if (ip.k - ip.m + 1 > BUILD_MAX_WINDOW)
    die("coverage supports windows of up to " + std::to_string(BUILD_MAX_WINDOW) + " m-mers (k - m + 1 = " + std::to_string(ip.k - ip.m + 1) + ")");
  // GenomeLibrary.joinSequencesAndLabels (GenomeLibrary.scala:50-57): the sequences joined with the labels by header -- every
  // label, with no isDefined filter (unlike `build`: the source taxon is only carried)
  std::unordered_map<std::string, Taxon> labels;
  for (auto &lb : read_label_map(o.library)) labels[lb.first] = lb.second;
  return coverage_run(o, [&](auto fn) { for_each_labelled_sequence(o.library, labels, fn); });
}

// ---- support: the sample support reports of Dynamic.reportDynamicIndexSupport (S/slacken/Dynamic.scala:210-228), behind a command of
// its own as `coverage` is; `classify2 --index-reports` stays refused.  The two coverage files of that method are `coverage`'s.
static int cmd_support(int argc, char **argv) {
  SupportOptions o = parse_support_options(argc, argv);
  const IndexParams ip = read_index_params(o.index);
  refuse_wide("support", ip);
  if (ip.k - ip.m + 1 > BUILD_MAX_WINDOW)
    die("support supports windows of up to " + std::to_string(BUILD_MAX_WINDOW) + " m-mers (k - m + 1 = " + std::to_string(ip.k - ip.m + 1) + ")");
  note_one_support_device(o.devices);
  o.devices.resize(1);
  const double t0 = wall_seconds();
  LoadedIndex lib(o.index, o.devices);
  const SupportCounts c = support_pass(lib.dev, lib.tax, o.files, o.paired, o.rank_depth, true);
  // Classifier.classify(subjects, cpar, 0.0) grouped by taxon (multiStatsPerTaxon :160-162): the detection pass of classify2 -R at
  // confidence 0, titles regrouped
  ClassifyOpts co;
  co.files = o.files; co.paired = o.paired; co.min_hits = o.min_hits; co.init_confidence = 0.0;
  const TaxonSupport classified = support_by_classified_reads(lib.dev, co);
  write_support_files(lib.tax, c.rows, std::vector<std::pair<Taxon, long>>(classified.begin(), classified.end()), o.output);
  std::cout << "support: " << c.sequences << " sequences, " << c.supermers << " super-mers, " << c.matched << " matched, " << c.kept << " at rank "
            << o.rank << " or below, " << c.rows.size() << " taxa, " << wall_seconds() - t0 << " s" << std::endl;
  return 0;
}

// coverage-report TAXONOMY_DIR COUNTS_TSV SIZES_TSV ROWS_TSV OUTPUT: the three files `coverage` writes, from "taxon \t records",
// "source \t k-mers" and "source \t depth \t all \t distinct" lines (host only: the outputs without a GPU)
static int cmd_coverage_report(int argc, char **argv) {
  if (argc != 5) die("usage: coverage-report TAXONOMY_DIR COUNTS_TSV SIZES_TSV ROWS_TSV OUTPUT");
  const Taxonomy tax = Taxonomy::load(argv[0]);
  std::map<Taxon, uint64_t> records, sizes;
  long long t, d;
  unsigned long long c, c2;
  std::ifstream f1 = open_input(argv[1]);
  while (f1 >> t >> c) records[(Taxon)t] += c;
  std::ifstream f2 = open_input(argv[2]);
  while (f2 >> t >> c) sizes[(Taxon)t] += c;
  std::vector<CoverageRow> rows;
  std::ifstream f3 = open_input(argv[3]);
  while (f3 >> t >> d >> c >> c2) rows.push_back({(int32_t)t, (int32_t)d, c, c2});
  std::sort(rows.begin(), rows.end(), [](const CoverageRow &a, const CoverageRow &b) { return a.source != b.source ? a.source < b.source : a.depth < b.depth; });
  write_coverage_files(tax, TaxonCounts(records.begin(), records.end()), std::vector<std::pair<Taxon, uint64_t>>(sizes.begin(), sizes.end()), rows, argv[4]);
  return 0;
}

static int cmd_respace(int argc, char **argv) {
  std::string index, output;
  std::vector<int> spaces, devices{0};
  LibraryWriter::Format format = LibraryWriter::AUTO;
  for (Args a(argc, argv); a.take();) {
    if (a == "-i" || a == "--index") index = a.next();
    else if (a == "-o" || a == "--output") output = a.next();
    else if (a == "--format") format = LibraryWriter::parse_format(a.next());
    else if (a == "-s" || a == "--spaces") { while (a.peek() && a.peek()[0] >= '0' && a.peek()[0] <= '9') spaces.push_back(std::stoi(a.next())); }
    else if (a == "--devices") devices = parse_single_device(a.next(), "respace", "both tables must fit one GPU");
    else if (a == "--shard-table") refuse_shard_table("respace", "both tables must fit one GPU", RESPACE_USAGE);
    else die("unknown option " + a.opt + "\n" + RESPACE_USAGE);
  }
  if (index.empty() || output.empty() || spaces.empty()) die(RESPACE_USAGE);
  size_t tag_at = 0, tag_len = 0;
  if (!find_spaces_tag(output, &tag_at, &tag_len)) die("Unable to guess the correct output location for new indexes at: " + output);
  if (format == LibraryWriter::PARQUET && !parquet_available()) die("--format parquet: this build has no Parquet support");
  refuse_wide("respace", read_index_params(index));
  LoadedIndex lib(index, devices);
  LibraryProperties lp = writer_properties(index, lib.ip);
  for (int s : spaces) {
    const std::string out_loc = output.substr(0, tag_at) + "_s" + std::to_string(s) + output.substr(tag_at + tag_len);
    Timer t("Respace to " + out_loc);
    slk_index *nx = nullptr;
    SLK_CALL(slk_index_respace(lib.dev.ix, s, nullptr, &nx));   // (an s not above the library's own: the reference's wording, and the end)
    std::unique_ptr<slk_index, void (*)(slk_index *)> owner(nx, slk_index_destroy);
    lp.spaces = s;
    LibraryWriter w(out_loc, lp, index + "_taxonomy", format);
    export_to_writer(nx, w, lp.buckets, nullptr);
    w.finish();
    std::cout << "Stats for " << out_loc << "\n" << index_stats_text(lib.tax, device_taxon_counts(nx), lib.ip.m);
    std::cout.flush();
  }
  return 0;
}

static const char *HELP =
    "slacken-amd -- Slacken's classify path on an MI355X (libslacken_amd.so)\n"
    "  slacken-amd [--partitions N] classify  -i INDEX -o OUTPUT [options] FILES...\n"
    "  slacken-amd [--partitions N] classify2 -i INDEX -o OUTPUT --library DIR [options] FILES...\n"
    "options of both (the reference's `classify`, Slacken.scala:66-100):\n"
    "  -i, --index LOC        library location: LOC.properties, LOC_taxonomy/{nodes,names}.dmp, LOC/*.parquet (or LOC.slkrec)\n"
    "  -o, --output PREFIX    writes PREFIX_c<threshold>/sample=<id>/part-*.txt.gz and PREFIX_c<threshold>/<id>_kreport.txt\n"
    "  -c, --confidence T...  confidence thresholds in [0, 1] (default 0.0)\n"
    "      --min-hits N       distinct minimizer hits needed to classify (default 2)\n"
    "  -p, --paired           FILES are pairs (file_1 file_2 ...), joined by read id without /1 /2\n"
    "      --sample-regex RE  group 1 of the first match in the read id names the sample (\"other\" without a match).  The dialect is\n"
    "                         std::regex's ECMAScript, not java.util.regex: no possessive quantifiers, look-behind, \\p{..} or named\n"
    "                         groups; character classes, alternation, greedy and lazy quantifiers, look-ahead and back-references\n"
    "                         behave alike.  A match in which group 1 took no part names the sample \"null\", as the reference does\n"
    "      --[no]unclassified keep (default) or drop unclassified reads\n"
    "      --[no]detailed     per-read output (default) or reports only\n"
    "      --devices LIST     GPUs that share the reads, `all` or e.g. 0,1,2,3 (default 0); the library is replicated on each\n"
    "      --shard-table      classify: spread the library over the devices instead (each holds the records whose minimizer falls to it;\n"
    "                         minimizers travel to their owners and taxa back): for a library beyond one GPU's memory\n"
    "      --device-parse     classify: send the files' text to the device as it is and find the records there (unpaired input, a\n"
    "                         replicated table, m <= 32; `parse --device FILE` shows what the device finds); the default parses on the host\n"
    "      --split-long LEN   classify: split unpaired sequences of at least LEN bases (contigs, assemblies) over many waves of the\n"
    "                         device; the results do not change.  Takes effect where no per-read lines are written (--nodetailed:\n"
    "                         those need hit lists, which keep the other routes unless --split-hits is given); not with -p or\n"
    "                         --shard-table.  0: never\n"
    "      --split-hits       classify, with --split-long LEN (LEN > 0): split those sequences also where per-read lines are written --\n"
    "                         their hit lists are put together from the pieces; the files do not change\n"
    "      --device-pairs     classify -p: send both mate files' text to the device, which finds the records and pairs them in lockstep\n"
    "                         (a replicated table, m <= 32); mates that are out of order end the run -- the default joins them on the host\n"
    "  FILES                  FASTA / FASTQ, plain, .gz or .bz2; @list.txt names a file of file names\n"
    "options of classify2 (Slacken.scala:199-260): --library DIR (DIR/library/**/*.fna, DIR/seqid2taxid.map), --rank RANK (species),\n"
    "  -R, --reads N (100) | -C, --min-count N | -D, --min-distinct N, --init-confidence X (0.15)\n"
    "  -g, --gold-set FILE (a taxon per line: the detected set is compared with it), --classify-with-gold (the dynamic library is built\n"
    "  from the gold set instead of a detected one), --promote-gold-set RANK (gold taxa without sequence in the library: keep the\n"
    "  ancestors they are promoted to down to RANK), --bracken-length L (Bracken weights of the dynamic library's genomes for reads of\n"
    "  length L, written to OUTPUT/databaseLmers.kmer_distrib)\n"
    "  slacken-amd bracken-build -i INDEX --library DIR [--read-len L (100)] [--devices LIST] (Slacken.scala:264-279): Bracken weights\n"
    "  of every genome of DIR labelled in DIR/seqid2taxid.map, written to INDEX_bracken/databaseLmers.kmer_distrib; the records are\n"
    "  shared out over the devices\n"
    "  slacken-amd compare-index -i SUBJECT -r REFERENCE -o OUTPUT [--devices D] (also spelled compareIndex; Slacken.scala:332-341):\n"
    "  the records of library SUBJECT joined on the minimizer with those of library REFERENCE (normally a superset; its table goes to\n"
    "  one GPU).  stdout: how many records moved up by how many standard ranks; OUTPUT_taxaToRoot_report.txt: a Kraken report of the\n"
    "  taxa whose minimizers went to the root or to cellular organisms.  Both libraries must share k, m, spaces, mask and canonical\n"
    "  slacken-amd compare -t TAXONOMY_DIR -r REFERENCE -o OUTPUT [--id-col 2] [-T|--taxon-col 3] [--header] (--test-files F... |\n"
    "  --multi-dirs D...) [--devices D] [--host] (Slacken.scala:343-366, MappingComparison.scala): the per-read lines `classify` wrote are\n"
    "  joined on the read id with a truth mapping (TSV; rows whose id holds /2 are dropped, every /1 is removed from the others' ids) -- on\n"
    "  the GPU, byte for byte, the mapping resident and uploaded once per file.  Per test location and for the ranks Genus and Species:\n"
    "  true, vague and false positives and false negatives per read, precision and recall per taxon (a taxon counts with 10 reads); stdout\n"
    "  has the reference's lines, OUTPUT_metrics.tsv one row per location and rank whose title has the shape\n"
    "  FAMILY/GROUP/LIBRARY_K_M_sS_cC_classified/sample=ID (any other title is reported and left out, as by the reference -- so always\n"
    "  with --test-files, whose title is the file name).  --test-files: files, or directories of part files (names beginning with _ or .\n"
    "  are skipped; plain, .gz, .bz2), all against REFERENCE.  --multi-dirs: every subdirectory sample=ID of every D against\n"
    "  REFERENCE/sampleID/reads_mapping.tsv, e.g. what `classify -o OUT --sample-regex ... -c 0.15` left, renamed to the shape above:\n"
    "    slacken-amd compare -t TAX -r TRUTH -o eval --multi-dirs fam/grp/std_35_31_s7_c0.15_classified\n"
    "  --header drops the first non-empty line of REFERENCE.  --host: the same command with the join in a host hash map (no GPU is\n"
    "  opened).  Unlike the reference, which throws or silently multiplies rows: a line with too few columns, an empty id or taxon, or\n"
    "  a taxon that is no non-negative int ends the run naming file and line; so does a taxon outside the taxonomy, an id that occurs\n"
    "  twice among the kept reference rows, and an id that occurs twice among the test rows that have a reference row.  Ids containing\n"
    "  a double quote are not pinned against Spark's CSV reader.  One device\n"
    "  slacken-amd stats -i INDEX [--histogram] [--devices D] (Slacken.scala:281-315): the splitter's masks, then how many taxa the\n"
    "  library stores, how many of them are leaves and how many records lie on leaves; with --histogram the records and the stored\n"
    "  taxa by rank depth instead.  Counted on the GPU from the resident table (--library, the genome coverage check, is not supported)\n"
    "  slacken-amd inspect -i INDEX -o OUTPUT [--labels FILE] [--devices D] (Slacken.scala:317-330): Kraken-style reports of the\n"
    "  library's contents, OUTPUT_min_report.txt (records per taxon) and OUTPUT_genome_report.txt (one per stored taxon); with\n"
    "  --labels (seqid TAB taxon lines) OUTPUT_missing_report.txt of the labelled taxa the library does not store\n"
    "  slacken-amd respace -i INDEX -o OUTPUT --spaces S [S ...] [--format parquet|slkrec] [--devices D] (Slacken.scala:173-184): for\n"
    "  each S above the library's own minimizerSpaces, in the order given, the library at S spaces derived on the GPU from the resident\n"
    "  table (keys masked, records regrouped by LCA; no genome is read) and written to OUTPUT with its first _s<digits> replaced by\n"
    "  _sS -- .properties, _taxonomy and the records as bucketed Parquet (as .slkrec with --format slkrec or without Arrow) -- followed\n"
    "  by `Stats for <location>` and the two lines `stats` prints\n"
    "  slacken-amd [--partitions N] build -i INDEX -t TAXONOMY_DIR -l LIBRARY_DIR [-k 35] [-m 31] [-s|--spaces 7] [--check]\n"
    "  [--format parquet|slkrec] [--expected-records N] [--mask] [--base LIB] [--devices D] (Slacken.scala:123-171): a library from the genomes of\n"
    "  LIBRARY_DIR/library/**/*.fna labelled in LIBRARY_DIR/seqid2taxid.map -- minimizers found and merged by LCA on the GPU, the table\n"
    "  exported piece by piece, grouped by Spark's bucket, into --partitions (200) Parquet files (or INDEX.slkrec), with\n"
    "  INDEX.properties and a copy of TAXONOMY_DIR as INDEX_taxonomy -- followed by the two lines `stats` prints and the label file's\n"
    "  statistics.  --check only reports the sequences without a minimizer (host only, nothing is written).  --mask: every batch of\n"
    "  genomes is masked on the GPU as `mask` would with its defaults (window 64, threshold 20, letters replaced by x) before it is\n"
    "  scanned, so low-complexity sequence yields no minimizers; the files are not touched (--check ignores it).  --base LIB: the\n"
    "  records of the library LIB, translated into TAXONOMY_DIR, are merged into the table before the genomes are walked -- genomes\n"
    "  added to a library whose own genomes are not at hand; -k, -m and -s default to LIB's and are refused when they differ from them\n"
    "  slacken-amd [--partitions N] merge -i OUT [-t TAXONOMY_DIR] [--format parquet|slkrec] [--expected-records N] [--devices D]\n"
    "  LIB LIB [LIB ...] (no counterpart in the reference): the libraries united on the GPU -- every record of every LIB into one table,\n"
    "  the taxa of a shared minimizer merged by LCA, which under one taxonomy is the library `build` makes of all their genomes; no\n"
    "  genome is read.  The taxonomy is TAXONOMY_DIR or the first LIB's; every LIB's taxa are translated into it (its merged.dmp is\n"
    "  honoured) and a taxon it lacks ends the run with nothing written.  The libraries must share k, m, minimizerSpaces, XORmask and\n"
    "  canonical (m <= 32).  Written as `build` writes, into --partitions (200) Parquet files or OUT.slkrec, followed by the two lines\n"
    "  `stats` prints.  One device\n"
    "  slacken-amd mask [-l LIBRARY_DIR | FILES...] [--window 64] [--threshold 20] [--replace x | --soft] [--host] [--devices D]\n"
    "  (scripts/k2/mask_low_complexity.sh, which runs `k2mask -r x` before a library is built): low-complexity masking of genome files\n"
    "  on the GPU -- symmetric DUST (Morgulis et al. 2006) with a window of 8..64 letters and a threshold of 1..255 tenths, as k2mask\n"
    "  -W / -T.  Of a directory every *.fna below it is taken; a file with FILE.masked beside it is skipped; otherwise the masked text\n"
    "  goes to FILE.tmp, which is renamed over FILE, and FILE.masked is created.  Masked letters become x (--replace C: the character\n"
    "  C; --soft: their lower-case form).  Unlike k2mask, which re-wraps lines, the output differs from the input ONLY in the masked\n"
    "  letters: header lines, line breaks and line lengths stay byte for byte (a .fai index made beforehand stays valid); line breaks\n"
    "  inside a sequence do not end a run; every record is masked.  Equality with k2mask's own output is not pinned.  --host: the same\n"
    "  function on the CPU (no GPU is opened).  One device: the first of --devices.  Prints letters read, letters masked, files skipped\n"
    "  slacken-amd coverage -i INDEX -l|--library LIBRARY_DIR -o OUTPUT [--devices D] (IndexStatistics.scala:38-52, 86-111; the reference's\n"
    "  `stats --library`, `inspect --library` and `classify2 --index-reports` reach this arithmetic, here those flags stay refused): every\n"
    "  genome of LIBRARY_DIR labelled in LIBRARY_DIR/seqid2taxid.map is scanned on the GPU and every super-mer's minimizer looked up in\n"
    "  INDEX's resident table.  OUTPUT_support_report_minimizerCoverage.txt and OUTPUT_support_report_minimizerDistinctCoverage.txt: per\n"
    "  source taxon `<taxon>  <depth>:<count>|..`, its minimizers (with repetitions / distinct) by the rank depth of the LCA taxon the\n"
    "  library stores for them; OUTPUT_min_report.txt: the Kraken report of `inspect` with the columns TKC1-LeafOnly, TKC2-FirstChildren and\n"
    "  TKC3-AllChildren (average k-mers per genome).  A library with more super-mers than the GPU's memory takes at once is counted in\n"
    "  groups of source taxa, one pass over LIBRARY_DIR each\n"
    "  slacken-amd support -i INDEX -o OUTPUT [--rank RANK (species)] [--min-hits N] [-p] [--devices D] FILES... (Dynamic.scala:152-180,\n"
    "  210-228; the sample support reports of the reference's `classify2 --index-reports`): every super-mer of every read (FILES as for\n"
    "  classify, ambiguous regions kept) is looked up on the GPU, the hits whose taxon lies at RANK or below are grouped by taxon, and\n"
    "  four Kraken reports are written: OUTPUT_support_report_totalKmerCount.txt (k-mers of the hit super-mers),\n"
    "  OUTPUT_support_report_totalMinimizerCount.txt (hit super-mers), OUTPUT_support_report_distinctMinimizerCount.txt (different\n"
    "  minimizers among them) and OUTPUT_support_report_classifiedReadCount.txt (reads classified at confidence 0, --min-hits as for\n"
    "  classify).  The counts are taken on one device, the first of --devices; the two coverage files are written by `coverage`\n"
    "host-only helpers: copy-records -i INDEX -o OUTPUT [--format parquet|slkrec] (a library rewritten by the library writer) |\n"
    "  report TAXONOMY_DIR COUNTS_TSV | kmer-distrib TRIPLES_TSV (dest source count) |\n"
    "  stats-report TAXONOMY_DIR COUNTS_TSV (taxon count) M [--histogram] [-o OUTPUT [--labels FILE]] |\n"
    "  migration-report SUBJECT_TAXONOMY_DIR REFERENCE_TAXONOMY_DIR PAIRS_TSV (t1 t2 count) OUTPUT |\n"
    "  coverage-report TAXONOMY_DIR COUNTS_TSV (taxon records) SIZES_TSV (source k-mers) ROWS_TSV (source depth all distinct) OUTPUT | parse FILE [MATE_FILE] | props INDEX | records INDEX | repeated [-p] FILES\n"
    "environment: SLK_HOST_THREADS (formatting/decoding threads), SLK_INPUT_STREAMS (input files read side by side, default 8),\n"
    "             SLK_PARSE_THREADS (threads parsing one plain input file, default min(8, cores/2)), SLK_GZIP_LEVEL (1..9, default zlib's),\n"
    "             SLK_GZ_THREADS (threads inflating one gzip input file, default min(16, cores / files read side by side); 0: zlib),\n"
    "             SLK_CLASSIFY_THREADS (threads classifying batches, each with its own stream, default 2),\n"
    "             SLK_HOST_TIMING (report where the wall clock of the classify loop went),\n"
    "             SLK_BUILD_BATCH_BASES (bases per batch of `build` and `coverage`, default 2^30), SLK_MASK_BATCH_BASES (bytes of text per piece\n"
    "             of `mask` and letters per staged batch of slk_mask_sequences, default 2^28), SLK_COVERAGE_MAX_PAIRS ((minimizer, source\n"
    "             taxon) pairs `coverage` counts at a time, default: what half of the GPU's free memory holds), SLK_EXPORT_PIECE_BUCKETS (table buckets per exported\n"
    "             piece of `build` and `respace`, default 2^23), SLK_COMPARE_CHUNK (bytes of text `compare` joins at a time, default 2^26)\n";

int main(int argc, char **argv) {
  int i = 1;
  // global Spark option of the reference: `buckets` of the library `build` writes; the other commands accept and ignore it
  while (i < argc && std::string(argv[i]) == "--partitions") {
    if (i + 1 < argc) g_partitions = atoi(argv[i + 1]);
    i += 2;
  }
  if (i >= argc) die("usage: slacken-amd [--partitions N] classify|classify2|build|merge|mask|bracken-build|compare-index|compare|respace|coverage|support|stats|inspect|copy-records|report|parse|props|records ... (--help for the options)");
  std::string cmd = argv[i++];
  if (cmd == "--help" || cmd == "-h" || cmd == "help") { std::cout << HELP; return 0; }
  if (cmd == "--version") { std::cout << slk_version() << "\n"; return 0; }
  static const struct { const char *name; int (*run)(int, char **); } COMMANDS[] = {
      {"classify", cmd_classify}, {"classify2", cmd_classify2}, {"report", cmd_report}, {"parse", cmd_parse}, {"gunzip", cmd_gunzip},
      {"props", cmd_props}, {"records", cmd_records}, {"repeated", cmd_repeated}, {"taxonomy", cmd_taxonomy},
      {"bracken-build", cmd_bracken_build}, {"kmer-distrib", cmd_kmer_distrib}, {"compare-index", cmd_compare_index},
      {"compareIndex", cmd_compare_index}, {"migration-report", cmd_migration_report}, {"stats", cmd_stats}, {"inspect", cmd_inspect},
      {"stats-report", cmd_stats_report}, {"respace", cmd_respace}, {"copy-records", cmd_copy_records}, {"build", cmd_build},
      {"coverage", cmd_coverage}, {"coverage-report", cmd_coverage_report}, {"support", cmd_support}, {"mask", cmd_mask},
      {"compare", cmd_compare}, {"merge", cmd_merge}};
  // (`stats` or `inspect` with nothing behind it is answered below, by the list of what this engine implements, as it was before
  //  they were commands)
  const bool bare = (cmd == "stats" || cmd == "inspect") && i >= argc;
  try {
    for (const auto &c : COMMANDS)
      if (cmd == c.name && !bare) return c.run(argc - i, argv + i);
  } catch (const std::exception &e) {
    die(e.what());
  }
  die("unknown command line `" + cmd + "` (this engine implements `classify`, `classify2`, `build`, `merge`, `mask`, `bracken-build`, `compare-index`, `compare`, `respace`, `coverage`, `support`, `stats -i INDEX` and "
      "`inspect -i INDEX -o OUTPUT`; the reference's other subcommands are out of scope; --help for the options)");
}
