// compare.hpp -- `compare`: classifications against a truth mapping, mirroring MappingComparison
// (S/slacken/analysis/MappingComparison.scala) and its command (S/slacken/Slacken.scala:343-366).  Header only, host only (C++17).
// The work has two halves.  The JOIN of the test rows with the reference rows on the read id leaves a few numbers: the joined rows per
// (reference taxon, test taxon), raw ids, and the kept reference rows per raw taxon (CompareCounts).  It is done on the GPU
// (slk_compare_*, csrc/compare.hip) or, with --host, by HostJoin below: the statement the device is compared with.  The METRICS are
// functions of those numbers and the taxonomy (location_report, metrics_row): primary(), the isDefined filter, hitCategory and the
// per-taxon sets are applied to the distinct pairs -- thousands of rows, not millions.  DESIGN.md 22 has the contract and the
// deviations; tests/compare_model.py restates it.
#pragma once
#include <cstring>
#include <filesystem>
#include <map>
#include <memory>
#include <regex>
#include <set>
#include <string_view>
#include <unordered_map>

#include "taxonomy.hpp"

namespace slk_host {

// ---- numbers as Java prints them ------------------------------------------------------------------------------------------------

// Double.toString: the shortest decimal digits that identify the double; plain notation from 1e-3 up to 1e7, "d.dddE<n>" outside.
inline std::string java_double_string(double d) {
  if (std::isnan(d)) return "NaN";
  if (std::isinf(d)) return d > 0 ? "Infinity" : "-Infinity";
  const std::string sign = std::signbit(d) ? "-" : "";
  if (d == 0) return sign + "0.0";
  const double x = std::fabs(d);
  char b[64];
  for (int prec = 1; prec <= 17; prec++) {
    snprintf(b, sizeof b, "%.*e", prec - 1, x);
    if (strtod(b, nullptr) == x) break;
  }
  std::string digits;   // d.dddde[+-]XX -> digits, x = d.ddd * 10^e10
  const char *p = b;
  for (; *p && *p != 'e'; p++) if (*p != '.') digits.push_back(*p);
  const int e10 = atoi(p + 1);
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  if (x >= 1e-3 && x < 1e7) {
    std::string whole, frac;
    if (e10 >= 0) {
      whole = digits.substr(0, std::min(digits.size(), (size_t)e10 + 1));
      whole.append((size_t)e10 + 1 - whole.size(), '0');
      if (digits.size() > (size_t)e10 + 1) frac = digits.substr((size_t)e10 + 1);
    } else {
      whole = "0";
      frac = std::string((size_t)(-e10 - 1), '0') + digits;
    }
    return sign + whole + "." + (frac.empty() ? "0" : frac);
  }
  return sign + digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(e10);
}

// Helpers.formatPerc (S/kmers/package.scala:60): "%.2f%%".format(d * 100), d >= 0 or NaN
inline std::string java_format_perc(double d) {
  const double v = d * 100;
  if (std::isnan(v)) return "NaN%";
  if (std::isinf(v)) return v > 0 ? "Infinity%" : "-Infinity%";
  const std::string s = java_format_6_2f(v);
  return s.substr(s.find_first_not_of(' ')) + "%";
}

// ---- text -------------------------------------------------------------------------------------------------------------------------
// Lines end with \n, \r\n or a lone \r; empty lines are skipped; fields are split at TAB only, quotes mean nothing.

constexpr int COMPARE_BAD_LINE = 1, COMPARE_DUPLICATE_REFERENCE = 2, COMPARE_DUPLICATE_TEST = 3;   // SLK_COMPARE_* of the C ABI
struct CompareTextError {
  uint64_t offset;   // of the line in the whole text given to the joiner (all chunks counted)
  int kind;
};

// f(offset, line, length) for every non-empty line of a chunk.  final = false: a line counts only when its terminator lies inside the
// chunk and is decided (a \r on the last byte is not).  Returns the start of the first undecided line: where the next chunk starts.
template <class F>
inline size_t for_each_line(const char *p, size_t n, bool final, F &&f) {
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && p[j] != '\n' && p[j] != '\r') j++;
    size_t next = j + 1;
    if (j == n || (p[j] == '\r' && j + 1 == n)) {
      if (!final) return i;
      next = n;
    } else if (p[j] == '\r' && p[j + 1] == '\n') {
      next = j + 2;
    }
    if (j > i) f(i, p + i, j - i);
    i = next;
  }
  return n;
}

// where the text goes on behind its first non-empty line (--header); std::string::npos: not decided inside this chunk
inline size_t header_end(const char *p, size_t n, bool final) {
  size_t end = std::string::npos;
  bool seen = false;
  for_each_line(p, n, final, [&](size_t at, const char *, size_t len) {
    if (seen) return;
    seen = true;
    end = at + len;
  });
  if (!seen) return final ? n : std::string::npos;
  // the terminator of that line: decided, because the line counted
  if (end < n && p[end] == '\r') end += (end + 1 < n && p[end + 1] == '\n') ? 2 : 1;
  else if (end < n) end += 1;
  return end;
}

// The columns id_col and taxon_col (counted from 0) of a line; false: too few columns, an empty field, or a taxon that Java's
// Integer.parseInt refuses ("+7" is 7) or that is negative.
inline bool compare_fields(const char *line, size_t len, int id_col, int taxon_col, std::string_view &id, int32_t &taxon) {
  const int last = std::max(id_col, taxon_col);
  std::string_view tx;
  bool have_id = false, have_tx = false;
  int col = 0;
  size_t fs = 0;
  for (size_t q = 0;; q++) {
    if (q == len || line[q] == '\t') {
      if (col == id_col) { id = std::string_view(line + fs, q - fs); have_id = true; }
      if (col == taxon_col) { tx = std::string_view(line + fs, q - fs); have_tx = true; }
      if (col == last) break;
      if (q == len) return false;
      col++;
      fs = q + 1;
    }
  }
  if (!have_id || !have_tx || id.empty() || tx.empty()) return false;
  size_t p = 0;
  bool neg = false;
  if (tx[0] == '+' || tx[0] == '-') { neg = tx[0] == '-'; p = 1; }
  if (p == tx.size()) return false;
  uint64_t v = 0;
  for (; p < tx.size(); p++) {
    if (tx[p] < '0' || tx[p] > '9') return false;
    v = v * 10 + (uint64_t)(tx[p] - '0');
    if (v > 2147483648ULL) return false;
  }
  if (neg ? v != 0 : v > 2147483647ULL) return false;
  taxon = (int32_t)v;
  return true;
}

// ---- the join ---------------------------------------------------------------------------------------------------------------------

struct CompareCounts {   // what a join leaves; taxa are RAW, as the texts have them
  struct Pair { Taxon ref, test; uint64_t rows; };
  std::vector<Pair> pairs;                              // joined rows of the current test, ascending by (ref, test)
  std::vector<std::pair<Taxon, uint64_t>> ref_taxa;     // kept reference rows per taxon, ascending
  uint64_t reference_rows = 0, dropped_second = 0, kept_ids = 0, test_rows = 0, joined_rows = 0;
};

// One resident reference mapping and the tests streamed against it.  Text is given in chunks; the calls return what they consumed.
// A bad line or a duplicate id throws CompareTextError.
struct CompareJoiner {
  virtual ~CompareJoiner() = default;
  virtual size_t add_reference(const char *p, size_t n, int id_col, int taxon_col, bool final) = 0;   // columns counted from 1
  virtual void begin_test() = 0;
  virtual size_t add_test(const char *p, size_t n, bool final) = 0;
  virtual CompareCounts counts() = 0;
};

// --host: the join by a host hash map keyed by the normalised id (readCustomFormat :265-274, readKrakenFormat :259-263, the joins
// :157-159 and :216-217)
class HostJoin : public CompareJoiner {
  struct Row { Taxon taxon; bool matched; };
  std::unordered_map<std::string, Row> ref_;
  std::map<std::pair<Taxon, Taxon>, uint64_t> pairs_;
  std::map<Taxon, uint64_t> ref_taxa_;
  CompareCounts totals_;
  uint64_t ref_base_ = 0, test_base_ = 0;
  std::string key_;

 public:
  size_t add_reference(const char *p, size_t n, int id_col, int taxon_col, bool final) override {
    const size_t consumed = for_each_line(p, n, final, [&](size_t at, const char *line, size_t len) {
      std::string_view id;
      int32_t taxon = 0;
      if (!compare_fields(line, len, id_col - 1, taxon_col - 1, id, taxon)) throw CompareTextError{ref_base_ + at, COMPARE_BAD_LINE};
      totals_.reference_rows++;
      if (id.find("/2") != std::string_view::npos) { totals_.dropped_second++; return; }   // the second mate's row (:269)
      key_.clear();
      for (size_t q = 0; q < id.size();) {   // replaceAll("/1", "") (:271): one pass from the left
        if (id[q] == '/' && q + 1 < id.size() && id[q + 1] == '1') { q += 2; continue; }
        key_.push_back(id[q++]);
      }
      if (!ref_.emplace(key_, Row{taxon, false}).second) throw CompareTextError{ref_base_ + at, COMPARE_DUPLICATE_REFERENCE};
      totals_.kept_ids++;
      ref_taxa_[taxon]++;
    });
    ref_base_ += consumed;
    return consumed;
  }
  void begin_test() override {
    pairs_.clear();
    for (auto &kv : ref_) kv.second.matched = false;
    totals_.test_rows = totals_.joined_rows = 0;
    test_base_ = 0;
  }
  size_t add_test(const char *p, size_t n, bool final) override {
    const size_t consumed = for_each_line(p, n, final, [&](size_t at, const char *line, size_t len) {
      std::string_view id;
      int32_t taxon = 0;
      if (!compare_fields(line, len, 1, 2, id, taxon)) throw CompareTextError{test_base_ + at, COMPARE_BAD_LINE};
      totals_.test_rows++;
      key_.assign(id.data(), id.size());   // the id as it is
      auto it = ref_.find(key_);
      if (it == ref_.end()) return;
      if (it->second.matched) throw CompareTextError{test_base_ + at, COMPARE_DUPLICATE_TEST};
      it->second.matched = true;
      totals_.joined_rows++;
      pairs_[{it->second.taxon, taxon}]++;
    });
    test_base_ += consumed;
    return consumed;
  }
  CompareCounts counts() override {
    CompareCounts c = totals_;
    for (auto &kv : pairs_) c.pairs.push_back({kv.first.first, kv.first.second, kv.second});
    c.ref_taxa.assign(ref_taxa_.begin(), ref_taxa_.end());
    return c;
  }
};

// One file's bytes to add(p, n, final) -> consumed, in chunks of about chunk_bytes with the unconsumed tail carried over; a chunk
// that holds no whole line grows.  read(dst, cap) -> bytes, 0 at the end.  skip_header: the first non-empty line is not given.
// *skipped (if given): the bytes not given in front, the header line with what precedes it -- set before the first add.
template <class Read, class Add>
inline void feed_text(Read &&read, size_t chunk_bytes, bool skip_header, Add &&add, uint64_t *skipped = nullptr) {
  std::vector<char> buf(std::max<size_t>(chunk_bytes, 16));
  size_t have = 0;
  bool eof = false;
  if (skipped) *skipped = 0;
  for (;;) {
    while (!eof && have < buf.size()) {
      const size_t got = read(buf.data() + have, buf.size() - have);
      if (got == 0) eof = true;
      have += got;
    }
    size_t used = 0;
    if (skip_header) {
      const size_t h = header_end(buf.data(), have, eof);
      if (h != std::string::npos) {
        used = h;
        skip_header = false;
        if (skipped) *skipped = h;
      }
    }
    if (!skip_header && have > used) used += add(buf.data() + used, have - used, eof);
    if (eof) break;
    if (used == 0) buf.resize(buf.size() * 2);   // no whole line yet
    memmove(buf.data(), buf.data() + used, have - used);
    have -= used;
  }
}

// the number, counted from 1, of the line that starts at byte `offset` of a file, and its text
template <class Read>
inline uint64_t locate_line(Read &&read, uint64_t offset, std::string &text) {
  std::vector<char> buf((size_t)1 << 20);
  uint64_t line = 1, at = 0;
  char prev = 0;
  text.clear();
  while (size_t got = read(buf.data(), buf.size())) {
    for (size_t i = 0; i < got; i++, at++) {
      const char c = buf[i];
      if (at >= offset) {
        if (c == '\n' || c == '\r') return line;
        text.push_back(c);
      } else if (c == '\r' || (c == '\n' && prev != '\r')) {
        line++;
      }
      prev = c;
    }
  }
  return line;
}

// ---- the metrics ------------------------------------------------------------------------------------------------------------------

constexpr long COMPARE_MIN_COUNT_TAXON = 10;   // Slacken.scala:358
struct CompareRank { const char *name; int depth; };
inline const CompareRank *compare_ranks() {
  static const CompareRank r[2] = {{"Genus", 7}, {"Species", 8}};   // Taxonomy.scala:47-48, in the order of allMetrics :140-143
  return r;
}

// hitCategory :313-331 with level = Some(rank): the class (0 TruePos, 1 VaguePos, 2 FalseNeg, 3 FalsePos) and the hit index
struct HitCategory { int cls, index; };
inline HitCategory hit_category(const Taxonomy &tax, Taxon ref, Taxon test, int rank_depth) {
  if (test == NONE) return {2, 9};
  const Taxon anc = tax.standardAncestorAtLevel(ref, rank_depth);
  const Taxon ref_ancestor = anc != NONE ? anc : ref;
  if (ref == test) return {0, 0};
  if (ref_ancestor != ROOT && tax.hasAncestor(test, ref_ancestor)) return {0, 0};
  if (ref_ancestor == ROOT || tax.hasAncestor(ref, test)) return {1, tax.standardStepsToAncestor(ref, test)};
  if (test == ROOT) return {1, tax.standardStepsToAncestor(ref, test)};
  return {3, 9};
}

struct PerTaxonMetrics { long classified = 0, ref = 0; double precision = 0, recall = 0; };                                  // :32-34
struct PerReadMetrics { long classified = 0, total = 0, tp = 0, fp = 0, vp = 0, fn = 0; double ppv = 0, sensitivity = 0, index = 0; };   // :41-44
struct LocationMetrics {
  std::string title;
  PerTaxonMetrics taxon[2];   // Genus, Species
  PerReadMetrics read[2];
};

inline double java_div(double a, double b) { return b != 0 ? a / b : a == 0 ? std::nan("") : INFINITY; }   // Double division by zero

inline std::string compare_title(const std::string &data_file, bool multi) {   // allMetrics :151-152
  std::vector<std::string> spl;
  size_t a = 0;
  for (;;) {
    const size_t b = data_file.find('/', a);
    spl.push_back(data_file.substr(a, b == std::string::npos ? b : b - a));
    if (b == std::string::npos) break;
    a = b + 1;
  }
  while (!spl.empty() && spl.back().empty()) spl.pop_back();   // (Java's split drops trailing empty strings)
  std::string t;
  const size_t keep = multi ? 4 : 1;   // takeRight(4) | last
  const size_t from = spl.size() > keep ? spl.size() - keep : 0;
  for (size_t i = from; i < spl.size(); i++) {
    if (i > from) t += "/";
    t += spl[i];
  }
  return t;
}

// allMetrics :134-168 from what the join left: the text the reference prints for one location, and its metrics.  A taxon outside
// the taxonomy's range ends the run (std::runtime_error).
inline std::string location_report(const Taxonomy &tax, const CompareCounts &c, const std::string &data_file, bool multi, LocationMetrics &out) {
  auto check = [&](Taxon t) {
    if (t < 0 || t >= tax.size()) throw std::runtime_error("taxon " + std::to_string(t) + " lies outside the taxonomy (ids 0.." + std::to_string(tax.size() - 1) + ")");
  };
  std::ostringstream o;
  // readReferenceData :119-132: primary(), then the rows of taxa the taxonomy does not define are dropped
  std::map<Taxon, uint64_t> ref_by_taxon;
  std::set<Taxon> unknown;
  uint64_t ref_size = 0;
  for (auto &kv : c.ref_taxa) {
    check(kv.first);
    const Taxon t = tax.primary[kv.first];
    if (tax.isDefined(t)) { ref_by_taxon[t] += kv.second; ref_size += kv.second; }
    else unknown.insert(t);
  }
  for (Taxon t : unknown) o << "Reference contains unknown taxon, not known to taxonomy: " << t << ". It will be filtered out.\n";
  o << "Filtered reference size: " << ref_size << "\n";
  o << "--------" << data_file << "--------\n";
  std::map<std::pair<Taxon, Taxon>, uint64_t> joined;   // (refTaxon, testTaxon) after primary(), undefined reference taxa gone
  for (auto &p : c.pairs) {
    check(p.ref);
    check(p.test);
    const Taxon r = tax.primary[p.ref], t = tax.primary[p.test];
    if (tax.isDefined(r)) joined[{r, t}] += p.rows;
  }
  out.title = compare_title(data_file, multi);
  for (int ri = 0; ri < 2; ri++) {
    const CompareRank rank = compare_ranks()[ri];
    // perTaxonComparison :170-209
    std::set<Taxon> ref_taxa, cmp_taxa;
    for (auto &kv : ref_by_taxon) {
      const Taxon a = tax.standardAncestorAtLevel(kv.first, rank.depth);
      if (a != NONE) ref_taxa.insert(a);
    }
    std::map<Taxon, uint64_t> cmp_counts;
    for (auto &kv : joined) {
      const Taxon a = tax.standardAncestorAtLevel(kv.first.second, rank.depth);
      if (a != NONE) cmp_counts[a] += kv.second;
    }
    for (auto &kv : cmp_counts) if (kv.second >= (uint64_t)COMPARE_MIN_COUNT_TAXON) cmp_taxa.insert(kv.first);
    const std::vector<uint8_t> with_anc = tax.taxaWithAncestors(std::vector<Taxon>(ref_taxa.begin(), ref_taxa.end()));
    auto vague = [&](Taxon t) { return with_anc[t] && !ref_taxa.count(t); };
    long tp = 0, fp = 0, vp = 0, fn = 0, cmp_not_vague = 0;
    for (Taxon t : cmp_taxa) {
      if (ref_taxa.count(t)) tp++;
      else if (vague(t)) vp++;
      else fp++;
      if (!vague(t)) cmp_not_vague++;
    }
    for (Taxon t : ref_taxa) if (!cmp_taxa.count(t)) fn++;
    PerTaxonMetrics &pt = out.taxon[ri];
    pt.classified = (long)cmp_taxa.size();
    pt.ref = (long)ref_taxa.size();
    pt.precision = java_div((double)tp, (double)cmp_not_vague);
    pt.recall = java_div((double)tp, (double)ref_taxa.size());
    o << "*** Per taxon comparison (minimum " << COMPARE_MIN_COUNT_TAXON << ") at level Some(" << rank.name << ")\n";
    o << "Total ref taxa " << ref_taxa.size() << ", total classified taxa " << cmp_taxa.size() << "\n";
    o << "TP " << tp << ", VP " << vp << " FP " << fp << ", FN " << fn << "}\n";
    o << "Precision " << java_format_perc(pt.precision) << " recall " << java_format_perc(pt.recall) << "\n\n";
    // perReadComparison :211-257
    PerReadMetrics &pr = out.read[ri];
    pr = PerReadMetrics();
    long long index_sum = 0;
    for (auto &kv : joined) {
      const long n = (long)kv.second;
      pr.total += n;
      if (kv.first.second != NONE) pr.classified += n;
      const HitCategory hc = hit_category(tax, kv.first.first, kv.first.second, rank.depth);
      (hc.cls == 0 ? pr.tp : hc.cls == 1 ? pr.vp : hc.cls == 2 ? pr.fn : pr.fp) += n;
      index_sum += (long long)hc.index * n;
    }
    pr.sensitivity = java_div((double)pr.tp, (double)pr.total);
    pr.ppv = pr.tp + pr.fp > 0 ? (double)pr.tp / (double)(pr.tp + pr.fp) : 0.0;
    pr.index = pr.total ? (double)index_sum / (double)pr.total : std::nan("");
    o << "Total reads " << pr.total << "\n";
    o << "Classified " << pr.classified << " " << java_format_perc(java_div((double)pr.classified, (double)pr.total)) << "\n";
    o << "*** Per-read comparison at level Some(" << rank.name << ")\n";
    o << "PPV " << java_format_perc(pr.ppv) << " Sensitivity " << java_format_perc(pr.sensitivity) << "\n\n";
  }
  return o.str();
}

inline const char *compare_metrics_header() {   // Metrics.header :68
  return "title\tfamily\tgroup\tsample\tlibrary\tk\tm\tfrequency\tfl\ts\tc\trank\ttaxon_classified\ttaxon_total\ttaxon_precision\ttaxon_recall\t"
         "read_classified\tread_total\tread_tp\tread_fp\tread_vp\tread_fn\tread_ppv\tread_sensitivity\tread_index";
}

// Metrics.toTSVString :55-64: the row, or -- the title does not have the expected shape -- false and the line printed instead
inline bool metrics_row(const LocationMetrics &m, int ri, std::string &row) {
  static const std::regex pattern(R"((.*)/(.*)/(.+)_(\d+)_(\d+)_s(\d+)_c([\d.]+)_classified/sample=(.*))");   // :53
  std::smatch g;
  if (!std::regex_match(m.title, g, pattern)) {
    row = "Couldn't extract variables from filename: " + m.title + ". Omitting from output.";
    return false;
  }
  const PerTaxonMetrics &t = m.taxon[ri];
  const PerReadMetrics &r = m.read[ri];
  std::ostringstream o;
  o << m.title << '\t' << g[1] << '\t' << g[2] << '\t' << g[8] << '\t' << g[3] << '\t' << g[4] << '\t' << g[5] << "\t0\t0\t" << g[6] << '\t' << g[7] << '\t'
    << compare_ranks()[ri].name << '\t' << t.classified << '\t' << t.ref << '\t' << java_double_string(t.precision) << '\t'
    << java_double_string(t.recall) << '\t' << r.classified << '\t' << r.total << '\t' << r.tp << '\t' << r.fp << '\t' << r.vp << '\t' << r.fn
    << '\t' << java_double_string(r.ppv) << '\t' << java_double_string(r.sensitivity) << '\t' << java_double_string(r.index);
  row = o.str();
  return true;
}

// ---- the locations ----------------------------------------------------------------------------------------------------------------

// a test location's files: the file itself, or a directory's files whose names begin with neither '_' nor '.', by name
inline std::vector<std::string> compare_location_files(const std::string &location) {
  namespace fs = std::filesystem;
  std::vector<std::string> files;
  if (!fs::is_directory(location)) return {location};
  for (auto &e : fs::directory_iterator(location)) {
    const std::string name = e.path().filename().string();
    if (e.is_regular_file() && !name.empty() && name[0] != '_' && name[0] != '.') files.push_back(location + "/" + name);
  }
  std::sort(files.begin(), files.end());
  return files;
}

// processDirectories :90-103: every subdirectory sample=<id> of every dir, by name, with its reference mapping
inline std::vector<std::pair<std::string, std::string>> compare_multi_locations(const std::vector<std::string> &dirs, const std::string &reference_prefix) {
  namespace fs = std::filesystem;
  std::vector<std::pair<std::string, std::string>> out;
  for (auto &d : dirs) {
    std::vector<std::string> subs;
    for (auto &e : fs::directory_iterator(d))
      if (e.is_directory()) subs.push_back(e.path().filename().string());
    std::sort(subs.begin(), subs.end());
    for (auto &s : subs) {
      size_t use = std::string::npos;   // ".*sample=(.+)".r.findFirstMatchIn: the greedy .* takes the last "sample=" that has something behind it
      for (size_t q = s.find("sample="); q != std::string::npos; q = s.find("sample=", q + 1))
        if (q + 7 < s.size()) use = q;
      if (use == std::string::npos) continue;
      out.emplace_back(d + "/" + s, reference_prefix + "/sample" + s.substr(use + 7) + "/reads_mapping.tsv");
    }
  }
  return out;
}

}  // namespace slk_host
