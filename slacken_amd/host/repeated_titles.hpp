// repeated_titles.hpp -- titles that occur more than once.
// The reference regroups the hits of ALL fragments by title (groupBy("seqTitle") + collect_list, Classifier.scala:92; the
// same in SQLClassifier :281-290) and sorts each group by ordinal (:136, a stable sort): fragments that share a title are
// ONE read -- one row, one classification of the merged hit list.  Its paired reader is an inner join on the header
// (InputReader.scala:104-119), so a header that repeats inside a file of a pair multiplies before that grouping.
// The first pass streams the input once and treats every fragment on its own -- exact for every title that occurs once.
// The titles whose hash was seen twice (OutputSink, FragmentSource) are settled here: their records are read again, joined
// as the reference joins them, classified with hit lists, merged per title, classified again from the merged list
// (slk_classify_hits), and their rows and counts of the first pass are replaced.  The order of equal ordinals in a merged
// list is not defined by the reference (collect_list after a shuffle); here it is input order.
#pragma once
#include <unordered_map>

#include "device_index.hpp"

namespace slk_host {

struct RepeatFragment { std::string title, seq, mate; };
struct RepeatResult {
  std::vector<slk_hit> hits;
  std::vector<uint8_t> distinct;
  std::vector<int32_t> taxon;        // per threshold
  std::vector<uint8_t> classified;   // per threshold
};

inline std::vector<RepeatResult> classify_fragments(DeviceIndex &dev, const std::vector<RepeatFragment> &frags, const std::vector<size_t> &pick,
                                                    bool paired, int min_hits, const std::vector<double> &thresholds, bool want_distinct) {
  const int C = (int)thresholds.size();
  std::vector<RepeatResult> out(pick.size());
  size_t i0 = 0;
  while (i0 < pick.size()) {
    FragmentBatch fb;
    fb.paired = paired;
    size_t i1 = i0;
    while (i1 < pick.size() && i1 - i0 < ((size_t)1 << 16) && fb.bases.size() + fb.mate_bases.size() < ((size_t)256 << 20)) {
      const RepeatFragment &f = frags[pick[i1]];
      std::string_view m(f.mate);
      fb.add(f.title, f.seq, paired ? &m : nullptr);
      i1++;
    }
    const size_t n = i1 - i0, cap = fb.bases.size() + fb.mate_bases.size() + n + 1;
    std::vector<int32_t> taxon((size_t)C * n), nd(n), tk(n);
    std::vector<uint8_t> cls((size_t)C * n);
    std::vector<uint64_t> hit_offs(n + 1), span_offs(n + 1);
    std::vector<slk_hit> hits(cap);
    std::vector<slk_span> spans(want_distinct ? cap : 0);
    const uint8_t *mb = paired ? fb.mate_bases.data() : nullptr;
    const uint64_t *mo = paired ? fb.mate_offs.data() : nullptr;
    dev.classify_one(fb.bases.data(), fb.offs.data(), mb, mo, n, min_hits, thresholds.data(), C, taxon.data(), cls.data(), nd.data(), tk.data(),
                     hit_offs.data(), hits.data(), cap);
    if (want_distinct) SLK_CALL(slk_spans_batch(dev.ix, dev.st, fb.bases.data(), fb.offs.data(), mb, mo, n, span_offs.data(), spans.data(), cap));
    for (size_t i = 0; i < n; i++) {
      RepeatResult &r = out[i0 + i];
      r.hits.assign(hits.begin() + hit_offs[i], hits.begin() + hit_offs[i + 1]);
      if (want_distinct) {
        if (span_offs[i + 1] - span_offs[i] != hit_offs[i + 1] - hit_offs[i]) die("internal: span and hit lists differ in length");
        for (size_t j = span_offs[i]; j < span_offs[i + 1]; j++) r.distinct.push_back(spans[j].distinct);
      }
      for (int c = 0; c < C; c++) { r.taxon.push_back(taxon[(size_t)c * n + i]); r.classified.push_back(cls[(size_t)c * n + i]); }
    }
    i0 = i1;
  }
  return out;
}

// What the regrouping yields: per title that occurs more than once, the merged hit list and its classification per threshold
struct Regrouped {
  std::vector<std::string> titles;
  std::vector<uint64_t> moffs{0};
  std::vector<slk_hit> mhits;
  std::vector<uint8_t> mdistinct;  // beside mhits
  std::vector<int32_t> mtaxon;     // [C][titles]
  std::vector<uint8_t> mcls;
};

template <class Fn> void for_each_fragment_batch(FragmentSource &src, size_t max_fragments, size_t max_bases, Fn fn) {
  for (;;) {
    FragmentBatchPtr bp;   // (a fresh one: fill appends to what it is given)
    if (!src.fill(bp, max_fragments, max_bases)) return;
    fn(*bp);
  }
}

// The records of a file whose header, less the suffix, is among the titles of D (hashes of the titles seen more than once)
template <class Add> void for_each_repeated_record(const std::string &file, const char *suffix, const FlatHashSet<0> &D, Add add) {
  std::string_view h, s;
  AsyncRecordStream rs(file);
  while (rs.next(h, s)) {
    h = remove_suffix(h, suffix);
    if (D.contains(title_hash(h))) add(h, s);
  }
}

// PairedInputReader.getFragments: every record of file 1 with every record of file 2 of the same header.  Three readers at
// once -- file 1, file 2, and the pairing walk of the first pass (whose fragments, `first`, are what the merged rows replace) --,
// each with its own stream: one pass of wall time over the pair, not three one after the other.
inline void read_repeated_paired(const std::string &file1, const std::string &file2, const FlatHashSet<0> &D,
                                 std::vector<RepeatFragment> &joined, std::vector<RepeatFragment> &first) {
  std::vector<std::string> order;
  std::unordered_map<std::string, std::pair<std::vector<std::string>, std::vector<std::string>>> lists;
  std::unordered_map<std::string, std::vector<std::string>> second;
  std::exception_ptr err0, err1, err2;
  std::thread t1([&] {
    try {
      for_each_repeated_record(file1, "/1", D, [&](std::string_view h1, std::string_view s1) {
        auto it = lists.try_emplace(std::string(h1)).first;
        if (it->second.first.empty()) order.push_back(it->first);
        it->second.first.emplace_back(s1);
      });
    } catch (...) { err1 = std::current_exception(); }
  });
  std::thread t2([&] {
    try {
      for_each_repeated_record(file2, "/2", D, [&](std::string_view h2, std::string_view s2) { second[std::string(h2)].emplace_back(s2); });
    } catch (...) { err2 = std::current_exception(); }
  });
  try {
    FragmentSource src({file1, file2}, true);
    for_each_fragment_batch(src, (size_t)1 << 17, (size_t)512 << 20, [&](const FragmentBatch &b) {
      for (size_t i = 0; i < b.size(); i++)
        if (D.contains(title_hash(b.title(i)))) first.push_back({std::string(b.title(i)), std::string(b.seq(i)), std::string(b.mate(i))});
    });
  } catch (...) { err0 = std::current_exception(); }
  t1.join();
  t2.join();
  for (std::exception_ptr e : {err0, err1, err2}) if (e) std::rethrow_exception(e);
  for (auto &kv : second) {   // (a header of file 2 alone joins nothing)
    auto it = lists.find(kv.first);
    if (it != lists.end()) it->second.second = std::move(kv.second);
  }
  for (const std::string &title : order) {
    auto &l = lists[title];
    for (const std::string &s1 : l.first) for (const std::string &s2 : l.second) joined.push_back({title, s1, s2});
  }
}

// titles (compared as strings) with more than one fragment, in the order of their first fragment, and the fragments of all of them
struct TitleGroups {
  std::unordered_map<std::string_view, std::vector<size_t>> groups;   // every title's fragments (indices into joined)
  std::vector<std::string_view> merged_titles;
  std::vector<size_t> pick;
  bool repeats(const std::string &title) const { auto it = groups.find(title); return it != groups.end() && it->second.size() >= 2; }
};
inline TitleGroups group_by_title(const std::vector<RepeatFragment> &joined) {
  TitleGroups tg;
  std::vector<std::string_view> group_order;
  for (size_t i = 0; i < joined.size(); i++) {
    auto &g = tg.groups[joined[i].title];
    if (g.empty()) group_order.push_back(joined[i].title);
    g.push_back(i);
  }
  for (std::string_view title : group_order) {
    const auto &g = tg.groups[title];
    if (g.size() < 2) continue;   // (a hash collision, or a header that repeats on one side of a pair without a partner)
    tg.merged_titles.push_back(title);
    tg.pick.insert(tg.pick.end(), g.begin(), g.end());
  }
  return tg;
}

// merged hit lists: concatenation in input order, stable sort by ordinal (Classifier.scala:136); res follows tg.pick
inline void merge_hit_lists(const TitleGroups &tg, const std::vector<RepeatResult> &res, Regrouped &out) {
  size_t at = 0;
  struct Ref { uint32_t ordinal; uint32_t member; };
  std::vector<Ref> refs;
  for (std::string_view title : tg.merged_titles) {
    const size_t gn = tg.groups.at(title).size();
    refs.clear();
    for (size_t m = 0; m < gn; m++)
      for (size_t j = 0; j < res[at + m].hits.size(); j++) refs.push_back({(uint32_t)j, (uint32_t)m});
    std::stable_sort(refs.begin(), refs.end(), [](const Ref &a, const Ref &b) { return a.ordinal < b.ordinal; });
    for (const Ref &r : refs) {
      out.mhits.push_back(res[at + r.member].hits[r.ordinal]);
      out.mdistinct.push_back(res[at + r.member].distinct[r.ordinal]);
    }
    out.moffs.push_back(out.mhits.size());
    out.titles.emplace_back(title);
    at += gn;
  }
}

// the merged lists classified (bounded calls: a merged list per title, a few million hits per call)
inline void classify_merged_lists(DeviceIndex &dev, int min_hits, const std::vector<double> &thresholds, Regrouped &out) {
  const int C = (int)thresholds.size();
  const size_t R = out.titles.size();
  out.mtaxon.resize((size_t)C * R);
  out.mcls.resize((size_t)C * R);
  for (size_t r0 = 0; r0 < R;) {
    size_t r1 = r0 + 1;
    while (r1 < R && r1 - r0 < ((size_t)1 << 18) && out.moffs[r1 + 1] - out.moffs[r0] < ((size_t)1 << 23)) r1++;
    const size_t n = r1 - r0;
    std::vector<int32_t> tx((size_t)C * n);
    std::vector<uint8_t> cl((size_t)C * n);
    SLK_CALL(slk_classify_hits(dev.ix, dev.st, n, out.moffs.data() + r0, out.mhits.data(), out.mdistinct.data(), min_hits, thresholds.data(), C,
                               tx.data(), cl.data(), nullptr, nullptr));
    for (int c = 0; c < C; c++)
      for (size_t i = 0; i < n; i++) { out.mtaxon[(size_t)c * R + r0 + i] = tx[(size_t)c * n + i]; out.mcls[(size_t)c * R + r0 + i] = cl[(size_t)c * n + i]; }
    r0 = r1;
  }
}

// D: hashes of the titles seen more than once.  uncount(title, result) is called for every fragment the FIRST pass made of such a
// title (its row and its count are what the merged row replaces).
template <class Uncount>
Regrouped regroup_repeated_titles(DeviceIndex &dev, const std::vector<std::string> &files, bool is_paired, int min_hits,
                                  const std::vector<double> &thresholds, const FlatHashSet<0> &D, Uncount uncount) {
  Regrouped out;
  std::vector<RepeatFragment> joined;   // the fragments of the reference's reader for these titles
  std::vector<RepeatFragment> first;    // paired: the fragments the first pass made of them (its rows are what gets replaced)
  if (is_paired) for (size_t u = 0; u + 2 <= files.size(); u += 2) read_repeated_paired(files[u], files[u + 1], D, joined, first);
  else for (const std::string &file : files)
    for_each_repeated_record(file, "", D, [&](std::string_view h, std::string_view sq) { joined.push_back({std::string(h), std::string(sq), std::string()}); });
  const TitleGroups tg = group_by_title(joined);
  if (tg.merged_titles.empty()) return out;
  std::cerr << tg.merged_titles.size() << " read titles occur more than once (" << tg.pick.size() << " fragments): their hits are regrouped by title" << std::endl;
  const std::vector<RepeatResult> res = classify_fragments(dev, joined, tg.pick, is_paired, min_hits, thresholds, true);
  // what the first pass counted (and wrote) for these titles
  if (!is_paired) {
    for (size_t i = 0; i < tg.pick.size(); i++) uncount(joined[tg.pick[i]].title, res[i]);
  } else {
    std::vector<size_t> pick1;
    for (size_t i = 0; i < first.size(); i++) if (tg.repeats(first[i].title)) pick1.push_back(i);
    const std::vector<RepeatResult> res1 = classify_fragments(dev, first, pick1, true, min_hits, thresholds, false);
    for (size_t i = 0; i < pick1.size(); i++) uncount(first[pick1[i]].title, res1[i]);
  }
  merge_hit_lists(tg, res, out);
  classify_merged_lists(dev, min_hits, thresholds, out);
  return out;
}

}  // namespace slk_host
