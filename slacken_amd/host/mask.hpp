// mask.hpp -- low-complexity masking on the host: the serial statement of what slacken_amd/csrc/mask.hip computes (symmetric DUST,
// Morgulis et al. 2006, as the reference's scripts/k2/mask_low_complexity.sh applies it with `k2mask -r x`), the walk
// over FASTA text that keeps every byte but the masked letters, and the file protocol of that script (FILE.tmp, rename, FILE.masked).
// No GPU dependency: `mask --host` runs on this alone and the tests compile it into a program of its own.
#pragma once
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <vector>

#include "../../include/slacken_amd.h"

namespace slk_host {

// 0..3 for A C G T/U in either case, 4 for everything else: the letters slk_index_add_sequences takes
inline int mask_code(uint8_t c) {
  switch (c | 0x20) { case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': case 'u': return 3; default: return 4; }
}

inline bool mask_config_ok(const slk_mask_config &c) {   // (after mask_config_defaults)
  return c.window >= 8 && c.window <= 64 && c.threshold >= 1 && c.threshold <= 255;
}
inline slk_mask_config mask_config_defaults(const slk_mask_config *c) {   // window 0, threshold 0: 64, 20
  slk_mask_config r{64, 20, 0};
  if (c) { r = *c; if (!r.window) r.window = 64; if (!r.threshold) r.threshold = 20; }
  return r;
}

// One run of valid letters: marks[p] = 1 for every letter inside a perfect interval.  M(a, b), the best score of any sub-interval of
// [a, b], is kept as the exact pair (S, l - 1) and compared by cross-multiplication (S <= 1891: the products fit 32 bits); starts are
// taken from the right, so that `above` is the row M(a + 1, .) while the row of a is written over it from the left.
inline void mask_run_marks(const uint8_t *run, size_t n, uint32_t window, uint32_t threshold, uint8_t *marks) {
  if (n < 3) return;
  const size_t nt = n - 2;
  std::vector<uint8_t> trip(nt);
  for (size_t i = 0; i < nt; i++) trip[i] = (uint8_t)(mask_code(run[i]) << 4 | mask_code(run[i + 1]) << 2 | mask_code(run[i + 2]));
  struct Score { uint32_t s, d; };
  Score above[64];   // above[d] = M(a + 1, a + 1 + d), d = 0: an interval of one triplet, which counts as (0, 1)
  size_t above_n = 0;
  std::vector<uint8_t> reach(nt, 0);    // letters from a that its longest perfect interval covers
  for (size_t a = nt; a-- > 0;) {
    uint8_t counts[64];
    memset(counts, 0, sizeof(counts));
    counts[trip[a]] = 1;
    uint32_t s = 0;
    Score left{0, 1};
    const size_t steps = std::min<size_t>(nt - 1 - a, window - 3);
    Score row[64];
    row[0] = Score{0, 1};
    for (uint32_t d = 1; d <= steps; d++) {
      const uint8_t v = trip[a + d];
      s += counts[v]++;
      const Score up = d - 1 < above_n ? above[d - 1] : Score{0, 1};
      const Score best = up.s * left.d > left.s * up.d ? up : left;
      const bool on_top = s * best.d >= best.s * d;   // a tie keeps the interval
      if (on_top && 10 * s > threshold * d) reach[a] = (uint8_t)(d + 3);
      left = on_top ? Score{s, d} : best;
      row[d] = left;
    }
    memcpy(above, row, (steps + 1) * sizeof(Score));
    above_n = steps + 1;
  }
  size_t until = 0;
  for (size_t a = 0; a < nt; a++) {
    if (reach[a]) until = std::max(until, a + reach[a]);
    if (a < until) marks[a] = 1;
  }
  for (size_t p = nt; p < n; p++)
    if (p < until) marks[p] = 1;
}

// One sequence, in place: every maximal run of valid letters is masked on its own.  Returns the letters changed.
inline uint64_t mask_sequence_host(uint8_t *seq, size_t n, const slk_mask_config &cfg) {
  uint64_t changed = 0;
  std::vector<uint8_t> marks;
  for (size_t i = 0; i < n;) {
    if (mask_code(seq[i]) > 3) { i++; continue; }
    size_t j = i;
    while (j < n && mask_code(seq[j]) <= 3) j++;
    marks.assign(j - i, 0);
    mask_run_marks(seq + i, j - i, cfg.window, cfg.threshold, marks.data());
    for (size_t p = i; p < j; p++) {
      if (!marks[p - i]) continue;
      const uint8_t c = cfg.replacement ? cfg.replacement : (uint8_t)(seq[p] | 0x20);
      changed += c != seq[p];
      seq[p] = c;
    }
    i = j;
  }
  return changed;
}


// Sequences in the layout of slk_index_add_sequences, in place, shared out over `threads` threads sequence by sequence.
inline uint64_t mask_sequences_host(uint8_t *bases, const uint64_t *offsets, uint64_t n_sequences, const slk_mask_config &cfg, size_t threads) {
  std::atomic<uint64_t> next{0}, changed{0};
  auto work = [&] {
    for (uint64_t i; (i = next.fetch_add(1)) < n_sequences;) changed += mask_sequence_host(bases + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), cfg);
  };
  std::vector<std::thread> th;
  for (size_t t = 1; t < std::min<uint64_t>(std::max<size_t>(threads, 1), n_sequences); t++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  return changed;
}

// ---- FASTA text <-> the sequences / offsets layout --------------------------------------------------------------------------
// fn(i) for every byte text[i] that is a letter of a record, new_record() at every header line: a line that begins with '>' is a
// header up to its '\n'; '\n' and '\r' are line ends and do not end a run; every other byte after the first header is a letter (an
// invalid one, if it is not ACGTU).  Bytes before the first header are no record's.  The text is whole records.
template <class Letter, class Record>
inline void walk_fasta(const uint8_t *text, size_t n, Letter letter, Record new_record) {
  bool in_record = false;
  for (size_t i = 0; i < n;) {
    if (text[i] == '>' && (i == 0 || text[i - 1] == '\n')) {
      in_record = true;
      new_record();
      const void *nl = memchr(text + i, '\n', n - i);
      i = nl ? (size_t)((const uint8_t *)nl - text) + 1 : n;
      continue;
    }
    if (in_record && text[i] != '\n' && text[i] != '\r') letter(i);
    i++;
  }
}

// One piece of a file, whole records: its text as read, and the letters of its records without header lines and line ends --
// sequence i is bases[offsets[i] .. offsets[i+1]); every record is taken, an empty one as an empty sequence.
struct MaskPiece {
  std::vector<uint8_t> text, bases;
  std::vector<uint64_t> offsets;
  bool failed = false;   // the read failed
  void extract() {
    bases.clear();
    offsets.clear();
    walk_fasta(text.data(), text.size(), [&](size_t i) { bases.push_back(text[i]); }, [&] { offsets.push_back(bases.size()); });
    if (offsets.empty()) offsets.push_back(0);   // (no record: nothing to mask)
    else offsets.push_back(bases.size());
  }
  uint64_t n_sequences() const { return offsets.size() - 1; }
  void put_back() {   // the letters, masked, to where they came from: nothing else of the text changes
    size_t j = 0;
    walk_fasta(text.data(), text.size(), [&](size_t i) { text[i] = bases[j++]; }, [] {});
  }
};

// Reads whole records of about `piece_bytes` from f; `carry` holds what was read beyond the last piece (it begins at a header
// line).  A record longer than that is a piece of its own.  An empty text: the file has ended.
inline void read_piece(FILE *f, size_t piece_bytes, std::vector<uint8_t> *carry, MaskPiece *p) {
  p->text.swap(*carry);
  carry->clear();
  p->failed = false;
  size_t searched = p->text.empty() ? 0 : 1;   // (the piece's own header line, at 0, is no cut)
  for (;;) {
    if (p->text.size() >= piece_bytes) {   // cut at the last header line, if there is one beyond the first byte
      size_t cut = 0;
      for (size_t i = p->text.size(); i-- > std::max<size_t>(searched, 1);)
        if (p->text[i] == '>' && p->text[i - 1] == '\n') { cut = i; break; }
      if (cut) {
        carry->assign(p->text.begin() + cut, p->text.end());
        p->text.resize(cut);
        break;
      }
      searched = p->text.size();
    }
    const size_t at = p->text.size(), want = std::max<size_t>(std::min<size_t>(piece_bytes, (size_t)1 << 24), 4096);
    p->text.resize(at + want);
    const size_t got = fread(p->text.data() + at, 1, want, f);
    p->text.resize(at + got);
    if (got == 0) { p->failed = ferror(f) != 0; break; }
  }
  p->extract();
}

struct MaskTotals { uint64_t letters = 0, masked = 0; };

// FILE -> FILE.tmp, renamed over FILE, then FILE.masked is created: scripts/k2/mask_low_complexity.sh.  The text differs from the
// input in the masked letters only.  mask_batch(bases, offsets, n_sequences) masks in place and returns the letters changed; the next
// piece is read while it runs.  On a failure FILE is as it was, FILE.tmp is gone and no FILE.masked appears; `error` says what failed.
template <class MaskBatch>
inline bool mask_file(const std::string &path, size_t piece_bytes, MaskBatch mask_batch, MaskTotals *totals, std::string *error) {
  const std::string tmp = path + ".tmp";
  FILE *in = fopen(path.c_str(), "rb");
  if (!in) { *error = "cannot open " + path + ": " + strerror(errno); return false; }
  FILE *out = fopen(tmp.c_str(), "wb");
  if (!out) { *error = "cannot write " + tmp + ": " + strerror(errno); fclose(in); return false; }
  std::vector<uint8_t> carry;
  MaskPiece piece[2];
  int cur = 0;
  bool ok = true;
  read_piece(in, piece_bytes, &carry, &piece[cur]);
  while (ok && !piece[cur].text.empty()) {
    MaskPiece &p = piece[cur], &q = piece[cur ^ 1];
    if (p.failed) { *error = "cannot read " + path; ok = false; break; }
    std::future<void> reading = std::async(std::launch::async, [&] { read_piece(in, piece_bytes, &carry, &q); });
    totals->letters += p.bases.size();
    totals->masked += mask_batch(p.bases.data(), p.offsets.data(), p.n_sequences());
    p.put_back();
    if (fwrite(p.text.data(), 1, p.text.size(), out) != p.text.size()) { *error = "cannot write " + tmp + ": " + strerror(errno); ok = false; }
    reading.get();
    cur ^= 1;
  }
  if (ok && piece[cur].failed) { *error = "cannot read " + path; ok = false; }
  fclose(in);
  if (fclose(out) != 0 && ok) { *error = "cannot write " + tmp + ": " + strerror(errno); ok = false; }
  if (ok && rename(tmp.c_str(), path.c_str()) != 0) { *error = "cannot rename " + tmp + " over " + path + ": " + strerror(errno); ok = false; }
  if (!ok) { remove(tmp.c_str()); return false; }
  FILE *m = fopen((path + ".masked").c_str(), "wb");
  if (!m) { *error = "cannot create " + path + ".masked: " + strerror(errno); return false; }
  fclose(m);
  return true;
}

}  // namespace slk_host
