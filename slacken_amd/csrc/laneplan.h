// laneplan.h -- the host's plan of a batch as plain arithmetic: which passes of the lane path run and where their limits lie
// (plan_lane), how the piece route's scratch is carved (piece_layout), the staged scan's block and ring (plan_scan), whether a sharded step's lookups ride in its scan
// (shard_side_per_tile).  No HIP header: tests/test_laneplan_cpu.py compiles it alone -- a wrong bound here is a device buffer too small.
#pragma once
#include "layouts.h"

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace slk {

// The routing of a batch on the hot path, one lane per fragment (window of at most 32 m-mers, taxon ids of at most 22 bits:
// lane_path_ok).  What that kernel does not take -- fragments over 1000 bases, taxon maps that overflow -- it appends to the hand-on
// list of the kernel that does (engine.h: FusedArgs.hand_*): four length classes for its own long variant (1001 .. 4999 bases), the
// lane-per-segment kernel (unpaired, w = 5, the fragments that are long for their batch), the wave-per-fragment kernel (the rest, and
// what the long variant hands on in turn).  Everything here follows from the batch's numbers and the switches of PlanSwitches.
struct LanePlan {
  bool lane = false;                             // the lane path runs at all (else: the wave-per-fragment kernel alone)
  bool route_first = false, seg_on = false;      // a routing kernel stands for the first pass; the lane-per-segment kernel takes its share
  uint32_t long_max = 0, long_bound[3] = {0, 0, 0};   // the long variant's limit (0: no such pass) and the borders of its classes
  uint32_t seg_min_len = 0, wave_min = 0, wave_ratio_q10 = 0;
  uint64_t long_cap = 0;      // entries of a list of fragments over 1000 bases
  size_t hand_bytes = 0;      // the hand-on buffer: header and lists
  // the piece route (engine.h: PieceArgs): on when piece_min_len != 0; then seg_min_len is at most piece_min_len, so that the
  // routing hands every fragment the cut may take to the segment pass's list
  uint32_t piece_min_len = 0, piece_windows = 0;
  uint64_t piece_frags = 0, piece_units = 0, piece_map = 0;   // entries the batch can need at most
  bool piece_hits = false;    // the route writes hit lists (slk_stream_set_split_hits): a side array of PieceHitRecords, the move kernel
};

// The SLK_* switches the plan depends on, as values, each under its name in lower case (where unset means something: an int is
// -1, an Opt not set) -- read per call, so that tests can move them.  The two A/B switches among them say which implementation runs
// as a batch's only one: SLK_FORCE_WAVE (force_wave) the wave-per-fragment kernel instead of the lane path, SLK_FORCE_V1 (force_v1)
// the staged kernels instead of either (classify.hip: use_fused).  A classify call reads them once (run_classify) and carries them.
struct PlanSwitches {
  struct Opt { bool set = false; long long v = 0; };
  bool force_wave = false, force_v1 = false, seg_hits = false;
  long long_max = 4999, piece_windows = (long)PIECE_DEFAULT_WINDOWS;   // (SLK_LANE_LONG_MAX)
  int route_first = -1, piece_hits = -1;
  Opt seg_min_len, piece_min_len;
};
inline PlanSwitches read_plan_switches() {
  const auto tri = [](const char *name) { const char *e = getenv(name); return e ? (e[0] == '1' ? 1 : 0) : -1; };
  PlanSwitches s;
  s.force_wave = env_on("SLK_FORCE_WAVE"); s.force_v1 = env_on("SLK_FORCE_V1"); s.seg_hits = env_on("SLK_SEG_HITS");
  s.long_max = env_long("SLK_LANE_LONG_MAX", s.long_max); s.piece_windows = env_long("SLK_PIECE_WINDOWS", s.piece_windows);
  s.route_first = tri("SLK_ROUTE_FIRST"); s.piece_hits = tri("SLK_PIECE_HITS");
  if (const char *e = getenv("SLK_SEG_MIN_LEN")) s.seg_min_len = {true, atol(e)};
  if (const char *e = getenv("SLK_PIECE_MIN_LEN")) s.piece_min_len = {true, atoll(e)};
  return s;
}
// what the plan is made from: the batch's fragments and bases (both mates'), the splitter's w and k, the stream's settings of the piece
// route, 2^bits of the cells' taxon field, and the fragments' offsets where the host holds them ([R + 1]), else null
struct PlanInput {
  uint64_t R = 0, all_bases = 0;
  bool paired = false, want_hits = false, split_hits = false;
  int w = 0, k = 0;
  int64_t split_long = -1;
  uint32_t taxa_bound = 0;
  const uint64_t *h_offsets = nullptr;
};

// The engine's own threshold of the piece route (slk_stream_set_split_long(-1)): the smallest length at which the route measured
// faster than the routes before it by more than the spread of the runs (profiles/r16_contigs.json: 100 against 82 Gbp/s at 300 kbp,
// 105 / 41 at 1 Mbp, 108 / 10 at 4 Mbp), never under two pieces.  Unasked, the route runs only where the host can tell
// that it costs nothing: in batches whose fragments average over 1000 bases (the batches of reads -- the headline -- see no launch,
// memset or allocation of it), and while its map scratch stays under PIECE_DEFAULT_MAP_BYTES (a caller who names a threshold gets
// the scratch the batch needs, whatever it is).
// What the batch needs: with the offsets on the host (h_offsets: slk_classify_batch[_packed], slk_classify_text) the fragments at or
// above the threshold are counted and their pieces and map ranges summed exactly -- a batch without such a fragment runs nothing of
// the route.  The device entries know total_bases alone: the sums are bounds then (a cut fragment has at least min_len bases, makes at
// most n / windows + 1 pieces of its n windows, and its map has at most 4 min(n, taxa) + 64 entries), and a batch that holds
// min_len bases in all gets the header's memset, the four launches and the scratch of those bounds whether it has a long fragment or not.
constexpr int64_t PIECE_DEFAULT_MIN_LEN = 300000;
constexpr uint64_t PIECE_DEFAULT_MAP_BYTES = 2ull << 30;
// ... and under PIECE_DEFAULT_MAP_PER_BASE bytes per base of the batch: the ranges are cleared before the pieces run and read whole by
// the merge, and where they outweigh the bases the route loses what it gains (18 taxon bits, profiles/r16_contigs_18bit.json: 28 bytes
// of map per base at 300 kbp, 34 against the parent's 79 Gbp/s; 8.4 at 1 Mbp, 54 against 40; 2.1 at 4 Mbp, 59 against 10)
constexpr uint64_t PIECE_DEFAULT_MAP_PER_BASE = 8;

inline LanePlan plan_lane(const PlanInput &in, const PlanSwitches &sw) {
  LanePlan p;
  const uint64_t R = in.R, all_bases = in.all_bases;
  p.lane = !sw.force_wave && R < 0xFFFFFFFFull;
  if (!p.lane) return p;
  p.long_cap = std::min<uint64_t>(R, all_bases / 1001 + 1);
  // SLK_LANE_LONG_MAX moves the long variant's limit (at most 8191: queue entries carry 13-bit k-mer counts; 0: no such pass)
  const int long_max = (int)std::min(sw.long_max, 8191L);
  // A batch whose fragments average more than 1000 bases gets a routing kernel instead of a first pass (engine.h:
  // FusedArgs.hand_short; SLK_ROUTE_FIRST=0 / 1 says so either way)
  p.route_first = long_max > 1000 && (sw.route_first >= 0 ? sw.route_first == 1 : all_bases / 1000 > R);
  p.hand_bytes = HandOn::WORDS * sizeof(uint64_t) + HandOn::entries(R, p.long_cap, p.route_first) * sizeof(uint32_t);
  // SLK_SEG_MIN_LEN moves the segment kernel's limit (0: wave kernel only).
  // Wave or segment kernel: on batches of ONE length the wave kernel is the faster one up to ~250 000 bases since round 4's diet
  // (115 against 101 Gbp/s at 15 kbp, 111 / 100 at 30 kbp, 91 / 92 at 100 kbp, 90 / 74 at 200 kbp, 70 / 75 at 300 kbp,
  // profiles/r04_long_routes.txt) -- but it takes a fragment per wave at ~15 Mbp/s, so a fragment that is long for its batch is
  // what the batch then waits for.  So the default follows the batch: the segment kernel takes what a single wave would need
  // about half the batch's time for -- fragments of more than 1/16384 of the batch's bases --, never under 16 000 bases (below
  // that its lanes have too little each) and always from 250 000; and the wave kernel starts its long fragments longest first
  // (engine.h: hand_hdr).  Nanopore-like mix, 200 .. 50 000 bases, 1 Gbp: 90-94 Gbp/s with the threshold at 12-16 000, 93-99 at
  // 30 000, 97-101 at 64 000 (none on the segment kernel).
  const uint64_t seg_auto = std::min<uint64_t>(250000, std::max<uint64_t>(16000, all_bases >> 14));
  const int seg_min = (int)(sw.seg_min_len.set ? (long)sw.seg_min_len.v : (long)seg_auto);
  // (hit lists: the segment kernel can put them together -- SLK_SEG_HITS=1 --, but the queues that take its spans to memory
  //  in order cost it half its resident waves, and it measured 51-53 Gbp/s against the wave kernel's 68-79 on the same reads:
  //  profiles/r03_long_hits_*.json; so per-read lines of long reads keep the wave kernel unless asked otherwise)
  const bool seg_ok = !in.paired && in.w == 5 && seg_min > 0;
  p.seg_on = (!in.want_hits || sw.seg_hits) && seg_ok;
  p.long_max = long_max > 1000 ? (uint32_t)long_max : 0;
  if (p.long_max) {  // class borders: a geometric ladder from 1000 to the limit (a tile's lanes then differ by at most ~1.5x)
    const double ratio = pow((double)p.long_max / 1000.0, 0.25);
    for (int i = 0; i < 3; i++) p.long_bound[i] = (uint32_t)(1000.0 * pow(ratio, i + 1));
  }
  p.seg_min_len = p.seg_on ? (uint32_t)std::max(seg_min, (int)std::max<uint32_t>(p.long_max, 1000) + 1) : 0;
  p.wave_min = std::max<uint32_t>(p.long_max, 1000) + 1;   // (the wave kernel's eight length classes: 1.75^7 = 50 times the shortest)
  p.wave_ratio_q10 = 1792;
  // The piece route takes what the segment kernel would, cut up: same scope (unpaired, w = 5, no hit lists).  SLK_PIECE_MIN_LEN
  // overrides the stream's setting (0: off), SLK_PIECE_WINDOWS sets the piece size (a multiple of 64, at least 64 x 64).
  // A call that wants hit lists takes it only where the caller asked for both: a threshold (never the engine's own choice) and
  // slk_stream_set_split_hits, which SLK_PIECE_HITS=0|1 overrides; the segment pass is then on for the cut's sake, and unless
  // SLK_SEG_HITS says otherwise its list holds nothing but what the cut takes.
  int64_t piece_min = sw.piece_min_len.set ? (int64_t)sw.piece_min_len.v : in.split_long;
  const bool unasked = piece_min < 0;
  const bool hits_on = sw.piece_hits >= 0 ? sw.piece_hits == 1 : in.split_hits;
  if (in.want_hits ? (seg_ok && hits_on && piece_min > 0) : (p.seg_on && (unasked ? p.route_first : piece_min > 0))) {
    const uint64_t win = (uint64_t)std::max(1L, sw.piece_windows);
    p.piece_windows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((win + 63) / 64 * 64, PIECE_MIN_WINDOWS), 1u << 30);
    if (unasked) piece_min = std::max<int64_t>(PIECE_DEFAULT_MIN_LEN, 2 * (int64_t)p.piece_windows);
    const uint64_t min_len = std::min<uint64_t>(std::max<uint64_t>((uint64_t)piece_min, (uint64_t)std::max<uint32_t>(p.long_max, 1000) + 1), 0x7FFFFFFFull);
    uint64_t units = 0;
    if (in.h_offsets) {
      for (uint64_t r = 0; r < R; r++) {
        const uint64_t len = in.h_offsets[r + 1] - in.h_offsets[r];
        if (len < min_len || len > 0x7FFFFFFFull) continue;   // (host entries hold no longer fragment: validate_reads)
        const uint32_t nwin = (uint32_t)len - (uint32_t)in.k + 1;
        p.piece_frags++;
        units += (nwin + p.piece_windows - 1) / p.piece_windows;
        p.piece_map += piece_map_cap(nwin, in.taxa_bound);
      }
    } else {
      p.piece_frags = std::min<uint64_t>(R, all_bases / min_len);
      units = all_bases / p.piece_windows + p.piece_frags;
      p.piece_map = 4 * std::min<uint64_t>(all_bases, p.piece_frags * (uint64_t)in.taxa_bound) + 64 * p.piece_frags;
    }
    // (no fragment of the batch is that long, or the engine's own choice would take too much scratch: nothing of the route runs)
    const uint64_t map_bytes = p.piece_map * 2 * sizeof(int32_t);
    if (p.piece_frags != 0 && !(unasked && (map_bytes > PIECE_DEFAULT_MAP_BYTES || map_bytes > PIECE_DEFAULT_MAP_PER_BASE * all_bases))) {
      p.piece_min_len = (uint32_t)min_len;
      p.piece_units = units;
      p.piece_hits = in.want_hits;
      p.seg_min_len = p.seg_on ? std::min(p.seg_min_len, p.piece_min_len) : p.piece_min_len;
      p.seg_on = true;
    }
  }
  return p;
}

// The piece route's device scratch for a plan, in bytes: piece_scratch holds the header (at 0), the fragment slots, the unit list and
// the piece records; piece_maps the keys, then the counts; piece_hits the side records of a call with hit lists, else nothing.
struct PieceLayout { size_t frags_at, units_at, records_at, scratch_bytes, maps_bytes, hits_bytes; };
inline PieceLayout piece_layout(const LanePlan &p) {
  PieceLayout l{};
  l.frags_at = PieceHdr::WORDS * sizeof(uint64_t);
  l.units_at = l.frags_at + p.piece_frags * sizeof(PieceFrag);
  l.records_at = l.units_at + p.piece_units * sizeof(uint64_t);
  l.scratch_bytes = l.records_at + p.piece_units * sizeof(PieceRecord);
  l.maps_bytes = p.piece_map * 2 * sizeof(int32_t);
  l.hits_bytes = p.piece_hits ? p.piece_units * sizeof(PieceHitRecord) : 0;
  return l;
}

// The staged scan (kernels.hip: scan_kernel) keeps a lane's last w keys in LDS, 8 bytes each: a block of 256 lanes while that stays
// within 64 KiB, halved down to one wave beyond (w > 32).  A wave's ring is 512 w bytes, more than 64 KiB from w = 129 on; what a
// workgroup may have is the device's to say (160 KiB on MI355X: w <= 320), so slk_index_create asks scan_max_window and refuses the
// splitter whose ring no block can hold -- launch_scan never asks for more than the device gives.
struct ScanLaunch { int block; size_t lds; };
inline ScanLaunch plan_scan(int w) {
  int block = 256;
  while (block > 64 && (size_t)block * (size_t)w * 8 > 65536) block >>= 1;
  return {block, (size_t)block * (size_t)w * 8};
}
inline int scan_max_window(size_t lds_per_workgroup) { return (int)std::min<size_t>(lds_per_workgroup / (64 * 8), 512); }

// A sharded step's lookups (slk_shard_step_device) ride in the scan, their 64-key batches dealt out to its tiles -- unless the scan
// is far too short for them (a tile sends off about 2 / (w + 1) keys per base; a tile handed several times as many lookups as that
// would finish them alone, at its end, with the rest of the part idle): then they run as a kernel of their own, like those of a step
// without a scan.  Returns the 64-key batches per tile, or 0 for "a kernel of their own".
inline uint32_t shard_side_per_tile(bool scans, uint64_t R, uint64_t bases, int w, uint64_t lookups) {
  if (!scans || lookups == 0) return 0;
  const uint64_t tiles = (R + 63) / 64, batches = (lookups + 63) / 64;
  const double own = 2.0 / (w + 1) * (double)bases / 64.0 / (double)tiles;
  const uint64_t per_tile = (batches + tiles - 1) / tiles;
  return (double)per_tile <= 3.0 * own + 8.0 ? (uint32_t)per_tile : 0;
}

}  // namespace slk
