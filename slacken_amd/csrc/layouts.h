// layouts.h -- the plain layouts that the kernels and the host's plan of a batch (laneplan.h) share: the hand-on lists, the piece
// route's records and header, its constants.  No HIP header: hipcc takes it through engine.h, the host compiler alone through
// laneplan.h (tests/test_laneplan_cpu.py), and both see the same definitions.
#pragma once
#include <stdint.h>

#include <cstdlib>

// host and device under hipcc, plain inline for the host compiler alone
#ifdef __HIPCC__
#define SLK_HD __host__ __device__ __forceinline__
#else
#define SLK_HD inline
#endif

// SLK_* switches of the environment (host side; the kernels' launchers read theirs too).  Which of them are read once per process
// (a `static const` at the place of use) and which per call (tests move those) is the caller's business.
inline bool env_on(const char *name) { const char *e = getenv(name); return e != nullptr && e[0] == '1'; }
inline long env_long(const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; }

namespace slk {

// Layout of the hand-on lists and their header (engine.h: FusedArgs.hand_*)
struct HandOn {
  enum { SEG = 4, REST = 5, WAVE0 = 6, WAVE_CLASSES = 8, LATE = WAVE0 + WAVE_CLASSES, SHORT = LATE + 1, LISTS = SHORT + 1 };
  // header words: [l] = entries of list l for l < 6, then
  enum { LONG_DRAW = 6, SEG_DRAW = 7, WAVE_DRAW = 8,  // tile / unit draws of the long, segment and wave pass
         HANDED = 9,                                  // fragments handed on by the first pass (or: routed to another list than 15)
         ORDERED = 10,                                // entries of the wave pass's list as launch_order_wave_list put it together
         N_LATE = 11, LATE_DRAW = 12, N_SHORT = 13, N_WAVE0 = 16, WORDS = 32 };
  static SLK_HD int count_word(int l) {
    return l < WAVE0 ? l : l < LATE ? N_WAVE0 + (l - WAVE0) : l == LATE ? N_LATE : N_SHORT;
  }
  // where list l starts (entries from hand_lists); lists 0..5 and SHORT hold up to `stride` entries, the others `long_cap`
  static SLK_HD uint64_t list_at(int l, uint64_t stride, uint64_t long_cap) {
    return l < WAVE0 ? (uint64_t)l * stride : l < LATE ? WAVE0 * stride + (uint64_t)(l - WAVE0) * long_cap
           : l == LATE ? (WAVE0 + 1) * stride + WAVE_CLASSES * long_cap : (WAVE0 + 1) * stride + (WAVE_CLASSES + 1) * long_cap;
  }
  static SLK_HD uint64_t ordered_at(uint64_t stride, uint64_t long_cap) {   // (`stride` entries)
    return WAVE0 * stride + WAVE_CLASSES * long_cap;
  }
  static SLK_HD uint64_t entries(uint64_t stride, uint64_t long_cap, bool with_short) {
    return (WAVE0 + 1 + (with_short ? 1 : 0)) * stride + (WAVE_CLASSES + 1) * long_cap;
  }
};

// The piece route (engine.h: PieceArgs; pieces.h).  What crosses from one of its kernels to the next lies in HBM: a
// record per piece and the fragment's taxon -> count map, an open-addressing table in a range of the fragment's own (EMPTY keys,
// sized so that it cannot fill: piece_map_cap).
struct PieceRecord {                     // what a piece leaves for the merge (its inner borders are settled)
  uint64_t first_key, last_key;          // keys of its first and of its last super-mer (PIECEF_HAS)
  uint32_t flags;                        // SEGF_* of its last lane, PIECEF_* of its first
  int32_t nd, n_out, total, np;          // provisional: the borders between pieces are not settled
  uint32_t pad[3];
};
enum { PIECEF_HAS = 1, PIECEF_ENDS_OPEN = 2, PIECEF_END_AMB = 4,   // (= SEGF_*, fused.hip)
       PIECEF_STARTS_SEQ = 8,            // its first window is a k-mer of a sequence run
       PIECEF_FIRST_AMB = 16,            // its first run is an ambiguous span
       PIECEF_FIRST_NZ = 32 };           // its first super-mer has a taxon (so it was counted as a distinct hit group)
// HIT LISTS ON THE PIECE ROUTE (PieceArgs.hits != nullptr; slk_stream_set_split_hits): a piece's wave leaves its entries (taxon, meta)
// in the provisional region of span_keys -- lane j's i-th at offsets[r] + piece * windows + w0(j) + i, as the segment kernel does --
// and this record beside its PieceRecord; piece_merge_kernel fills in the plan, and piece_move_kernel, one wave per piece, moves the
// entries to their final places in span_taxon / span_meta.
struct PieceHitRecord {
  uint32_t lane[64];                     // entries of the lane << 1 | its first entry merged into the lane before (lane 0: 0)
  uint32_t head_kmers;                   // k-mers that go to the entry BEFORE the piece if a border cut its first entry: those of that
                                         // entry and of every lane's first entry that continues it
  uint32_t start;                        // the plan: where the piece's entries begin in the fragment's list,
  uint32_t cut;                          //           whether its first entry continues an earlier piece's last (then it is not stored),
  uint32_t carry;                        //           and the k-mers that LATER pieces' cut entries add to its last entry
};
struct PieceFrag {
  uint32_t r, npieces;
  uint64_t unit0;                        // its records are records[unit0 .. unit0 + npieces)
  uint64_t map0;                         // its map is map_key / map_cnt[map0 .. map0 + cap)
  uint32_t cap, shift;                   // a power of two; 32 - log2(cap)
};
struct PieceHdr {
  enum { N_FRAG = 0, N_UNIT = 1, N_MAP = 2, SPILLS = 3, UNIT_DRAW = 4,
         FAILED = 5,    // the cut ran out of scratch (PIECE_STATUS_SCRATCH): the passes behind it do nothing
         WORDS = 8 };
};
constexpr uint32_t PIECE_TAKEN = 0xFFFFFFFFu;       // entry of the segment list whose fragment went to the piece route (R < 2^32 - 1)
constexpr uint32_t PIECE_MIN_WINDOWS = 64 * 64;     // 64 lanes x SEG_MIN_WINDOWS
constexpr uint32_t PIECE_DEFAULT_WINDOWS = 64 * 1024;
constexpr int PIECE_GRID_BLOCKS = 256 * 8;          // piece_kernel's grid (four waves a block; = SLK_PIECE_GRID_WAVES / 4)
// status bits (1, 2: stream.hip check_status; 4: readform.hip): a fragment of 2^31 bases or more; the cut ran out of the scratch the
// host sized; a fragment's map range filled or held more taxa than its sizing allows (cannot happen: an internal error)
constexpr int PIECE_STATUS_TOO_LONG = 8, PIECE_STATUS_SCRATCH = 16, PIECE_STATUS_MAP = 32;
// entries of a fragment's map: its distinct taxa are at most min(windows, taxa) + 1 (NONE), held at a load of at most 0.5
SLK_HD uint32_t piece_map_cap(uint32_t nwin, uint32_t taxa_bound) {
  const uint64_t need = 2 * ((uint64_t)(nwin < taxa_bound ? nwin : taxa_bound) + 1);
  uint32_t cap = 64;
  while (cap < need) cap <<= 1;          // (taxa_bound <= 2^22 on the lane path: at most 2^24)
  return cap;
}

}  // namespace slk
