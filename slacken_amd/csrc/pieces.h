// pieces.h -- CONTIG-LENGTH FRAGMENTS SPLIT OVER MANY WAVES (engine.h: PieceArgs).  Included by fused.hip alone, behind
// that file's wave helpers (WaveLds, the LDS map, resolve_map): the piece kernel itself is segment_kernel's body (fused.hip:
// segment_body<false, true>), and what stands here is the rest of the route --
//   piece_cut_kernel    walks the segment pass's hand-on list: a fragment of at least X.min_len bases gets a slot, its range of the
//                       unit list (one unit per piece of X.windows k-mer windows, the last piece the rest), of the piece records and
//                       of the map scratch (piece_map_cap entries: it cannot fill), and leaves the list (PIECE_TAKEN).  Count, scan
//                       and scatter per wave, one atomic per wave and counter -- the host never learns the numbers
//   piece_clear_kernel  empties the map ranges handed out
//   piece_map_add/fold  a piece's taxon counts go to its fragment's map in HBM: open addressing, atomicCAS on the key and atomicAdd on
//                       the count (tablebuild.h's insert-or-add)
//   piece_merge_kernel  one wave per cut fragment: settles the borders BETWEEN pieces from the records with the rules the lanes of a
//                       piece settle theirs with (fused.hip "the borders"), sums the counts and resolves from the HBM map -- up to 128
//                       entries through the wave's LDS map and resolve_map as they are, more through the same interval arithmetic
//                       (resolve_intervals) over the fragment's range.  With hit lists (X.hits) it also writes the plan of the move
//                       into the pieces' PieceHitRecords: where each piece's entries begin in the fragment's list, whether a border
//                       cut its first entry, and the k-mers that later pieces' cut entries add to its last one
//   piece_move_kernel   hit lists only, one wave per piece: the piece's entries from the provisional region (span_keys) to their final
//                       places in span_taxon / span_meta, 64 consecutive places at a time.  It reads one buffer and writes another (a
//                       piece's final places may lie in an earlier piece's provisional stretch), and no wave adds to an entry that
//                       another wave stores: what crosses a border between pieces is in the plan's carry
// The pieces' records and map entries reach the merge across the kernel boundary: no fence wider than a workgroup in any kernel.
#pragma once
#include "engine.h"
#include "wavetools.h"

namespace slk {

__device__ __forceinline__ void piece_map_add(const PieceArgs &X, const PieceFrag &f, int32_t taxon, int32_t count, int32_t *status) {
  int32_t *const keys = X.map_key + f.map0, *const cnts = X.map_cnt + f.map0;
  const uint32_t mask = f.cap - 1;
  uint32_t slot = ((uint32_t)taxon * 0x9E3779B1u) >> f.shift;
  for (uint32_t probe = 0; probe < f.cap; probe++) {
    const int32_t old = atomicCAS(&keys[slot], MAP_EMPTY, taxon);
    if (old == MAP_EMPTY || old == taxon) {
      atomicAdd(&cnts[slot], count);
      return;
    }
    slot = (slot + 1) & mask;
  }
  atomicOr(status, PIECE_STATUS_MAP);   // (a range sized by piece_map_cap never fills: more taxa than the cells' taxon field can name)
}
// the wave's LDS map into the fragment's map, and empty again (the caller's wave_sync on either side)
__device__ __forceinline__ void piece_map_fold(WaveLds *L, const PieceArgs &X, const PieceFrag &f, int lane, int32_t *status) {
#pragma unroll
  for (int half = 0; half < 2; half++) {
    const int slot = lane + 64 * half;
    const int32_t kk = L->map_key[slot];
    if (kk != MAP_EMPTY) {
      piece_map_add(X, f, kk, L->map_cnt[slot], status);
      L->map_key[slot] = MAP_EMPTY;
      L->map_cnt[slot] = 0;
    }
  }
}

__global__ void __launch_bounds__(256) piece_cut_kernel(FusedArgs A, PieceArgs X) {
  const int lane = threadIdx.x & 63;
  const uint64_t n = (uint64_t)*X.seg_count;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4, wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (uint64_t b = wave * 64; b < n; b += nwaves * 64) {
    const uint64_t i = b + lane;
    uint32_t r = 0;
    uint64_t len = 0;
    if (i < n) { r = X.seg_list[i]; len = A.offsets[r + 1] - A.offsets[r]; }
    bool take = i < n && len >= X.min_len;
    if (take && len >= 0x80000000ull) {   // (32-bit counts, as everywhere on the fused path: refused, check_status says so)
      atomicOr(A.status, PIECE_STATUS_TOO_LONG);
      X.seg_list[i] = PIECE_TAKEN;
      take = false;
    }
    const uint32_t nwin = take ? (uint32_t)len - (uint32_t)A.P.k + 1 : 0;   // (min_len > k)
    const uint32_t npieces = take ? (nwin + X.windows - 1) / X.windows : 0;
    const uint32_t cap = take ? piece_map_cap(nwin, X.taxa_bound) : 0;
    const uint64_t T = __ballot(take);
    if (T == 0) continue;
    uint32_t iu = npieces, im = cap;   // inclusive sums over the lanes (64 x 2^19 pieces, 64 x 2^24 entries: 32 bits)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)iu, d), m = (uint32_t)__shfl_up((int)im, d);
      if (lane >= d) { iu += u; im += m; }
    }
    const uint32_t tot_f = (uint32_t)__popcll(T), tot_u = (uint32_t)__builtin_amdgcn_readlane((int)iu, 63),
                   tot_m = (uint32_t)__builtin_amdgcn_readlane((int)im, 63);
    unsigned long long bf = 0, bu = 0, bm = 0;
    if (lane == 0) {
      bf = atomicAdd(&X.hdr[PieceHdr::N_FRAG], (unsigned long long)tot_f);
      bu = atomicAdd(&X.hdr[PieceHdr::N_UNIT], (unsigned long long)tot_u);
      bm = atomicAdd(&X.hdr[PieceHdr::N_MAP], (unsigned long long)tot_m);
    }
    bf = readlane64(bf, 0); bu = readlane64(bu, 0); bm = readlane64(bm, 0);
    if (bf + tot_f > X.frag_cap || bu + tot_u > X.unit_cap || bm + tot_m > X.map_cap) {
      // (the host's bounds hold for every batch whose total_bases is true -- laneplan.h plan_lane; where they do not, nothing is
      //  written past them, the passes behind the cut do nothing, and the call fails)
      if (lane == 0) {
        atomicExch(&X.hdr[PieceHdr::FAILED], 1ull);
        atomicOr(A.status, PIECE_STATUS_SCRATCH);
      }
      continue;
    }
    if (take) {
      const uint64_t slot = bf + (uint64_t)lane_rank(T);
      PieceFrag f;
      f.r = r; f.npieces = npieces;
      f.unit0 = bu + (iu - npieces);
      f.map0 = bm + (im - cap);
      f.cap = cap; f.shift = (uint32_t)__builtin_clz(cap) + 1;   // 32 - log2(cap)
      X.frags[slot] = f;
      for (uint32_t p = 0; p < npieces; p++) X.units[f.unit0 + p] = (slot << 32) | p;
      X.seg_list[i] = PIECE_TAKEN;
    }
  }
}

// (ranges are multiples of 64 entries: whole 16-byte stores)
__global__ void __launch_bounds__(256) piece_clear_kernel(PieceArgs X) {
  const uint64_t used = (uint64_t)X.hdr[PieceHdr::N_MAP];
  const uint64_t n4 = (used < X.map_cap ? used : X.map_cap) / 4;
  int4 *const k4 = (int4 *)X.map_key, *const c4 = (int4 *)X.map_cnt;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * 256) {
    k4[i] = make_int4(MAP_EMPTY, MAP_EMPTY, MAP_EMPTY, MAP_EMPTY);
    c4[i] = make_int4(0, 0, 0, 0);
  }
}

// a fragment's map once it is dense in the front of its range, the taxa's Euler-tour intervals in the back half (piece_merge_kernel)
struct HbmMapView {
  const int32_t *tx, *ct;
  const uint32_t *tin, *tout;
  __device__ __forceinline__ int32_t taxon(int i) const { return tx[i]; }
  __device__ __forceinline__ int32_t count(int i) const { return ct[i]; }
  __device__ __forceinline__ uint32_t in(int i) const { return tin[i]; }
  __device__ __forceinline__ uint32_t out(int i) const { return tout[i]; }
};
// what other lanes of THIS wave wrote to the fragment's range (workgroup scope: fused.hip, the hit lists' scratch, says why)
__device__ __forceinline__ void piece_range_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  wave_sync();
}

__global__ void __launch_bounds__(FW * 64) piece_merge_kernel(FusedArgs A, PieceArgs X) {
  __shared__ WaveLds lds[FW];
  const int lane = threadIdx.x & 63;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  WaveLds *L = &lds[wib];
  const uint64_t nfrag = X.hdr[PieceHdr::FAILED] ? 0 : (uint64_t)X.hdr[PieceHdr::N_FRAG];
  for (uint64_t fi = (uint64_t)blockIdx.x * FW + wib; fi < nfrag; fi += (uint64_t)gridDim.x * FW) {
    const PieceFrag frag = X.frags[fi];
    const uint64_t r = frag.r;
    // ---- the borders between pieces: 64 records at a time, what went before in c_* ----
    uint64_t *const lk = L->span_key;                 // the records' last keys and flags, for the lanes' looks backwards
    uint32_t *const fg = (uint32_t *)L->span_meta;
    bool c_has = false;                               // some earlier piece has a super-mer, and the last such piece's last key
    uint64_t c_last = 0;
    uint32_t c_pflags = 0;                            // flags and last key of the piece right before this round's first
    uint64_t c_plast = 0;
    int32_t nd = 0, n_out = 0, total = 0, np = 0;
    // (hit lists) the entries of the pieces so far; the last piece so far that stores an entry, and the k-mers its last entry gets from
    // the pieces behind it -- written once the next such piece is known: an entry can be cut by many borders in a row, and a piece
    // that holds nothing but the continuation of an earlier entry stores none and passes its k-mers on
    uint32_t h_start = 0, h_carry = 0;
    int64_t h_open = -1;
    int32_t *const cr = L->result;
    for (uint32_t p0 = 0; p0 < frag.npieces; p0 += 64) {
      const uint32_t p = p0 + (uint32_t)lane;
      const bool in = p < frag.npieces;
      PieceRecord rec{};
      if (in) rec = X.records[frag.unit0 + p];
      lk[lane] = rec.last_key;
      fg[lane] = rec.flags;
      wave_sync();
      bool undo_distinct = false;
      int merged = 0;
      if (in) {
        if ((rec.flags & PIECEF_HAS) && (rec.flags & PIECEF_FIRST_NZ)) {   // the super-mer before this piece's first one: the nearest earlier piece that has any
          int q = lane - 1;
          while (q >= 0 && !(fg[q] & PIECEF_HAS)) q--;
          undo_distinct = q >= 0 ? lk[q] == rec.first_key : (c_has && c_last == rec.first_key);
        }
        if (p > 0) {
          const uint32_t fp = lane > 0 ? fg[lane - 1] : c_pflags;
          const uint64_t kp = lane > 0 ? lk[lane - 1] : c_plast;
          if ((fp & PIECEF_ENDS_OPEN) && (rec.flags & PIECEF_STARTS_SEQ) && kp == rec.first_key) merged = 1;   // one super-mer, cut
          if ((fp & PIECEF_END_AMB) && (rec.flags & PIECEF_FIRST_AMB)) merged = 1;                             // one ambiguous span, cut
        }
      }
      if (X.hits) {
        PieceHitRecord *const hr = X.hits + frag.unit0 + p;           // (in: else unused)
        const uint32_t own = in ? (uint32_t)(rec.n_out - merged) : 0u;
        const uint32_t head = (in && merged) ? hr->head_kmers : 0u;
        uint32_t incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
          if (lane >= d) incl += up;
        }
        cr[lane] = 0;
        wave_sync();
        const uint64_t NZ = __ballot(own > 0);
        const uint64_t before = NZ & ((1ull << lane) - 1);
        if (head != 0 && before != 0) atomicAdd(&cr[63 - __builtin_clzll(before)], (int32_t)head);
        h_carry += (uint32_t)wave_sum((head != 0 && before == 0) ? (int32_t)head : 0);
        wave_sync();
        const int last_nz = NZ ? 63 - __builtin_clzll(NZ) : -1;
        if (NZ != 0 && h_open >= 0 && lane == 0) X.hits[frag.unit0 + (uint64_t)h_open].carry = h_carry;
        if (in) {
          hr->start = h_start + incl - own;
          hr->cut = (uint32_t)merged;
          if (lane != last_nz) hr->carry = (uint32_t)cr[lane];
        }
        if (NZ != 0) { h_open = (int64_t)p0 + last_nz; h_carry = (uint32_t)cr[last_nz]; }
        h_start += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      }
      nd += rec.nd - (undo_distinct ? 1 : 0);
      n_out += rec.n_out - merged;
      total += rec.total;
      np += rec.np;
      const uint64_t H = __ballot(in && (rec.flags & PIECEF_HAS));
      if (H != 0) { c_has = true; c_last = lk[63 - __builtin_clzll(H)]; }
      const uint32_t cnt = min(64u, frag.npieces - p0);
      c_pflags = fg[cnt - 1];
      c_plast = lk[cnt - 1];
      wave_sync();
    }
    nd = wave_sum(nd); n_out = wave_sum(n_out); total = wave_sum(total); np = wave_sum(np);
    if (X.hits && lane == 0) {
      if (h_open >= 0) X.hits[frag.unit0 + (uint64_t)h_open].carry = h_carry;
      A.span_count[r] = n_out;
    }

    // ---- the map: dense in the front of its range (in place: an entry moves down, to slots that have been read) ----
    int32_t *const mk = X.map_key + frag.map0, *const mc = X.map_cnt + frag.map0;
    uint32_t D = 0;
    for (uint32_t s0 = 0; s0 < frag.cap; s0 += 64) {
      const int32_t kk = mk[s0 + lane], cc = mc[s0 + lane];
      const uint64_t O = __ballot(kk != MAP_EMPTY);
      if (kk != MAP_EMPTY) {
        const uint32_t d = D + (uint32_t)lane_rank(O);
        mk[d] = kk; mc[d] = cc;
      }
      D += (uint32_t)__popcll(O);
    }
    piece_range_sync();
    if (D <= (uint32_t)MAP_CAP) {
      L->map_key[lane] = MAP_EMPTY; L->map_key[lane + 64] = MAP_EMPTY;
      L->map_cnt[lane] = 0; L->map_cnt[lane + 64] = 0;
      wave_sync();
      for (uint32_t i = lane; i < D; i += 64) (void)map_try_insert(L, mk[i], mc[i]);   // (at most MAP_CAP keys: every one finds a slot)
      wave_sync();
      resolve_map(L, A, r, lane, total, nd);
    } else if (D <= frag.cap / 2 && A.nodes != nullptr) {
      const uint32_t half = frag.cap / 2;             // (piece_map_cap: the taxa fill at most half the range)
      for (uint32_t i = lane; i < D; i += 64) {
        const uint4 nn = tax_node(A.nodes, A.ntax, mk[i]);
        mk[half + i] = (int32_t)nn.y; mc[half + i] = (int32_t)nn.z;
      }
      piece_range_sync();
      resolve_intervals(L, A, r, lane, total, nd, HbmMapView{mk, mc, (const uint32_t *)mk + half, (const uint32_t *)mc + half}, (int)D);
    } else {
      if (lane == 0) atomicOr(A.status, PIECE_STATUS_MAP);   // (the lane path has an Euler tour, and the range was sized for its taxa)
    }
    if (lane == 0) {
      if (A.out_nd) A.out_nd[r] = nd;
      if (A.out_tk) A.out_tk[r] = total;
      if (A.out_nh) A.out_nh[r] = n_out;
      if (A.out_np) A.out_np[r] = np;
    }
    wave_sync();
  }
}

// the lanes' ends in the piece's part of the list, and whether a lane's first entry is left out (it went into the entry before it)
struct __attribute__((aligned(16))) MoveLds {
  uint32_t end[64], skip[64];
};
__global__ void __launch_bounds__(256) piece_move_kernel(FusedArgs A, PieceArgs X) {
  __shared__ MoveLds lds[4];
  const int lane = threadIdx.x & 63;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  MoveLds *M = &lds[wib];
  const uint64_t nunits = X.hdr[PieceHdr::FAILED] ? 0 : (uint64_t)X.hdr[PieceHdr::N_UNIT];
  for (uint64_t unit = (uint64_t)blockIdx.x * 4 + wib; unit < nunits; unit += (uint64_t)gridDim.x * 4) {
    const uint64_t u = X.units[unit];
    const PieceFrag frag = X.frags[u >> 32];
    const uint32_t piece = (uint32_t)u;
    const uint64_t fo = A.offsets[frag.r];
    const uint32_t w_first = piece * X.windows;
    const uint32_t nwin = min(X.windows, (uint32_t)(A.offsets[frag.r + 1] - fo) - (uint32_t)A.P.k + 1 - w_first);
    const uint32_t S = max(SEG_MIN_WINDOWS, (nwin + 63) / 64);          // (segment_body: lane j's stretch starts at j * S)
    const PieceHitRecord *const hr = X.hits + frag.unit0 + piece;
    const uint2 *const prov = (const uint2 *)A.span_keys + fo + w_first;
    const uint64_t dst = fo + hr->start;
    const uint32_t carry = hr->carry;
    const uint32_t v = hr->lane[lane];
    const uint32_t lcount = v >> 1;
    const uint32_t skip = min(lcount, lane == 0 ? hr->cut : (v & 1u));
    const uint32_t kept = lcount - skip;
    uint32_t incl = kept;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t off = incl - kept;
    M->end[lane] = incl;
    M->skip[lane] = skip;
    wave_sync();
    const uint32_t n_list = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    for (uint32_t t = lane; t < n_list; t += 64) {
      int j = 0;
#pragma unroll
      for (int b = 32; b > 0; b >>= 1) j += (M->end[j + b - 1] <= t) ? b : 0;   // the first lane whose end lies beyond t
      const uint32_t begin = j > 0 ? M->end[j - 1] : 0u;
      uint2 e = prov[(uint64_t)j * S + M->skip[j] + (t - begin)];
      if (t == n_list - 1) e.y += carry << 4;                                  // (engine.h pack_meta: k-mers << 4)
      A.span_taxon[dst + t] = (int32_t)e.x;
      A.span_meta[dst + t] = (int32_t)e.y;
    }
    // the entries cut by a border between two lanes of the piece: into the entry before them, which this wave has just stored (those
    // whose entry before lies in an earlier piece -- off == 0 -- are in that piece's carry)
    piece_range_sync();
    if (skip && off > 0) atomicAdd(&A.span_meta[dst + off - 1], meta_kmers((int32_t)prov[(uint64_t)lane * S].y) << 4);
    wave_sync();
  }
}

}  // namespace slk
