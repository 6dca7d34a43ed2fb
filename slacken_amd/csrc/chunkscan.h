// chunkscan.h -- the lane-per-chunk scan that build.hip, coverage.hip and support.hip share: one lane walks a chunk of a sequence base by base,
// keeps the last w m-mer keys in its column of an LDS ring and the window's minimum beside them, and tells its caller at every base
// whether a k-mer window of the chunk ends there and whether that window starts a new super-mer.  What is done with a super-mer --
// inserted (build.hip) or looked up (coverage.hip) when it starts, or looked up when it closes and its windows are known
// (support.hip) -- is the caller's.
//
// Seams.  build.hip only needs the SET of minimizers: its chunks overlap by k - 1 bases, a super-mer that straddles a seam is found
// twice, and it never primes.  Where that would be counted twice (coverage.hip, support.hip), a chunk that is not the first of its
// sequence starts ONE base early (`prime`; an overlap of k with the chunk before): the
// window that ends at its step k - 1 is the last window of the chunk before, and it only primes cur_val / have_cur -- it is not
// reported.  If that window holds an invalid base, nvalid does not reach k there, nothing is primed, and the chunk's first own
// window rightly starts a new segment.
#pragma once
#include "engine.h"
#include "wavetools.h"

namespace slk {

struct ChunkScan {
  enum { NO_WINDOW = 0, SAME = 1, FRESH = 2 };   // step(): no window of the chunk ends here / one of the running super-mer / the first of a new one
  uint64_t fwd = 0, rc = 0, minv = ~0ULL, cur_val = 0, lo = 0, hi = 0;   // cur_val: the minimizer of the window reported last
  uint32_t nvalid = 0;
  int head, minage = 0;
  bool have_cur = false;

  __device__ __forceinline__ explicit ChunkScan(int w) : head(w - 1) {}

  // Base `step` of the chunk of `len` bases at bases + start (steps beyond len count as invalid: the lanes of a wave walk in
  // lockstep to the longest chunk).  ring: [w][stride] keys, this lane's column is `tid`.  total_bases: the bytes of the buffer.
  __device__ __forceinline__ int step(const ScanParams &P, uint64_t *ring, uint32_t stride, uint32_t tid, const uint8_t *bases, uint64_t start,
                                      uint64_t total_bases, uint32_t step, uint32_t len, bool prime) {
    const int w = P.w;
    if ((step & 15) == 0) {  // 16 bytes per lane every 16 steps (the buffer's last block: byte loads, engine.h)
      uint4 v = make_uint4(0, 0, 0, 0);
      if (step < len) v = load_block16(bases + start + step, clamp_room(total_bases - start - step));
      lo = ((uint64_t)v.y << 32) | v.x;
      hi = ((uint64_t)v.w << 32) | v.z;
    }
    const uint32_t ch = (uint32_t)(lo & 0xff);
    lo = (lo >> 8) | (hi << 56);
    hi >>= 8;
    const int t = (step < len) ? base_code(ch) : 5;
    if (t >= 4) {  // InputReader.removeInvalid (InputReader.scala:60-72): sequences are split around anything else
      nvalid = 0; fwd = 0; rc = 0; head = w - 1; minage = 0; minv = ~0ULL; have_cur = false;
      return NO_WINDOW;
    }
    nvalid++;
    fwd = (fwd << 2) | ((uint64_t)t << P.sh);
    rc = ((rc >> 2) | ((uint64_t)(3 - t) << 62)) & P.keep;
    if (nvalid < (uint32_t)P.m) return NO_WINDOW;
    const uint64_t canon = (P.canonical && rc < fwd) ? rc : fwd;
    const uint64_t key = (canon ^ P.xmask) & P.smask;
    head = (head + 1 == w) ? 0 : head + 1;
    ring[(uint32_t)head * stride + tid] = key;
    if (key <= minv) { minv = key; minage = 0; }
    else if (++minage >= w) {
      int slot = (head + 1 == w) ? 0 : head + 1;
      minv = ~0ULL;
      for (int a = w - 1; a >= 0; a--) {
        const uint64_t v = ring[(uint32_t)slot * stride + tid];
        if (v <= minv) { minv = v; minage = a; }
        slot = (slot + 1 == w) ? 0 : slot + 1;
      }
    }
    if (nvalid < (uint32_t)P.k) return NO_WINDOW;
    const bool fresh = !have_cur || minv != cur_val;   // a new super-mer starts
    have_cur = true;
    cur_val = minv;
    if (prime && step == (uint32_t)(P.k - 1)) return NO_WINDOW;   // (the priming window belongs to the chunk before)
    return fresh ? FRESH : SAME;
  }
};

}  // namespace slk
