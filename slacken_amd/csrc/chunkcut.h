// chunkcut.h -- how the host hands sequences to the lane-per-chunk scan (chunkscan.h): groups of whole sequences that fit the device
// buffer, every sequence cut into chunks of at most `cw` k-mer windows.  Plain C++, no HIP: index.hip (library construction),
// coverage.hip and support.hip include it, and tests/test_chunkcut_cpu.py compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>

namespace slk {

// The end j of the group of whole sequences that starts at sequence i < R: as many as lie within group_bytes, one at least.
inline uint64_t group_end(const uint64_t *offsets, uint64_t i, uint64_t R, uint64_t group_bytes) {
  uint64_t j = i;
  while (j < R && (j == i || offsets[j + 1] - offsets[i] <= group_bytes)) j++;
  return j;
}

// The chunks of sequences [i, j): emit(q, start, bases, early) for every chunk of sequence q, `start` counted from the group's first
// base (offsets[i]).  A sequence with skip(q), or shorter than k, has none.  Every chunk covers up to cw windows of its own, that is
// windows + k - 1 bases.  exact_seams: a chunk that is not the first of its sequence starts one base early (`early` = 1: it has one
// base more, and its first window, the last of the chunk before, only primes the scan -- chunkscan.h); otherwise neighbours overlap
// by k - 1 bases, a window belongs to one chunk, and a super-mer across the seam is seen by both.
template <class Skip, class Emit>
inline void cut_chunks(const uint64_t *offsets, uint64_t i, uint64_t j, uint32_t k, uint32_t cw, bool exact_seams, Skip &&skip, Emit &&emit) {
  for (uint64_t q = i; q < j; q++) {
    const uint64_t len = offsets[q + 1] - offsets[q];
    if (len < k || skip(q)) continue;
    const uint64_t windows = len - k + 1;
    for (uint64_t w0 = 0; w0 < windows; w0 += cw) {
      const uint64_t nw = std::min<uint64_t>(cw, windows - w0);
      const uint32_t early = exact_seams && w0 ? 1 : 0;
      emit(q, offsets[q] - offsets[i] + w0 - early, (uint32_t)(nw + k - 1 + early), early);
    }
  }
}

}  // namespace slk
