// textlines.h -- what the passes over raw text share (textparse.hip: FASTA / FASTQ records; compare.hip: the lines of TSV mappings):
// the tile layout, the block scans, the line-start rule with its count / scan / scatter passes, and the byte comparison of two
// strings that lie at any alignment.  Everything sits in an unnamed namespace: each translation unit holds its own kernels.  Internal.
//
// Layout.  A TILE is TL_TILE = 4096 bytes: a block of 256 lanes, 16 bytes per lane in one load (the text must be 16-byte aligned; the
// bytes past n are never read: a lane whose 16 bytes cross n assembles them from byte loads).  Inside a block, ranks are wave scans
// (shuffles; ballots and mbcnt where a lane holds one flag) and four wave totals in LDS.  Across blocks every quantity takes the
// count / scan / scatter shape of export.hip: a pass leaves one number per tile, one block scans the tiles' numbers, the next pass
// reads its tile's carry.  No block waits for another inside a kernel.
#pragma once
#include "hostside.h"

namespace {

constexpr int TL_BLOCK = 256;
constexpr int TL_LANE_BYTES = 16;
constexpr uint32_t TL_TILE = TL_BLOCK * TL_LANE_BYTES;
constexpr int TL_SCAN_BLOCK = 1024;
constexpr unsigned TL_MAX_GRID = 2048;   // 256 CUs x 8 blocks; the kernels stride over their tiles

struct TpArgs {
  const uint8_t *text;
  uint64_t n;          // bytes of text (< 2^32)
  uint32_t ntiles;     // tiles of TL_TILE positions (FASTA, final: n + 1 positions -- the end of the text closes a record)
  uint32_t final;
  uint32_t *tiles;     // per-tile numbers, arrays of ntiles + 1 (the scan leaves the total behind the last tile's carry)
  uint32_t *S;         // FASTQ: line starts [M + 2], S[M] = S[M + 1] = n
  uint32_t *dst;       // FASTQ: [M + 1] where in `bases` line j goes, TP_NONE = nowhere
  uint32_t *ltiles;    // FASTQ: per 256 lines, two arrays of nlt_max + 1: records, sequence bytes
  uint32_t nlt_max;
  uint8_t *bases;
  uint64_t bases_capacity;
  uint64_t *offsets;
  uint64_t *title_pos;
  uint32_t *title_len;
  uint64_t records_capacity;
  uint64_t *counts;    // [4]: records, bases, consumed, overflow
};

__device__ __forceinline__ uint32_t tp_op(bool mx, uint32_t a, uint32_t b) { return mx ? (a > b ? a : b) : a + b; }

// exclusive prefix of v over the block's 256 lanes (sum, or max with 0 as "nothing"); total = over all of them.  lds: 4 words.
template <bool MAX>
__device__ __forceinline__ uint32_t tp_block_excl(uint32_t v, uint32_t *lds, uint32_t &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc = tp_op(MAX, inc, t);
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < TL_BLOCK / 64; i++) {
    const uint32_t t = lds[i];
    if (i < w) before = tp_op(MAX, before, t);
    total = tp_op(MAX, total, t);
  }
  __syncthreads();   // (the words are free again)
  uint32_t excl = __shfl_up(inc, 1, 64);
  if (lane == 0) excl = 0;
  return tp_op(MAX, before, excl);
}

// the lane's 16 positions [p, p + 16) as four words, little-endian; positions at or beyond n read as 0 and are not touched in memory
__device__ __forceinline__ void tp_load16(const uint8_t *text, uint64_t n, uint64_t p, uint32_t (&w)[4]) {
  if (p + TL_LANE_BYTES <= n) {
    const uint4 v = *(const uint4 *)(text + p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int k = 0; k < TL_LANE_BYTES; k++)
      if (p + k < n) w[k >> 2] |= (uint32_t)text[p + k] << ((k & 3) * 8);
  }
}
__device__ __forceinline__ uint32_t tp_byte(const uint32_t (&w)[4], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu; }
__device__ __forceinline__ uint32_t tp_below(uint32_t mask, int k) { return mask & ((1u << k) - 1u); }
__device__ __forceinline__ int tp_top(uint32_t mask) { return 31 - __clz((int)mask); }   // mask != 0

// per-tile arrays, scanned in place by one block each: v[i] = what tiles 0 .. i - 1 hold, v[count] = what all hold.  The count is
// given, or ceil(*m_dev / div) where only the device knows it; bit a of max_mask: array a is a max-scan, else a sum.
__global__ void __launch_bounds__(TL_SCAN_BLOCK) tp_scan_kernel(uint32_t *base, uint64_t stride, uint32_t count, const uint32_t *m_dev,
                                                                uint32_t div, uint32_t max_mask) {
  __shared__ uint32_t part[TL_SCAN_BLOCK];
  uint32_t *v = base + (uint64_t)blockIdx.x * stride;
  const bool mx = (max_mask >> blockIdx.x) & 1u;
  const uint64_t n = m_dev ? ((uint64_t)*m_dev + div - 1) / div : count;
  const uint64_t per = (n + TL_SCAN_BLOCK - 1) / TL_SCAN_BLOCK;
  const uint64_t a = umin64(n, threadIdx.x * per), b = umin64(n, a + per);
  uint32_t acc = 0;
  for (uint64_t g = a; g < b; g++) acc = tp_op(mx, acc, v[g]);
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 1; o < TL_SCAN_BLOCK; o <<= 1) {
    const uint32_t add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] = tp_op(mx, part[threadIdx.x], add);
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (uint64_t g = a; g < b; g++) {
    const uint32_t x = v[g];
    v[g] = run;
    run = tp_op(mx, run, x);
  }
  if (threadIdx.x == TL_SCAN_BLOCK - 1) v[n] = part[TL_SCAN_BLOCK - 1];
}

// ---- lines --------------------------------------------------------------------------------------------------------------------

// bit k: position p + k (< n) starts a line -- seqio.hpp: is_line_start
__device__ __forceinline__ uint32_t fq_start_mask(const TpArgs &A, uint64_t p, const uint32_t (&w)[4]) {
  if (p >= A.n) return 0;
  uint32_t prev = p ? A.text[p - 1] : '\n';
  uint32_t mask = 0;
#pragma unroll
  for (int k = 0; k < TL_LANE_BYTES; k++) {
    const uint32_t c = tp_byte(w, k);
    if (p + k < A.n && (prev == '\n' || (prev == '\r' && c != '\n'))) mask |= 1u << k;
    prev = c;
  }
  return mask;
}

// WRITE = 0: tiles[t] = the line starts of tile t.  WRITE = 1 (tiles scanned): S[] = their positions, in order.
template <int WRITE>
__global__ void __launch_bounds__(TL_BLOCK) fq_lines_kernel(TpArgs A) {
  __shared__ uint32_t lds[TL_BLOCK / 64];
  for (uint32_t t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
    const uint64_t p = (uint64_t)t * TL_TILE + threadIdx.x * TL_LANE_BYTES;
    uint32_t w[4];
    tp_load16(A.text, A.n, p, w);
    const uint32_t mask = fq_start_mask(A, p, w);
    uint32_t total;
    const uint32_t excl = tp_block_excl<false>(__popc(mask), lds, total);
    if (!WRITE) {
      if (threadIdx.x == 0) A.tiles[t] = total;
    } else {
      uint32_t j = A.tiles[t] + excl;
      for (uint32_t m = mask; m; m &= m - 1) A.S[j++] = (uint32_t)(p + (__ffs((int)m) - 1));
      if (t == 0 && threadIdx.x == 0) {
        const uint32_t M = A.tiles[A.ntiles];
        A.S[M] = (uint32_t)A.n;
        A.S[M + 1] = (uint32_t)A.n;
      }
    }
  }
}

// the end of the line [s, next) without its terminator (\n, \r\n, \r or, on the last line of the text, none)
__device__ __forceinline__ uint32_t fq_line_end(const uint8_t *text, uint32_t s, uint32_t next) {
  uint32_t e = next;
  if (e > s && text[e - 1] == '\n') {
    e--;
    if (e > s && text[e - 1] == '\r') e--;
  } else if (e > s && text[e - 1] == '\r') {
    e--;
  }
  return e;
}

// ---- strings ------------------------------------------------------------------------------------------------------------------

// Strings lie at any alignment in two buffers: eight bytes at a time while eight are left INSIDE the string, single bytes for the rest --
// no load reaches past the string's last byte, so none reaches past its buffer.
__device__ __forceinline__ bool pt_equal(const uint8_t *a, const uint8_t *b, uint32_t len) {
  uint32_t k = 0;
  for (; k + 8 <= len; k += 8) {
    uint64_t x, y;
    __builtin_memcpy(&x, a + k, 8);
    __builtin_memcpy(&y, b + k, 8);
    if (x != y) return false;
  }
  for (; k < len; k++)
    if (a[k] != b[k]) return false;
  return true;
}

}  // namespace
