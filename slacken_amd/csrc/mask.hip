// mask.hip -- low-complexity masking of genomes on the device (include/slacken_amd.h: slk_mask_*): the symmetric DUST
// of Morgulis et al. 2006 as the reference's library preparation applies it (scripts/k2/mask_low_complexity.sh: k2mask -r x),
// pinned to the published definition in integers.  The serial statement of the same function is slacken_amd/host/mask.hpp.
//
// The recurrence.  M(a, b), the best score of any sub-interval of the triplet interval [a, b], is the exact pair (S, l - 1);
// M(a, b) = max(score(a, b), M(a + 1, b), M(a, b - 1)) by cross-multiplication, and [a, b] is perfect iff it is good and
// score(a, b) >= max(M(a + 1, b), M(a, b - 1)).  One lane per start a, all lanes at the same length d = b - a: M(a, b - 1) is the
// lane's own value of the step before, M(a + 1, b) the next lane's, read from a row in LDS.  A step is one triplet fetched, one
// counter bumped (S += c before the increment), two compares and the exchange.
//
// Three kernels on the stream: the sequence starts go to a bitmap; the tiles find the perfect intervals and OR the letters they cover
// into a second bitmap; the last pass rewrites the letters whose bit is set.  The letters are only read until that last pass, so a
// tile never sees a letter that another tile has already replaced.
#include "hostside.h"
#include "wavetools.h"

namespace {

constexpr uint32_t MK_THREADS = 512;                  // lanes of a tile: one interval start each
constexpr uint32_t MK_HALO = 64;                      // the last lanes only feed M(a + 1, .) to the lanes before them
constexpr uint32_t MK_TILE = MK_THREADS - MK_HALO;    // starts a tile answers for (a multiple of 64: its first mask word is whole)
constexpr uint32_t MK_LETTERS = MK_THREADS + 64;      // letters a tile reads: the last lane's longest interval ends 63 letters on
constexpr uint32_t MK_WORDS = MK_LETTERS / 32;
constexpr uint32_t MK_MAX_GRID = 1u << 20;
static_assert(MK_TILE % 64 == 0 && MK_LETTERS % 64 == 0, "whole ballots and whole mask words per tile");
static_assert(MK_HALO >= 64 - 4, "a wrong M(a + 1, .) at the tile's end moves one lane to the left per step: window - 3 steps");

struct MaskArgs {
  const uint8_t *bases;
  uint64_t n;             // letters
  const uint32_t *starts; // bit p: a sequence starts at letter p
  uint32_t *mask;         // bit p: letter p lies in a perfect interval
  uint64_t n_words;       // words of either bitmap
  uint64_t n_tiles;
  uint32_t window, threshold;
};

__device__ __forceinline__ uint32_t mask_code(uint8_t c) {   // A C G T/U in either case: 0..3; everything else: 4
  switch (c | 0x20) { case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': case 'u': return 3; default: return 4; }
}

__global__ void mask_starts_kernel(const uint64_t *offsets, uint64_t n_sequences, uint64_t n, uint32_t *starts) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_sequences; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o = offsets[i];
    if (o < n) atomicOr(&starts[o >> 5], 1u << (o & 31));
  }
}

__device__ __forceinline__ uint32_t pack_score(uint32_t s, uint32_t d) { return s << 8 | d; }   // S <= 1891, l - 1 <= 61

__global__ __launch_bounds__(MK_THREADS) void mask_tile_kernel(MaskArgs A) {
  // the lanes' triplet counters, a byte each: counter v of lane i is byte v & 3 of word (v >> 2) * MK_THREADS + i -- a lane's words
  // are its own, and the lanes of a wave fall on 32 different banks twice over
  __shared__ uint32_t counters[16 * MK_THREADS];
  __shared__ uint32_t row[2][MK_THREADS + 1];        // M of every lane after the step before (and after this one)
  __shared__ uint8_t code[MK_LETTERS];
  __shared__ uint8_t trip[MK_LETTERS];
  __shared__ uint64_t stops[MK_LETTERS / 64 + 1];    // bit q: letter q of the tile is invalid, lies past the end, or starts a sequence
  __shared__ uint32_t marks[MK_WORDS];
  const uint32_t i = threadIdx.x, lane = i & 63;
  uint8_t *const cb = (uint8_t *)counters;
  auto counter = [&](uint32_t v) -> uint8_t & { return cb[((v >> 2) * MK_THREADS + i) * 4 + (v & 3)]; };
  auto clear_counters = [&] {
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) counters[k * MK_THREADS + i] = 0;
  };

  for (uint64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const uint64_t p0 = tile * MK_TILE;
    // (the second round is wave 0's alone, whole: the ballots stay wave-uniform)
    for (uint32_t q = i; q < MK_LETTERS; q += MK_THREADS) {
      const uint64_t p = p0 + q;
      uint32_t c = 4;
      bool starts = false;
      if (p < A.n) {
        c = mask_code(A.bases[p]);
        starts = (A.starts[p >> 5] >> (p & 31)) & 1;
      }
      code[q] = (uint8_t)c;
      const uint64_t stop = __ballot(c > 3 || starts);
      if (lane == 0) stops[q >> 6] = stop;
    }
    if (i == 0) stops[MK_LETTERS / 64] = ~0ULL;
    if (i < MK_WORDS) marks[i] = 0;
    __syncthreads();
    for (uint32_t q = i; q + 2 < MK_LETTERS; q += MK_THREADS)   // (a triplet with an invalid letter is never fetched by a live lane)
      trip[q] = (uint8_t)((code[q] << 4 | code[q + 1] << 2 | code[q + 2]) & 63);
    // the letters of this lane's run from its own letter on, 64 at the most
    const uint32_t q1 = i + 1;
    uint64_t bits = stops[q1 >> 6] >> (q1 & 63);
    if (q1 & 63) bits |= stops[(q1 >> 6) + 1] << (64 - (q1 & 63));
    const uint32_t run = code[i] > 3 ? 0 : 1 + (bits ? (uint32_t)__ffsll((unsigned long long)bits) - 1 : 64);
    const uint32_t span = min(run, A.window);
    const uint32_t steps = span >= 3 ? span - 3 : 0;   // lengths d = 1 .. steps: the interval [a, a + d] needs the letters a .. a + d + 2
    __syncthreads();

    // first the scores alone, without M and without the exchange: a perfect interval is good, and most tiles hold no good one
    clear_counters();
    bool good = false;
    if (steps && i < MK_TILE) {
      counter(trip[i]) = 1;
      uint32_t S = 0;
      for (uint32_t d = 1; d <= steps; d++) {
        uint8_t &c = counter(trip[i + d]);
        S += c;
        c++;
        good |= 10 * S > A.threshold * d;
      }
    }
    if (!__syncthreads_or(good)) continue;

    clear_counters();
    if (steps) counter(trip[i]) = 1;
    row[0][i] = pack_score(0, 1);   // an interval of one triplet counts as (0, 1)
    if (i == 0) row[0][MK_THREADS] = row[1][MK_THREADS] = pack_score(0, 1);
    __syncthreads();
    uint32_t S = 0, mS = 0, mD = 1, reach = 0;
    for (uint32_t d = 1; d + 3 <= A.window; d++) {
      const uint32_t cur = d & 1;
      if (d <= steps) {
        uint8_t &c = counter(trip[i + d]);
        S += c;
        c++;
        const uint32_t up = row[cur ^ 1][i + 1], uS = up >> 8, uD = up & 255;   // (lane i + 1 was live at d - 1 whenever this one is at d)
        const bool take_up = uS * mD > mS * uD;
        const uint32_t bS = take_up ? uS : mS, bD = take_up ? uD : mD;
        const bool on_top = S * bD >= bS * d;   // a tie keeps the interval
        if (on_top && 10 * S > A.threshold * d) reach = d + 3;
        mS = on_top ? S : bS;
        mD = on_top ? d : bD;
        row[cur][i] = pack_score(mS, mD);
      }
      __syncthreads();
    }
    // letters i .. i + reach - 1 of the tile (at most letter MK_TILE + 62), first into the tile's words, then into the device's
    if (reach && i < MK_TILE) {
      const uint32_t lo = i, hi = i + reach;
      for (uint32_t w = lo >> 5; w <= (hi - 1) >> 5; w++) {
        const uint32_t a = max(lo, w * 32) - w * 32, b = min(hi, w * 32 + 32) - w * 32;
        atomicOr(&marks[w], (b - a == 32 ? ~0u : (1u << (b - a)) - 1) << a);
      }
    }
    __syncthreads();
    if (i < MK_WORDS && marks[i]) {
      const uint64_t w = (p0 >> 5) + i;
      if (w < A.n_words) atomicOr(&A.mask[w], marks[i]);
    }
    __syncthreads();
  }
}

// the letters [lo, hi) whose bit is set become `replacement` (0: lower case); *count grows by the letters that changed
__global__ void mask_apply_kernel(uint8_t *bases, const uint32_t *mask, uint64_t lo, uint64_t hi, uint8_t replacement, unsigned long long *count) {
  uint32_t changed = 0;
  if (lo < hi) {
    const uint64_t w0 = lo >> 5, w1 = (hi - 1) >> 5;
    for (uint64_t w = w0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= w1; w += (uint64_t)gridDim.x * blockDim.x) {
      uint32_t m = mask[w];
      if (w == w0) m &= ~0u << (lo & 31);
      if (w == w1 && (hi & 31)) m &= ~0u >> (32 - (hi & 31));
      while (m) {
        const uint64_t p = w * 32 + (uint32_t)__ffs((int)m) - 1;
        m &= m - 1;
        const uint8_t c = bases[p], r = replacement ? replacement : (uint8_t)(c | 0x20);
        if (r != c) { bases[p] = r; changed++; }
      }
    }
  }
  const uint32_t total = wave_sum32(changed);
  if ((threadIdx.x & 63) == 0 && total) atomicAdd(count, (unsigned long long)total);
}

int32_t check_mask_config(const slk_mask_config *cfg, slk_mask_config *out) {
  slk_mask_config c{64, 20, 0};
  if (cfg) { c = *cfg; if (!c.window) c.window = 64; if (!c.threshold) c.threshold = 20; }
  if (c.window < 8 || c.window > 64) return fail(SLK_E_INVALID, "mask window %u outside 8..64", c.window);
  if (c.threshold < 1 || c.threshold > 255) return fail(SLK_E_INVALID, "mask threshold %u outside 1..255", c.threshold);
  *out = c;
  return SLK_OK;
}

// The three kernels over n letters on the device, queued on the stream; letters [lo, hi) are rewritten and counted into *d_count
// (which is not cleared here).  Scratch: the stream's, two bits per letter.
int32_t queue_mask(slk_stream *st, uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_sequences, uint64_t n, const slk_mask_config &c,
                   uint64_t lo, uint64_t hi, uint64_t *d_count) {
  if (n == 0 || lo >= hi) return SLK_OK;
  hipStream_t s = st->s;
  const uint64_t n_words = (n + 31) / 32;
  HIPCHK(st->mask_scratch.ensure(2 * n_words * 4));
  HIPCHK(hipMemsetAsync(st->mask_scratch.p, 0, 2 * n_words * 4, s));
  MaskArgs A{};
  A.bases = d_bases; A.n = n;
  A.starts = st->mask_scratch.as<uint32_t>();
  A.mask = st->mask_scratch.as<uint32_t>() + n_words;
  A.n_words = n_words;
  A.n_tiles = (n + MK_TILE - 1) / MK_TILE;
  A.window = c.window; A.threshold = c.threshold;
  const unsigned start_blocks = (unsigned)std::min<uint64_t>((n_sequences + 1 + 255) / 256, MK_MAX_GRID);
  hipLaunchKernelGGL(mask_starts_kernel, dim3(start_blocks), dim3(256), 0, s, d_offsets, n_sequences, n, st->mask_scratch.as<uint32_t>());
  hipLaunchKernelGGL(mask_tile_kernel, dim3((unsigned)std::min<uint64_t>(A.n_tiles, MK_MAX_GRID)), dim3(MK_THREADS), 0, s, A);
  const uint64_t apply_words = ((hi - 1) >> 5) - (lo >> 5) + 1;
  hipLaunchKernelGGL(mask_apply_kernel, dim3((unsigned)std::min<uint64_t>((apply_words + 255) / 256, MK_MAX_GRID)), dim3(256), 0, s, d_bases,
                     A.mask, lo, hi, c.replacement, (unsigned long long *)d_count);
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

}  // namespace

extern "C" uint32_t slk_mask_tile_bases(void) { return MK_TILE; }

extern "C" int32_t slk_mask_device(slk_stream *st, uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_sequences, const slk_mask_config *cfg,
                                   uint64_t *d_masked) {
  if (!st || !d_offsets || !d_masked) return fail(SLK_E_INVALID, "null argument");
  slk_mask_config c;
  int32_t rc = check_mask_config(cfg, &c);
  if (rc) return rc;
  if ((rc = set_device(st->ix))) return rc;
  uint64_t n = 0;
  if ((rc = copy_out(st, &n, d_offsets + n_sequences, 8))) return rc;   // (waits for what the stream holds)
  if (n && !d_bases) return fail(SLK_E_INVALID, "null argument");
  HIPCHK(hipMemsetAsync(d_masked, 0, 8, st->s));
  return queue_mask(st, d_bases, d_offsets, n_sequences, n, c, 0, n, d_masked);
}

extern "C" int32_t slk_mask_sequences(slk_stream *st, uint8_t *bases, const uint64_t *offsets, uint64_t n_sequences, const slk_mask_config *cfg,
                                      uint64_t *out_masked) {
  if (!st || !offsets || !out_masked) return fail(SLK_E_INVALID, "null argument");
  *out_masked = 0;
  slk_mask_config c;
  int32_t rc = check_mask_config(cfg, &c);
  if (rc) return rc;
  if (offsets[0] != 0) return fail(SLK_E_INVALID, "offsets[0] must be 0");
  for (uint64_t i = 0; i < n_sequences; i++)
    if (offsets[i + 1] < offsets[i]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)i);
  const uint64_t N = offsets[n_sequences];
  if (N == 0) return SLK_OK;
  if (!bases) return fail(SLK_E_INVALID, "null argument");
  if ((rc = set_device(st->ix))) return rc;
  // Batches of B letters, each staged with the window - 1 letters before and behind it: every interval that covers a letter of the
  // batch lies inside what was staged, and whether an interval is perfect depends on its own letters alone.  Only the batch's own
  // letters are rewritten, counted and brought back.
  const uint64_t B = (uint64_t)std::max<long>(env_long("SLK_MASK_BATCH_BASES", 1L << 28), 64), halo = c.window - 1;
  HIPCHK(st->mask_count.ensure(8));
  HIPCHK(st->bases.ensure(std::min(N, B + 2 * halo)));
  DrainOnExit drain(st);
  HIPCHK(hipMemsetAsync(st->mask_count.p, 0, 8, st->s));
  std::vector<uint64_t> local;
  for (uint64_t c0 = 0; c0 < N; c0 += B) {
    const uint64_t c1 = std::min(N, c0 + B), lo = c0 > halo ? c0 - halo : 0, hi = std::min(N, c1 + halo);
    // the sequences that hold a letter of [lo, hi), cut to it
    const uint64_t first = (uint64_t)(std::upper_bound(offsets, offsets + n_sequences + 1, lo) - offsets) - 1;
    local.clear();
    for (uint64_t q = first; q <= n_sequences && (q == first || offsets[q] < hi); q++) local.push_back(std::max(offsets[q], lo) - lo);
    local.push_back(hi - lo);
    HIPCHK(st->offsets.ensure(local.size() * 8));
    rc = copy_in(st, st->bases.p, bases + lo, hi - lo);
    if (!rc) rc = copy_in(st, st->offsets.p, local.data(), local.size() * 8);
    if (!rc) rc = queue_mask(st, st->bases.as<uint8_t>(), st->offsets.as<uint64_t>(), local.size() - 1, hi - lo, c, c0 - lo, c1 - lo, st->mask_count.as<uint64_t>());
    if (!rc) rc = copy_out(st, bases + c0, st->bases.as<uint8_t>() + (c0 - lo), c1 - c0);   // (complete on return: `local` and the staged letters are free again)
    if (rc) return rc;
  }
  return copy_out(st, out_masked, st->mask_count.p, 8);
}

// slk_index_add_sequences with the letters masked first: uploaded once, masked where they lie (the defaults of slk_mask_config unless
// cfg says otherwise) and scanned where they lie.  The caller's letters are not touched.
extern "C" int32_t slk_index_add_sequences_masked(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa,
                                                  uint64_t n_sequences, const slk_mask_config *cfg, uint64_t *out_masked) {
  if (!ix || !st || !offsets || !out_masked || (n_sequences && !taxa)) return fail(SLK_E_INVALID, "null argument");
  *out_masked = 0;
  if (st->ix != ix) return fail(SLK_E_INVALID, "the stream belongs to another index");
  slk_mask_config c;
  int32_t rc = check_mask_config(cfg, &c);
  if (rc) return rc;
  if (offsets[0] != 0) return fail(SLK_E_INVALID, "offsets[0] must be 0");
  for (uint64_t i = 0; i < n_sequences; i++)
    if (offsets[i + 1] < offsets[i]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)i);
  const uint64_t N = offsets[n_sequences];
  if (N == 0) return SLK_OK;
  if (!bases) return fail(SLK_E_INVALID, "null argument");
  if ((rc = set_device(ix))) return rc;
  HIPCHK(st->mask_count.ensure(8));
  HIPCHK(st->bases.ensure(N));
  HIPCHK(st->offsets.ensure((n_sequences + 1) * 8));
  {
    DrainOnExit drain(st);
    HIPCHK(hipMemsetAsync(st->mask_count.p, 0, 8, st->s));
    rc = copy_in(st, st->bases.p, bases, N);
    if (!rc) rc = copy_in(st, st->offsets.p, offsets, (n_sequences + 1) * 8);
    if (!rc) rc = queue_mask(st, st->bases.as<uint8_t>(), st->offsets.as<uint64_t>(), n_sequences, N, c, 0, N, st->mask_count.as<uint64_t>());
    if (!rc) rc = copy_out(st, out_masked, st->mask_count.p, 8);   // (complete on return: the build stream may read the letters)
    if (rc) return rc;
  }
  return slk_index_add_sequences_device(ix, st->bases.as<uint8_t>(), offsets, taxa, n_sequences);
}
