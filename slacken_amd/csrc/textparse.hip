// textparse.hip -- FASTA / FASTQ text parsed on the device: the record rules of FastaTextInput and FastqTextInput
// (S/kmers/input/FileInputs.scala:155-221), which host/seqio.hpp applies byte by byte on the CPU, as byte classification, scans and
// scatters over the raw text.  Both rules are local (seqio.hpp: PlainSegmentParser), so every byte can decide its own fate from a few
// prefix quantities:
//   FASTQ   a line starts at 0 and after every \n, \r\n or lone \r.  Line j starts a record iff its first byte is '@', line j + 2
//           exists and its first byte is '+'; the sequence is line j + 1 verbatim, the title line j after the '@' up to the first space.
//   FASTA   the text is cut at every '>'.  Per byte: g = the last '>' at or before it, t = the last \n or \r at or before it; a byte
//           that is none of the three is KEPT (a nucleotide) iff t > g.  A piece is a record iff a byte of it is kept; the title is
//           what follows its '>' up to the first \n, \r or space.
// Chunks (final = 0): a FASTQ line counts only with its terminator inside the chunk (a \r on the last byte is undecided), a record
// only with lines j .. j + 2 present; a FASTA record only when the '>' that ends it is inside the chunk.  `consumed` is where the
// caller's next chunk starts.
//
// Layout (textlines.h holds the tile helpers, the scans and the line-start passes, which compare.hip runs too).  A TILE is TP_TILE = 4096 bytes: a block of 256 lanes, 16 bytes per lane in one load (the text must be 16-byte aligned; the
// bytes past n are never read: a lane whose 16 bytes cross n assembles them from byte loads).  Inside a block, ranks are wave scans
// (shuffles; ballots and mbcnt where a lane holds one flag) and four wave totals in LDS.  Across blocks every quantity takes the
// count / scan / scatter shape of export.hip: a pass leaves one number per tile, one block scans the tiles' numbers, the next pass
// reads its tile's carry.  No block waits for another inside a kernel.
//   FASTQ   lines<0> counts the tiles' line starts | scan | lines<1> writes the line starts S[] | records<0> flags the record lines
//           (one lane per line: the first bytes of lines j and j + 2) and sums records and sequence bytes per 256 lines | scan |
//           records<1> writes offsets, titles and where every line's bytes go | copy: every byte finds its line and moves itself.
//   FASTA   stage 0 leaves the tiles' last '>' and last terminator | max-scan | stage 1 the tiles' kept bytes | scan | stage 2 the
//           tiles' records (a '>' -- or the end of the final chunk -- closes a record iff a byte was kept since the '>' before) |
//           scan | stage 3 moves the kept bytes and writes offsets and titles.
// A record of any length is spread over as many lanes as it has bytes.  What stays serial is the walk along a TITLE to its first
// space, one lane per record.
// Scratch is sized from n alone (FASTQ: 8 bytes per byte of text for the line starts and the lines' destinations, every byte may be
// a line; FASTA: 20 bytes per tile), kept on the stream and grown like its other buffers.
// Two mate texts (slk_pair_device, slk_parse_text_paired): both are parsed as above, text 2 into the stream's mate
// buffers, then a compare pass (one lane per record: titles stripped of "/1" and "/2" and compared, a ballot and one atomicMin per wave)
// and a one-lane finish pass leave the pair record: how many leading records are mates and where either text's next chunk starts.
#include "textlines.h"

namespace {

// The layout's constants under the names this file's kernels use; textlines.h has them as TL_* for the passes it holds.
constexpr int TP_BLOCK = 256;
constexpr int TP_LANE_BYTES = 16;
constexpr uint32_t TP_TILE = TP_BLOCK * TP_LANE_BYTES;
constexpr int TP_SCAN_BLOCK = 1024;
constexpr unsigned TP_MAX_GRID = 2048;   // 256 CUs x 8 blocks; the kernels stride over their tiles
constexpr uint32_t TP_NONE = 0xFFFFFFFFu;
static_assert(TP_BLOCK == TL_BLOCK && TP_LANE_BYTES == TL_LANE_BYTES && TP_TILE == TL_TILE && TP_SCAN_BLOCK == TL_SCAN_BLOCK && TP_MAX_GRID == TL_MAX_GRID,
              "textparse.hip and textlines.h describe one layout");

// ---- FASTQ --------------------------------------------------------------------------------------------------------------------

// One lane per line.  WRITE = 0: the records and sequence bytes of every 256 lines.  WRITE = 1 (those scanned): offsets, titles, the
// lines' destinations and the counts record.
template <int WRITE>
__global__ void __launch_bounds__(TP_BLOCK) fq_records_kernel(TpArgs A) {
  __shared__ uint32_t lds[TP_BLOCK / 64];
  const uint32_t M = A.tiles[A.ntiles];   // lines that start inside the text (>= 1: n > 0)
  // lines that are PRESENT: all of a final chunk; otherwise those whose terminator is inside and decided
  const uint32_t Lp = A.final ? M : (A.text[A.n - 1] == '\n' ? M : M - 1);
  const uint32_t nlt = (M + TP_BLOCK - 1) / TP_BLOCK;
  uint32_t *lt_rec = A.ltiles, *lt_bases = A.ltiles + (A.nlt_max + 1);
  bool over = false;
  if (WRITE) over = lt_rec[nlt] > A.records_capacity || lt_bases[nlt] > A.bases_capacity;
  for (uint32_t lt = blockIdx.x; lt < nlt; lt += gridDim.x) {
    const uint64_t j = (uint64_t)lt * TP_BLOCK + threadIdx.x;
    bool rec = false;
    uint32_t s0 = 0, s1 = 0, len = 0;
    if (j + 2 < Lp) {
      s0 = A.S[j];
      const uint32_t s2 = A.S[j + 2];
      if (A.text[s0] == '@' && A.text[s2] == '+') {
        rec = true;
        s1 = A.S[j + 1];
        len = fq_line_end(A.text, s1, s2) - s1;
      }
    }
    // a lane holds one flag: its rank in the wave is a ballot and mbcnt; the waves' totals pass through LDS
    const unsigned long long ballot = __ballot(rec);
    const uint32_t rank_w = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t rank = rank_w, rec_total = 0;
#pragma unroll
    for (int i = 0; i < TP_BLOCK / 64; i++) {
      if (i < (int)(threadIdx.x >> 6)) rank += lds[i];
      rec_total += lds[i];
    }
    __syncthreads();
    uint32_t len_total;
    const uint32_t len_excl = tp_block_excl<false>(len, lds, len_total);
    if (!WRITE) {
      if (threadIdx.x == 0) { lt_rec[lt] = rec_total; lt_bases[lt] = len_total; }
      continue;
    }
    const uint32_t r = lt_rec[lt] + rank, d = lt_bases[lt] + len_excl;
    if (j < M) A.dst[j + 1] = rec && !over ? d : TP_NONE;   // (line j + 1 is the sequence of the record line j starts)
    if (j == 0) A.dst[0] = TP_NONE;
    if (rec && !over) {
      const uint32_t e0 = fq_line_end(A.text, s0, s1);
      uint32_t q = s0 + 1;
      while (q < e0 && A.text[q] != ' ') q++;
      A.offsets[r] = d;
      A.title_pos[r] = (uint64_t)s0 + 1;
      A.title_len[r] = q - (s0 + 1);
    }
  }
  if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) {
    if (!over) A.offsets[lt_rec[nlt]] = lt_bases[nlt];
    A.counts[0] = lt_rec[nlt];
    A.counts[1] = lt_bases[nlt];
    // the first line whose window could not be decided: the last but one that is present
    A.counts[2] = over ? 0 : A.final ? A.n : (Lp >= 2 ? A.S[Lp - 2] : 0);
    A.counts[3] = over ? 1 : 0;
  }
}

// every byte of a sequence line to its place in `bases`: the byte's line is the rank of the last line start at or before it
__global__ void __launch_bounds__(TP_BLOCK) fq_copy_kernel(TpArgs A) {
  __shared__ uint32_t lds[TP_BLOCK / 64];
  const uint32_t M = A.tiles[A.ntiles];
  const uint32_t nlt = (M + TP_BLOCK - 1) / TP_BLOCK;
  if (A.ltiles[nlt] > A.records_capacity || A.ltiles[A.nlt_max + 1 + nlt] > A.bases_capacity) return;   // overflow: nothing is written
  for (uint32_t t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
    const uint64_t p = (uint64_t)t * TP_TILE + threadIdx.x * TP_LANE_BYTES;
    uint32_t w[4];
    tp_load16(A.text, A.n, p, w);
    const uint32_t mask = fq_start_mask(A, p, w);
    uint32_t total;
    const uint32_t excl = tp_block_excl<false>(__popc(mask), lds, total);
    if (p >= A.n) continue;
    uint32_t line = A.tiles[t] + excl;   // line starts before p; position 0 is one, so the line of p + k is (starts <= p + k) - 1
    uint32_t d = TP_NONE, s = 0;
    if (!(mask & 1u)) { d = A.dst[line - 1]; s = A.S[line - 1]; }
#pragma unroll
    for (int k = 0; k < TP_LANE_BYTES; k++) {
      if (p + k >= A.n) continue;
      if (mask & (1u << k)) { d = A.dst[line]; s = A.S[line]; line++; }
      const uint32_t c = tp_byte(w, k);
      if (d != TP_NONE && c != '\n' && c != '\r') {
        const uint64_t at = (uint64_t)d + ((uint32_t)(p + k) - s);
        if (at < A.bases_capacity) A.bases[at] = (uint8_t)c;
      }
    }
  }
}

// ---- FASTA --------------------------------------------------------------------------------------------------------------------
// Positions travel as pos + 1 in 32 bits, 0 = none: the max-scans' neutral element.  tiles: five arrays of ntiles + 1 --
// [0] last '>', [1] last terminator, [2] kept bytes, [3] last kept byte, [4] records.
// STAGE 0: arrays 0, 1.  STAGE 1 (0, 1 scanned): arrays 2, 3.  STAGE 2 (2, 3 scanned): array 4.  STAGE 3 (4 scanned): the output.
template <int STAGE>
__global__ void __launch_bounds__(TP_BLOCK) fa_kernel(TpArgs A) {
  __shared__ uint32_t lds[TP_BLOCK / 64];
  const uint64_t stride = (uint64_t)A.ntiles + 1;
  uint32_t *t_gt = A.tiles, *t_tm = A.tiles + stride, *t_kept = A.tiles + 2 * stride, *t_lk = A.tiles + 3 * stride, *t_rec = A.tiles + 4 * stride;
  // Bytes are kept below `limit`: the end of a final chunk; else the last '>' of the chunk, which opens the first record not taken
  // (no '>' at all: nothing is taken).
  uint64_t limit = A.n;
  if (STAGE >= 1 && !A.final) limit = t_gt[A.ntiles] ? t_gt[A.ntiles] - 1 : 0;
  bool over = false;
  if (STAGE == 3) over = t_rec[A.ntiles] > A.records_capacity || t_kept[A.ntiles] > A.bases_capacity;
  for (uint32_t t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
    const uint64_t p = (uint64_t)t * TP_TILE + threadIdx.x * TP_LANE_BYTES;
    uint32_t w[4];
    tp_load16(A.text, A.n, p, w);
    uint32_t m_gt = 0, m_tm = 0, m_other = 0;
#pragma unroll
    for (int k = 0; k < TP_LANE_BYTES; k++) {
      const uint32_t c = tp_byte(w, k);
      if (p + k >= A.n) continue;
      if (c == '>') m_gt |= 1u << k;
      else if (c == '\n' || c == '\r') m_tm |= 1u << k;
      else m_other |= 1u << k;
    }
    const uint32_t P1 = (uint32_t)p + 1;   // (only used where the lane holds a byte below n: no wrap)
    uint32_t tot_gt, tot_tm;
    uint32_t lg = tp_block_excl<true>(m_gt ? P1 + tp_top(m_gt) : 0, lds, tot_gt);
    uint32_t lt = tp_block_excl<true>(m_tm ? P1 + tp_top(m_tm) : 0, lds, tot_tm);
    if (STAGE == 0) {
      if (threadIdx.x == 0) { t_gt[t] = tot_gt; t_tm[t] = tot_tm; }
      continue;
    }
    lg = max(lg, t_gt[t]);   // the last '>' and the last terminator before the lane's bytes
    lt = max(lt, t_tm[t]);
    // the kept bytes: neither '>' nor a terminator, a terminator since the last '>', below the limit
    uint32_t m_keep = 0;
    {
      uint32_t g = lg, x = lt;
#pragma unroll
      for (int k = 0; k < TP_LANE_BYTES; k++) {
        if (m_gt & (1u << k)) g = P1 + k;
        else if (m_tm & (1u << k)) x = P1 + k;
        else if ((m_other & (1u << k)) && x > g && p + k < limit) m_keep |= 1u << k;
      }
    }
    uint32_t tot_kept, tot_lk;
    uint32_t K = tp_block_excl<false>(__popc(m_keep), lds, tot_kept);
    uint32_t lk = tp_block_excl<true>(m_keep ? P1 + tp_top(m_keep) : 0, lds, tot_lk);
    if (STAGE == 1) {
      if (threadIdx.x == 0) { t_kept[t] = tot_kept; t_lk[t] = tot_lk; }
      continue;
    }
    K += t_kept[t];           // kept bytes before the lane's
    lk = max(lk, t_lk[t]);    // the last of them
    // what closes a piece: every '>', and the end of a final chunk (position n).  It closes a RECORD iff a byte was kept since the
    // '>' before it.
    uint32_t m_mark = m_gt;
    if (A.final && A.n >= p && A.n < p + TP_LANE_BYTES) m_mark |= 1u << (int)(A.n - p);
    uint32_t m_emit = 0;
    for (uint32_t m = m_mark; m; m &= m - 1) {
      const int k = __ffs((int)m) - 1;
      const uint32_t gb = tp_below(m_gt, k), kb = tp_below(m_keep, k);
      const uint32_t g = gb ? P1 + tp_top(gb) : lg, kk = kb ? P1 + tp_top(kb) : lk;
      if (kk > g) m_emit |= 1u << k;
    }
    uint32_t tot_rec;
    uint32_t r = tp_block_excl<false>(__popc(m_emit), lds, tot_rec);
    if (STAGE == 2) {
      if (threadIdx.x == 0) t_rec[t] = tot_rec;
      continue;
    }
    if (over) continue;
    r += t_rec[t];
    for (uint32_t m = m_keep; m; m &= m - 1) {
      const int k = __ffs((int)m) - 1;
      const uint64_t at = (uint64_t)K + __popc(tp_below(m_keep, k));
      if (at < A.bases_capacity) A.bases[at] = (uint8_t)tp_byte(w, k);
    }
    for (uint32_t m = m_emit; m; m &= m - 1, r++) {
      const int k = __ffs((int)m) - 1;
      const uint32_t gb = tp_below(m_gt, k);
      const uint64_t start = gb ? (uint64_t)p + tp_top(gb) + 1 : lg;   // behind the '>' that opens the record; 0: the text's first piece
      uint64_t q = start;
      while (q < p + k) {
        const uint8_t c = A.text[q];
        if (c == ' ' || c == '\n' || c == '\r') break;
        q++;
      }
      if (r < A.records_capacity) {
        A.offsets[r + 1] = (uint64_t)K + __popc(tp_below(m_keep, k));   // where record r ends = where record r + 1 starts
        A.title_pos[r] = start;
        A.title_len[r] = (uint32_t)(q - start);
      }
    }
  }
  if (STAGE == 3 && blockIdx.x == 0 && threadIdx.x == 0) {
    if (!over) A.offsets[0] = 0;
    A.counts[0] = t_rec[A.ntiles];
    A.counts[1] = t_kept[A.ntiles];
    A.counts[2] = over ? 0 : A.final ? A.n : limit;
    A.counts[3] = over ? 1 : 0;
  }
}

// an empty text: no record, nothing consumed
__global__ void tp_empty_kernel(uint64_t *offsets, uint64_t *counts) {
  offsets[0] = 0;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------
// Two parsed texts paired in lockstep (PairedInputReader.getFragments, S/kmers/input/InputReader.scala:105-131, while both files list
// their mates in the same order): record i of text 1 and record i of text 2 are mates iff their titles are equal once ONE trailing
// "/1" is taken off the first and ONE trailing "/2" off the second.  P = the leading records for which that holds.
struct PairArgs {
  const uint8_t *text1, *text2;
  uint64_t n1, n2;
  const uint64_t *title_pos1, *title_pos2;
  uint32_t *title_len1;          // rewritten: every record of text 1 loses its "/1"
  const uint32_t *title_len2;
  const uint64_t *offsets1, *offsets2, *counts1, *counts2;
  uint64_t R1, R2;
  unsigned long long *pair;      // the pair record; word 0 is the first differing index while the compare pass runs
};

// a title as the parser left it, held inside text[0, n); without one trailing '/' d
__device__ __forceinline__ void pt_title(const uint8_t *text, uint64_t n, uint64_t pos, uint32_t len, uint8_t d, uint64_t &p, uint32_t &l) {
  p = umin64(pos, n);
  l = (uint32_t)umin64(len, n - p);
  if (l >= 2 && text[p + l - 2] == '/' && text[p + l - 1] == d) l -= 2;
}
// One lane per record of text 1: it strips its title and, below min(R1, R2), compares it with its mate's.  A wave finds its first
// differing lane with a ballot and sends one atomicMin.
__global__ void __launch_bounds__(TP_BLOCK) pt_compare_kernel(PairArgs A) {
  const uint64_t M = umin64(A.R1, A.R2);
  for (uint64_t base = (uint64_t)blockIdx.x * TP_BLOCK; base < A.R1; base += (uint64_t)gridDim.x * TP_BLOCK) {
    const uint64_t i = base + threadIdx.x;
    bool differ = false;
    if (i < A.R1) {
      const uint32_t len1 = A.title_len1[i];
      uint64_t p1;
      uint32_t l1;
      pt_title(A.text1, A.n1, A.title_pos1[i], len1, '1', p1, l1);
      if (i < M) {
        uint64_t p2;
        uint32_t l2;
        pt_title(A.text2, A.n2, A.title_pos2[i], A.title_len2[i], '2', p2, l2);
        differ = l1 != l2 || !pt_equal(A.text1 + p1, A.text2 + p2, l1);
      }
      if (l1 != len1) A.title_len1[i] = l1;
    }
    const unsigned long long ballot = __ballot(differ);
    if (ballot && (threadIdx.x & 63) == 0) atomicMin(A.pair, (unsigned long long)(i + (__ffsll(ballot) - 1)));
  }
}

// the byte that opens the record whose title starts at pos: the '@' or '>' before it, or 0 for a FASTA record that opens the text bare
__device__ __forceinline__ uint64_t pt_opener(uint64_t pos) { return pos ? pos - 1 : 0; }

__global__ void pt_finish_kernel(PairArgs A) {
  const uint64_t M = umin64(A.R1, A.R2), P = umin64(A.pair[0], M);
  A.pair[0] = P;
  A.pair[1] = P < M ? 1 : 0;
  A.pair[2] = A.R1 > P ? pt_opener(A.title_pos1[P]) : A.counts1[2];
  A.pair[3] = A.R2 > P ? pt_opener(A.title_pos2[P]) : A.counts2[2];
  A.pair[4] = A.R1;
  A.pair[5] = A.R2;
  A.pair[6] = A.offsets1[P];
  A.pair[7] = A.offsets2[P];
}

}  // namespace

namespace slk {

// The passes of one parse, queued on the stream's HIP stream.  All pointers on the device; d_offsets holds records_capacity + 1.
int32_t launch_parse(slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t format, bool final, uint8_t *d_bases, uint64_t bases_capacity,
                     uint64_t *d_offsets, uint64_t *d_title_pos, uint32_t *d_title_len, uint64_t records_capacity, uint64_t *d_counts) {
  hipStream_t s = st->s;
  if (n == 0) {
    hipLaunchKernelGGL(tp_empty_kernel, dim3(1), dim3(1), 0, s, d_offsets, d_counts);
    HIPCHK(hipGetLastError());
    return SLK_OK;
  }
  const bool fastq = format == SLK_FORMAT_FASTQ;
  TpArgs A{};
  A.text = d_text;
  A.n = n;
  A.final = final ? 1 : 0;
  A.ntiles = (uint32_t)(((fastq || !final ? n : n + 1) + TP_TILE - 1) / TP_TILE);
  A.nlt_max = (uint32_t)(n / TP_BLOCK + 1);
  // scratch, in words: the tiles' arrays, then (FASTQ) the line starts, the lines' destinations and the line tiles' two arrays
  const uint64_t tile_words = (fastq ? 1 : 5) * ((uint64_t)A.ntiles + 1);
  const uint64_t words = tile_words + (fastq ? 2 * (n + 2) + 2 * ((uint64_t)A.nlt_max + 1) : 0);
  HIPCHK(st->parse_scratch.ensure(words * 4));
  A.tiles = st->parse_scratch.as<uint32_t>();
  A.S = A.tiles + tile_words;
  A.dst = A.S + (n + 2);
  A.ltiles = A.dst + (n + 2);
  A.bases = d_bases; A.bases_capacity = bases_capacity;
  A.offsets = d_offsets; A.title_pos = d_title_pos; A.title_len = d_title_len; A.records_capacity = records_capacity;
  A.counts = d_counts;
  const dim3 grid(std::min<unsigned>(A.ntiles, TP_MAX_GRID)), block(TP_BLOCK);
  if (fastq) {
    const dim3 lgrid(std::min<unsigned>(A.nlt_max, TP_MAX_GRID));
    hipLaunchKernelGGL(fq_lines_kernel<0>, grid, block, 0, s, A);
    hipLaunchKernelGGL(tp_scan_kernel, dim3(1), dim3(TP_SCAN_BLOCK), 0, s, A.tiles, (uint64_t)0, A.ntiles, (const uint32_t *)nullptr, 1u, 0u);
    hipLaunchKernelGGL(fq_lines_kernel<1>, grid, block, 0, s, A);
    hipLaunchKernelGGL(fq_records_kernel<0>, lgrid, block, 0, s, A);
    hipLaunchKernelGGL(tp_scan_kernel, dim3(2), dim3(TP_SCAN_BLOCK), 0, s, A.ltiles, (uint64_t)A.nlt_max + 1, 0u, (const uint32_t *)(A.tiles + A.ntiles),
                       (uint32_t)TP_BLOCK, 0u);
    hipLaunchKernelGGL(fq_records_kernel<1>, lgrid, block, 0, s, A);
    hipLaunchKernelGGL(fq_copy_kernel, grid, block, 0, s, A);
  } else {
    const uint64_t stride = (uint64_t)A.ntiles + 1;
    hipLaunchKernelGGL(fa_kernel<0>, grid, block, 0, s, A);
    hipLaunchKernelGGL(tp_scan_kernel, dim3(2), dim3(TP_SCAN_BLOCK), 0, s, A.tiles, stride, A.ntiles, (const uint32_t *)nullptr, 1u, 3u);
    hipLaunchKernelGGL(fa_kernel<1>, grid, block, 0, s, A);
    hipLaunchKernelGGL(tp_scan_kernel, dim3(2), dim3(TP_SCAN_BLOCK), 0, s, A.tiles + 2 * stride, stride, A.ntiles, (const uint32_t *)nullptr, 1u, 2u);
    hipLaunchKernelGGL(fa_kernel<2>, grid, block, 0, s, A);
    hipLaunchKernelGGL(tp_scan_kernel, dim3(1), dim3(TP_SCAN_BLOCK), 0, s, A.tiles + 4 * stride, stride, A.ntiles, (const uint32_t *)nullptr, 1u, 0u);
    hipLaunchKernelGGL(fa_kernel<3>, grid, block, 0, s, A);
  }
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

int32_t check_parse_args(uint64_t n, int32_t format) {
  if (format != SLK_FORMAT_FASTA && format != SLK_FORMAT_FASTQ) return fail(SLK_E_INVALID, "format %d is neither SLK_FORMAT_FASTA nor SLK_FORMAT_FASTQ", format);
  if (n >= (1ULL << 32)) return fail(SLK_E_INVALID, "a parse call takes less than 2^32 bytes of text (%llu given): cut it into chunks", (unsigned long long)n);
  return SLK_OK;
}

// text -> the stream's text buffer; parsed into the stream's read buffers (bases, offsets) and title buffers; the counts record to
// the host.  Synchronises st->s.  counts: records, bases, consumed, overflow.
int32_t parse_uploaded(slk_stream *st, const uint8_t *text, uint64_t n, int32_t format, bool final, uint64_t bases_capacity,
                       uint64_t records_capacity, uint64_t counts[4]) {
  HIPCHK(st->parse_text.ensure(std::max<uint64_t>(n, 16)));
  HIPCHK(st->bases.ensure(std::max<uint64_t>(bases_capacity, 16)));
  HIPCHK(st->offsets.ensure((records_capacity + 1) * 8));
  HIPCHK(st->parse_title_pos.ensure(std::max<uint64_t>(records_capacity, 1) * 8));
  HIPCHK(st->parse_title_len.ensure(std::max<uint64_t>(records_capacity, 1) * 4));
  HIPCHK(st->parse_counts.ensure(4 * 8));
  int32_t rc = copy_in(st, st->parse_text.p, text, n);
  if (rc) return rc;
  rc = launch_parse(st, st->parse_text.as<uint8_t>(), n, format, final, st->bases.as<uint8_t>(), bases_capacity, st->offsets.as<uint64_t>(),
                    st->parse_title_pos.as<uint64_t>(), st->parse_title_len.as<uint32_t>(), records_capacity, st->parse_counts.as<uint64_t>());
  if (rc) return rc;
  rc = copy_out(st, counts, st->parse_counts.p, 4 * 8);
  if (rc) return rc;
  if (counts[3])
    return fail(SLK_E_CAPACITY, "the text holds %llu records of %llu bases, the capacities are %llu and %llu", (unsigned long long)counts[0],
                (unsigned long long)counts[1], (unsigned long long)records_capacity, (unsigned long long)bases_capacity);
  return SLK_OK;
}

// the compare and finish passes over the outputs of two parses, queued on the stream
static int32_t launch_pair(slk_stream *st, const PairArgs &A) {
  hipStream_t s = st->s;
  HIPCHK(hipMemsetAsync(A.pair, 0xFF, 8, s));   // (no differing index yet: the finish pass takes the smaller of this word and min(R1, R2))
  if (A.R1) {
    const unsigned blocks = (unsigned)std::min<uint64_t>((A.R1 + TP_BLOCK - 1) / TP_BLOCK, TP_MAX_GRID);
    hipLaunchKernelGGL(pt_compare_kernel, dim3(blocks), dim3(TP_BLOCK), 0, s, A);
  }
  hipLaunchKernelGGL(pt_finish_kernel, dim3(1), dim3(1), 0, s, A);
  HIPCHK(hipGetLastError());
  return SLK_OK;
}

static uint64_t parse_scratch_bytes(uint64_t n, int32_t format, bool final) {   // what launch_parse will ask of parse_scratch
  const bool fastq = format == SLK_FORMAT_FASTQ;
  const uint64_t ntiles = ((fastq || !final ? n : n + 1) + TP_TILE - 1) / TP_TILE, nlt_max = n / TP_BLOCK + 1;
  return 4 * ((fastq ? 1 : 5) * (ntiles + 1) + (fastq ? 2 * (n + 2) + 2 * (nlt_max + 1) : 0));
}

int32_t parse_pair_uploaded(slk_stream *st, const PairText &t1, const PairText &t2, uint64_t pair[8]) {
  // every buffer at its size before the first launch: growing one frees it, and that waits for the device
  HIPCHK(st->parse_text.ensure(std::max<uint64_t>(t1.n, 16)));
  HIPCHK(st->parse_text2.ensure(std::max<uint64_t>(t2.n, 16)));
  HIPCHK(st->bases.ensure(std::max<uint64_t>((t1.bases_capacity + 15) / 16 * 16, 16)));
  HIPCHK(st->mate_bases.ensure(std::max<uint64_t>((t2.bases_capacity + 15) / 16 * 16, 16)));
  HIPCHK(st->offsets.ensure((t1.records_capacity + 1) * 8));
  HIPCHK(st->mate_offsets.ensure((t2.records_capacity + 1) * 8));
  HIPCHK(st->parse_title_pos.ensure(std::max<uint64_t>(t1.records_capacity, 1) * 8));
  HIPCHK(st->parse_title_len.ensure(std::max<uint64_t>(t1.records_capacity, 1) * 4));
  HIPCHK(st->parse_title_pos2.ensure(std::max<uint64_t>(t2.records_capacity, 1) * 8));
  HIPCHK(st->parse_title_len2.ensure(std::max<uint64_t>(t2.records_capacity, 1) * 4));
  HIPCHK(st->parse_counts.ensure(8 * 8));
  HIPCHK(st->parse_pair.ensure(8 * 8));
  HIPCHK(st->parse_scratch.ensure(std::max(parse_scratch_bytes(t1.n, t1.format, t1.final), parse_scratch_bytes(t2.n, t2.format, t2.final))));
  uint64_t *const d_counts = st->parse_counts.as<uint64_t>();
  int32_t rc = copy_in(st, st->parse_text.p, t1.text, t1.n);
  if (!rc) rc = copy_in(st, st->parse_text2.p, t2.text, t2.n);
  // (the two parses share parse_scratch: one after the other on the stream)
  if (!rc)
    rc = launch_parse(st, st->parse_text.as<uint8_t>(), t1.n, t1.format, t1.final, st->bases.as<uint8_t>(), t1.bases_capacity, st->offsets.as<uint64_t>(),
                      st->parse_title_pos.as<uint64_t>(), st->parse_title_len.as<uint32_t>(), t1.records_capacity, d_counts);
  if (!rc)
    rc = launch_parse(st, st->parse_text2.as<uint8_t>(), t2.n, t2.format, t2.final, st->mate_bases.as<uint8_t>(), t2.bases_capacity,
                      st->mate_offsets.as<uint64_t>(), st->parse_title_pos2.as<uint64_t>(), st->parse_title_len2.as<uint32_t>(), t2.records_capacity,
                      d_counts + 4);
  uint64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!rc) rc = copy_out(st, counts, d_counts, 8 * 8);
  if (rc) return rc;
  if (counts[3] || counts[7]) {
    pair[4] = counts[0]; pair[5] = counts[4]; pair[6] = counts[1]; pair[7] = counts[5];
    return fail(SLK_E_CAPACITY, "the texts hold %llu records of %llu bases and %llu records of %llu bases, the capacities are %llu, %llu and %llu, %llu",
                (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[4], (unsigned long long)counts[5],
                (unsigned long long)t1.records_capacity, (unsigned long long)t1.bases_capacity, (unsigned long long)t2.records_capacity,
                (unsigned long long)t2.bases_capacity);
  }
  PairArgs A{};
  A.text1 = st->parse_text.as<uint8_t>(); A.text2 = st->parse_text2.as<uint8_t>();
  A.n1 = t1.n; A.n2 = t2.n;
  A.title_pos1 = st->parse_title_pos.as<uint64_t>(); A.title_pos2 = st->parse_title_pos2.as<uint64_t>();
  A.title_len1 = st->parse_title_len.as<uint32_t>(); A.title_len2 = st->parse_title_len2.as<uint32_t>();
  A.offsets1 = st->offsets.as<uint64_t>(); A.offsets2 = st->mate_offsets.as<uint64_t>();
  A.counts1 = d_counts; A.counts2 = d_counts + 4;
  A.R1 = counts[0]; A.R2 = counts[4];
  A.pair = st->parse_pair.as<unsigned long long>();
  rc = launch_pair(st, A);
  if (!rc) rc = copy_out(st, pair, st->parse_pair.p, 8 * 8);
  return rc;
}

}  // namespace slk

extern "C" uint32_t slk_parse_tile_bytes(void) { return TP_TILE; }

extern "C" int32_t slk_parse_device(slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t format, int32_t final, uint8_t *d_bases,
                                    uint64_t bases_capacity, uint64_t *d_offsets, uint64_t *d_title_pos, uint32_t *d_title_len,
                                    uint64_t records_capacity, uint64_t *d_counts) {
  if (!st || !d_offsets || !d_counts || (n && !d_text) || (bases_capacity && !d_bases) || (records_capacity && (!d_title_pos || !d_title_len)))
    return fail(SLK_E_INVALID, "null argument");
  int32_t rc = check_parse_args(n, format);
  if (rc) return rc;
  if ((uintptr_t)d_text % TP_LANE_BYTES) return fail(SLK_E_INVALID, "d_text must be aligned to %d bytes", TP_LANE_BYTES);
  if ((rc = set_device(st->ix))) return rc;
  return launch_parse(st, d_text, n, format, final != 0, d_bases, bases_capacity, d_offsets, d_title_pos, d_title_len, records_capacity, d_counts);
}

extern "C" int32_t slk_parse_text(slk_stream *st, const uint8_t *text, uint64_t n, int32_t format, int32_t final, uint8_t *out_bases,
                                  uint64_t *out_offsets, uint64_t *out_title_pos, uint32_t *out_title_len, uint64_t bases_capacity,
                                  uint64_t records_capacity, uint64_t *out_records, uint64_t *out_n_bases, uint64_t *out_consumed) {
  if (!st || !out_offsets || !out_records || !out_n_bases || !out_consumed || (n && !text) || (bases_capacity && !out_bases) ||
      (records_capacity && (!out_title_pos || !out_title_len)))
    return fail(SLK_E_INVALID, "null argument");
  *out_records = *out_n_bases = *out_consumed = 0;
  int32_t rc = check_parse_args(n, format);
  if (rc) return rc;
  if ((rc = set_device(st->ix))) return rc;
  DrainOnExit drain(st);
  uint64_t counts[4] = {0, 0, 0, 0};
  rc = parse_uploaded(st, text, n, format, final != 0, bases_capacity, records_capacity, counts);
  *out_records = counts[0];   // (with SLK_E_CAPACITY too: what the capacities would have to be)
  *out_n_bases = counts[1];
  if (rc) return rc;
  *out_consumed = counts[2];
  const uint64_t R = counts[0];
  rc = copy_out(st, out_offsets, st->offsets.p, (R + 1) * 8);
  if (!rc) rc = copy_out(st, out_bases, st->bases.p, counts[1]);
  if (!rc) rc = copy_out(st, out_title_pos, st->parse_title_pos.p, R * 8);
  if (!rc) rc = copy_out(st, out_title_len, st->parse_title_len.p, R * 4);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st->s));
  return SLK_OK;
}

extern "C" int32_t slk_pair_device(slk_stream *st, const uint8_t *d_text1, uint64_t n1, const uint64_t *d_title_pos1, uint32_t *d_title_len1,
                                   const uint64_t *d_offsets1, const uint64_t *d_counts1, uint64_t R1, const uint8_t *d_text2, uint64_t n2,
                                   const uint64_t *d_title_pos2, const uint32_t *d_title_len2, const uint64_t *d_offsets2,
                                   const uint64_t *d_counts2, uint64_t R2, uint64_t *d_pair) {
  if (!st || !d_offsets1 || !d_offsets2 || !d_counts1 || !d_counts2 || !d_pair || (R1 && (!d_text1 || !d_title_pos1 || !d_title_len1)) ||
      (R2 && (!d_text2 || !d_title_pos2 || !d_title_len2)))
    return fail(SLK_E_INVALID, "null argument");
  if (n1 >= (1ULL << 32) || n2 >= (1ULL << 32)) return fail(SLK_E_INVALID, "a paired call takes less than 2^32 bytes of either text");
  int32_t rc = set_device(st->ix);
  if (rc) return rc;
  PairArgs A{};
  A.text1 = d_text1; A.text2 = d_text2; A.n1 = n1; A.n2 = n2;
  A.title_pos1 = d_title_pos1; A.title_pos2 = d_title_pos2; A.title_len1 = d_title_len1; A.title_len2 = d_title_len2;
  A.offsets1 = d_offsets1; A.offsets2 = d_offsets2; A.counts1 = d_counts1; A.counts2 = d_counts2;
  A.R1 = R1; A.R2 = R2;
  A.pair = (unsigned long long *)d_pair;
  return launch_pair(st, A);
}

extern "C" int32_t slk_parse_text_paired(slk_stream *st, const uint8_t *text1, uint64_t n1, int32_t format1, int32_t final1, const uint8_t *text2,
                                         uint64_t n2, int32_t format2, int32_t final2, uint8_t *out_bases, uint64_t *out_offsets,
                                         uint8_t *out_mate_bases, uint64_t *out_mate_offsets, uint64_t *out_title_pos, uint32_t *out_title_len,
                                         uint64_t bases_capacity1, uint64_t records_capacity1, uint64_t bases_capacity2,
                                         uint64_t records_capacity2, slk_pair_record *out_pair) {
  if (!st || !out_offsets || !out_mate_offsets || !out_pair || (n1 && !text1) || (n2 && !text2) || (bases_capacity1 && !out_bases) ||
      (bases_capacity2 && !out_mate_bases) || (records_capacity1 && (!out_title_pos || !out_title_len)))
    return fail(SLK_E_INVALID, "null argument");
  uint64_t pair[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(out_pair, pair, sizeof(pair));
  int32_t rc = check_parse_args(n1, format1);
  if (!rc) rc = check_parse_args(n2, format2);
  if (rc) return rc;
  if ((rc = set_device(st->ix))) return rc;
  DrainOnExit drain(st);
  rc = parse_pair_uploaded(st, PairText{text1, n1, format1, final1 != 0, bases_capacity1, records_capacity1},
                           PairText{text2, n2, format2, final2 != 0, bases_capacity2, records_capacity2}, pair);
  memcpy(out_pair, pair, sizeof(pair));   // (with SLK_E_CAPACITY too: what the capacities would have to be)
  if (rc) return rc;
  const uint64_t P = pair[0], R1 = pair[4];
  rc = copy_out(st, out_offsets, st->offsets.p, (P + 1) * 8);
  if (!rc) rc = copy_out(st, out_mate_offsets, st->mate_offsets.p, (P + 1) * 8);
  if (!rc) rc = copy_out(st, out_bases, st->bases.p, pair[6]);
  if (!rc) rc = copy_out(st, out_mate_bases, st->mate_bases.p, pair[7]);
  if (!rc) rc = copy_out(st, out_title_pos, st->parse_title_pos.p, R1 * 8);
  if (!rc) rc = copy_out(st, out_title_len, st->parse_title_len.p, R1 * 4);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st->s));
  return SLK_OK;
}
