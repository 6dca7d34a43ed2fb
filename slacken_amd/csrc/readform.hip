// readform.hip -- the compact forms of a batch (slk_pipe_submit: slk_reads) expanded on the device into what the classify kernels
// read: u32 lengths (or one length for all) -> u64 offsets, 2-bit codes with a short list of exception words -> ASCII.  gfx950.
//
// Lengths to offsets is count / scan / scatter, as export.hip and textparse.hip do it: a tile's sum, the sums' exclusive scan by ONE
// block, the tile's offsets from its own rank plus the tile's start.  Three launches ordered on the stream; no block waits for
// another inside a kernel.  Ranks inside a block are wave shuffles plus the waves' totals in LDS.
#include "engine.h"

namespace slk {

constexpr int RF_T = 256, RF_PER = 4;

// the exclusive rank of v among the block's threads, and the block's total (lds: RF_T / 64 words)
__device__ __forceinline__ uint64_t rf_block_rank(uint64_t v, uint64_t *lds, uint64_t &block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up((unsigned long long)incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  uint64_t before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < RF_T / 64; w++) { if (w < wave) before += lds[w]; tot += lds[w]; }
  block_total = tot;
  __syncthreads();   // (lds is free again for the caller's next round)
  return before + incl - v;
}

// count: sums[tile] = the lengths of the tile (nothing at or past lengths[n] is read)
__global__ void __launch_bounds__(RF_T) lengths_sums_kernel(const uint32_t *__restrict__ lengths, uint64_t n, uint64_t *__restrict__ sums) {
  __shared__ uint64_t lds[RF_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * READFORM_TILE + (uint64_t)threadIdx.x * RF_PER;
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < RF_PER; j++) if (base + j < n) v += lengths[base + j];
  uint64_t tot;
  (void)rf_block_rank(v, lds, tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
// scan, one block: sums[0 .. nb) -> where each tile starts, sums[nb] = everything; RF_T tiles per round, the carry in a register
__global__ void __launch_bounds__(RF_T) lengths_scan_kernel(uint64_t *__restrict__ sums, uint64_t nb) {
  __shared__ uint64_t lds[RF_T / 64];
  uint64_t carry = 0;
  for (uint64_t b0 = 0; b0 < nb; b0 += RF_T) {
    const uint64_t i = b0 + threadIdx.x;
    const uint64_t v = i < nb ? sums[i] : 0;
    uint64_t tot;
    const uint64_t ex = rf_block_rank(v, lds, tot);
    if (i < nb) sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}
// scatter: out[r] = the lengths before r, out[n] = all of them.  `expect` is the sum the host took when it sized the buffers: the
// lengths lie in memory the caller may (against the contract) have changed since, so no offset leaves [0, expect] -- the kernels
// behind then read inside the buffers whatever they classify --, and a sum that differs raises bit READFORM_STATUS_BIT.
__global__ void __launch_bounds__(RF_T) lengths_fill_kernel(const uint32_t *__restrict__ lengths, uint64_t n, const uint64_t *__restrict__ sums,
                                                            uint64_t *__restrict__ out, uint64_t expect, int32_t *status) {
  __shared__ uint64_t lds[RF_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * READFORM_TILE + (uint64_t)threadIdx.x * RF_PER;
  uint32_t c[RF_PER];
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < RF_PER; j++) { c[j] = base + j < n ? lengths[base + j] : 0u; v += c[j]; }
  uint64_t tot;
  uint64_t at = sums[blockIdx.x] + rf_block_rank(v, lds, tot);
#pragma unroll
  for (int j = 0; j < RF_PER; j++) { if (base + j < n) out[base + j] = at < expect ? at : expect; at += c[j]; }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    out[n] = expect;
    if (sums[gridDim.x] != expect) atomicOr(status, READFORM_STATUS_BIT);
  }
}
// reads that all have `len` bases: out[r] = r * len for r = 0 .. n
__global__ void __launch_bounds__(RF_T) uniform_offsets_kernel(uint32_t len, uint64_t n, uint64_t *__restrict__ out) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (uint64_t)gridDim.x * blockDim.x) out[r] = r * len;
}

void launch_lengths_to_offsets(const uint32_t *lengths, uint64_t n, uint64_t *out, uint64_t *tmp, uint64_t expect, int32_t *status, hipStream_t s) {
  const uint64_t nb = (n + READFORM_TILE - 1) / READFORM_TILE;   // (n >= 1)
  hipLaunchKernelGGL(lengths_sums_kernel, dim3((unsigned)nb), dim3(RF_T), 0, s, lengths, n, tmp);
  hipLaunchKernelGGL(lengths_scan_kernel, dim3(1), dim3(RF_T), 0, s, tmp, nb);
  hipLaunchKernelGGL(lengths_fill_kernel, dim3((unsigned)nb), dim3(RF_T), 0, s, lengths, n, tmp, out, expect, status);
}
void launch_uniform_offsets(uint32_t len, uint64_t n, uint64_t *out, hipStream_t s) {
  const uint64_t blocks = std::min<uint64_t>((n + 1 + RF_T - 1) / RF_T, 256 * 32);
  hipLaunchKernelGGL(uniform_offsets_kernel, dim3((unsigned)blocks), dim3(RF_T), 0, s, len, n, out);
}

// A word of 16 bases as text: "ACGT" by code where the validity bit is set, 'N' elsewhere (kernels.hip: unpack_bases_kernel's layout)
__device__ __forceinline__ uint4 word_text(uint32_t c, uint32_t v) {
  uint32_t o[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    uint32_t x = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int j = 4 * d + b;
      const uint32_t code = (c >> (2 * j)) & 3u;
      const uint32_t ch = ((v >> j) & 1u) ? ((0x54474341u >> (8 * code)) & 0xFFu) : (uint32_t)'N';   // "ACGT"
      x |= ch << (8 * b);
    }
    o[d] = x;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}
// Sparse validity, first pass: words [0, nwords) with every base valid.  One lane per word, one 16-byte store.
__global__ void __launch_bounds__(256) unpack_valid_kernel(const uint32_t *__restrict__ codes, uint64_t nwords, uint8_t *__restrict__ out) {
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * blockDim.x)
    *(uint4 *)(out + w * 16) = word_text(codes[w], 0xFFFFu);
}
// ... second pass, behind the first on the same stream: one lane per exception rewrites its word with the word's own validity bits.
// (A word index at or past nwords writes nothing: the host has checked the list, but it may lie in memory the caller still owns.
//  The bits of a last, partial word past the side's last base land in bytes no read owns.)
__global__ void __launch_bounds__(256) patch_exceptions_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ exc_word,
                                                               const uint16_t *__restrict__ exc_bits, uint64_t n_exc, uint64_t nwords,
                                                               uint8_t *__restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_exc; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w = exc_word[i];
    if (w < nwords) *(uint4 *)(out + w * 16) = word_text(codes[w], exc_bits[i]);
  }
}

void launch_unpack_sparse(const uint32_t *codes, uint64_t nwords, const uint32_t *exc_word, const uint16_t *exc_bits, uint64_t n_exc, uint8_t *out,
                          hipStream_t s) {
  if (nwords == 0) return;
  const uint64_t blocks = std::min<uint64_t>((nwords + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(unpack_valid_kernel, dim3((unsigned)blocks), dim3(256), 0, s, codes, nwords, out);
  if (n_exc == 0) return;
  const uint64_t eblocks = std::min<uint64_t>((n_exc + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(patch_exceptions_kernel, dim3((unsigned)eblocks), dim3(256), 0, s, codes, exc_word, exc_bits, n_exc, nwords, out);
}

}  // namespace slk
