// export.hip -- a bucket range of a resident table as records that arrive grouped by Spark's bucket: the device half of
// KeyValueIndex.writeRecords (S/slacken/KeyValueIndex.scala:125-139), which persists the records as a table CLUSTERED BY (id1) INTO n
// BUCKETS.  The library writer (host/library_writer.hpp) owes every row to the file of the bucket Spark computes for it,
//   g = pmod(Murmur3_x86_32.hashLong(id1, 42), n)
// and dealing rows to buckets one at a time on a host thread costs more than building the table.  Here the table gives a piece of its
// records back already ordered by g, with the place where every group starts, so that the writer appends runs.
//
// Two passes over the range's cells and a scan between them, all on the build stream; nothing but the results crosses to the host:
//   count    every occupied cell's key (tablebuild.h: cell_key) is hashed, and its group counted
//   scan     group_offsets = the exclusive prefix sums of the counts (one block: the groups are few beside the cells)
//   scatter  the same stream again; every record takes the next free slot of its group
// Both passes stream the cells as taxon_counts_kernel and respace_kernel do: persistent blocks, a grid-stride loop over 16-byte
// elements (two cells) with XR_UNROLL loads in flight per lane, 64-bit indices.  A cell whose taxon field is 0 is empty.
//
// While the groups fit a block's LDS (XR_LDS_GROUPS; SLK_EXPORT_LDS_GROUPS overrides it, so that tests take both routes at small
// sizes) a block counts into an LDS histogram.  The count pass leaves that histogram in device memory ([block][group]) beside adding
// it to the groups' totals; the scatter pass, which walks the same cells with the same grid, reads it back, reserves the block's run
// in each group it touches with ONE device atomic, and hands out the run's slots with LDS atomics: a device atomic per group and
// block, not per record.  Above the limit both passes use the device counters directly, one atomic per record.
//
// LDS budget: XR_BLOCK = 256 lanes and at most XR_LDS_GROUPS = 4096 counters of 4 bytes = 16 KiB per block, allocated dynamically at
// 4 bytes per group in use (200 groups, Spark's default partition count: 800 bytes).  XR_BLOCKS_PER_CU = 8 blocks are 32 waves and at
// most 128 KiB of the CU's 160 KiB: the histogram never costs a resident wave.  The passes are streams -- what they need is loads in
// flight -- with one integer hash and one LDS atomic per record on top.
//
// A grouped call covers at most 2^32 cells: a block's counters and the slots inside the piece are 32-bit then.  Pieces are the
// intended use (the CLI exports a few tens of millions of records at a time).
#include "hostside.h"
#include "tablebuild.h"

namespace {

constexpr int XR_BLOCK = 256;
constexpr int XR_UNROLL = 4;
constexpr int XR_BLOCKS_PER_CU = 8;
constexpr long XR_LDS_GROUPS = 4096;       // groups whose counters a block keeps in LDS (16 KiB)
constexpr long XR_LDS_GROUPS_MAX = 16384;  // what the override may raise it to: 64 KiB, a block's dynamic LDS
constexpr int XR_SCAN_BLOCK = 1024;

// Spark's bucket of a long column: Murmur3_x86_32.hashLong(value, seed 42), then pmod.  Restated for the device from
// host/library_writer.hpp (spark_hash_long, spark_bucket), which stays the host's definition; tests compare the two through
// slk_index_export_range.
__device__ __forceinline__ uint32_t xr_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ uint32_t xr_mix_k1(uint32_t k1) { k1 *= 0xcc9e2d51u; k1 = xr_rotl32(k1, 15); return k1 * 0x1b873593u; }
__device__ __forceinline__ uint32_t xr_mix_h1(uint32_t h1, uint32_t k1) { h1 ^= k1; h1 = xr_rotl32(h1, 13); return h1 * 5u + 0xe6546b64u; }
__device__ __forceinline__ uint32_t xr_group_of(uint64_t key, uint32_t n_groups) {
  uint32_t h1 = xr_mix_h1(42u, xr_mix_k1((uint32_t)key));
  h1 = xr_mix_h1(h1, xr_mix_k1((uint32_t)(key >> 32)));
  h1 ^= 8u;   // fmix(h1, length in bytes)
  h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
  const int32_t r = (int32_t)h1 % (int32_t)n_groups;   // pmod
  return (uint32_t)(r < 0 ? r + (int32_t)n_groups : r);
}

struct XrArgs {
  TableView T;
  uint64_t e0, n;                 // the range in 16-byte elements: first element, number of elements
  uint32_t n_groups;
  unsigned long long *counts;     // [n_groups]: records per group (count pass)
  unsigned long long *cursors;    // [n_groups]: the next free slot of every group (scatter pass; starts at the group's offset)
  uint32_t *block_hist;           // [grid][n_groups]: every block's own counts (LDS route)
  int64_t *keys;
  int32_t *taxa;
  uint64_t capacity;              // slots of keys / taxa
};

// f(cell index, cell) for every occupied cell of the range that falls to this block
template <class F>
__device__ __forceinline__ void xr_stream(const XrArgs &A, F f) {
  const ulonglong2 *__restrict__ cells = (const ulonglong2 *)A.T.cells + A.e0;
  const uint64_t tmask = (1ULL << A.T.g.taxon_bits) - 1;
  const uint64_t tile = (uint64_t)XR_BLOCK * XR_UNROLL, stride = (uint64_t)gridDim.x * tile;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < A.n; base += stride) {
    ulonglong2 v[XR_UNROLL];
#pragma unroll
    for (int u = 0; u < XR_UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * XR_BLOCK + threadIdx.x;
      v[u] = i < A.n ? cells[i] : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < XR_UNROLL; u++) {
      const uint64_t c = 2 * (A.e0 + base + (uint64_t)u * XR_BLOCK + threadIdx.x);
      if ((v[u].x & tmask) != 0) f(c, v[u].x);
      if ((v[u].y & tmask) != 0) f(c + 1, v[u].y);
    }
  }
}

template <bool LDS>
__global__ void __launch_bounds__(XR_BLOCK) xr_count_kernel(XrArgs A) {
  extern __shared__ uint32_t hist[];
  if (LDS) {
    for (uint32_t g = threadIdx.x; g < A.n_groups; g += XR_BLOCK) hist[g] = 0;
    __syncthreads();
  }
  xr_stream(A, [&](uint64_t i, uint64_t cell) {
    const uint32_t g = xr_group_of(cell_key(A.T.g, i, cell), A.n_groups);
    if (LDS) atomicAdd(&hist[g], 1u);
    else atomicAdd(&A.counts[g], 1ULL);
  });
  if (LDS) {
    __syncthreads();
    uint32_t *mine = A.block_hist + (uint64_t)blockIdx.x * A.n_groups;
    for (uint32_t g = threadIdx.x; g < A.n_groups; g += XR_BLOCK) {
      const uint32_t c = hist[g];
      mine[g] = c;
      if (c) atomicAdd(&A.counts[g], (unsigned long long)c);
    }
  }
}

// offsets[g] = counts[0] + .. + counts[g - 1] for g = 0 .. n (n + 1 values); cursors[g] = offsets[g] for g < n.  One block.
__global__ void __launch_bounds__(XR_SCAN_BLOCK) xr_scan_kernel(const unsigned long long *__restrict__ counts, uint32_t n,
                                                                unsigned long long *__restrict__ offsets,
                                                                unsigned long long *__restrict__ cursors) {
  __shared__ unsigned long long part[XR_SCAN_BLOCK];
  const uint64_t per = ((uint64_t)n + XR_SCAN_BLOCK - 1) / XR_SCAN_BLOCK;
  const uint64_t a = umin64(n, threadIdx.x * per), b = umin64(n, a + per);
  unsigned long long sum = 0;
  for (uint64_t g = a; g < b; g++) sum += counts[g];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < XR_SCAN_BLOCK; o <<= 1) {   // inclusive scan of the threads' sums
    const unsigned long long add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (uint64_t g = a; g < b; g++) {
    offsets[g] = run;
    cursors[g] = run;
    run += counts[g];
  }
  if (threadIdx.x == XR_SCAN_BLOCK - 1) offsets[n] = part[XR_SCAN_BLOCK - 1];
}

template <bool LDS>
__global__ void __launch_bounds__(XR_BLOCK) xr_scatter_kernel(XrArgs A) {
  extern __shared__ uint32_t next[];   // LDS route: the next free slot of this block's run in every group
  if (LDS) {
    const uint32_t *mine = A.block_hist + (uint64_t)blockIdx.x * A.n_groups;
    for (uint32_t g = threadIdx.x; g < A.n_groups; g += XR_BLOCK) {
      const uint32_t c = mine[g];
      // (a grouped call covers at most 2^32 cells: every slot of the piece is a 32-bit number)
      next[g] = c ? (uint32_t)atomicAdd(&A.cursors[g], (unsigned long long)c) : 0u;
    }
    __syncthreads();
  }
  xr_stream(A, [&](uint64_t i, uint64_t cell) {
    const uint64_t key = cell_key(A.T.g, i, cell);
    const uint32_t g = xr_group_of(key, A.n_groups);
    const uint64_t slot = LDS ? (uint64_t)atomicAdd(&next[g], 1u) : (uint64_t)atomicAdd(&A.cursors[g], 1ULL);
    if (slot < A.capacity) {
      A.keys[slot] = (int64_t)key;
      A.taxa[slot] = ext_taxon(A.T, (int32_t)(cell & ((1ULL << A.T.g.taxon_bits) - 1)));
    }
  });
}

long xr_lds_groups() {   // (per call: tests move it)
  return std::min(XR_LDS_GROUPS_MAX, std::max(0L, env_long("SLK_EXPORT_LDS_GROUPS", XR_LDS_GROUPS)));
}

}  // namespace

extern "C" int32_t slk_index_export_range(const slk_index *ix, uint64_t bucket0, uint64_t bucket1, int32_t n_groups, int64_t *keys,
                                          int32_t *taxa, uint64_t capacity, uint64_t *group_offsets, uint64_t *n_records) {
  if (!ix || !n_records || (capacity && (!keys || !taxa))) return fail(SLK_E_INVALID, "null argument");
  *n_records = 0;
  int32_t rc = set_device(ix);   // (a spent index: SLK_E_STATE)
  if (rc) return rc;
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "slk_index_export_range supports minimizers of up to 32 nt (one id column)");
  if (n_groups < 0) return fail(SLK_E_INVALID, "n_groups = %d", n_groups);
  if (bucket0 > bucket1 || bucket1 > ix->nbuckets)
    return fail(SLK_E_INVALID, "buckets [%llu, %llu) of a table of %llu", (unsigned long long)bucket0, (unsigned long long)bucket1,
                (unsigned long long)ix->nbuckets);
  const uint64_t cells = (bucket1 - bucket0) * CELLS;
  const bool grouped = n_groups > 0 && capacity > 0;
  if (n_groups > 0 && cells > (1ULL << 32))
    return fail(SLK_E_INVALID, "a grouped export covers at most 2^32 cells (%llu buckets): export the table in pieces",
                (unsigned long long)((1ULL << 32) / CELLS));
  if (grouped && !group_offsets) return fail(SLK_E_INVALID, "null argument");
  if (cells == 0) {
    if (grouped) std::fill(group_offsets, group_offsets + (size_t)n_groups + 1, (uint64_t)0);
    return SLK_OK;
  }
  hipStream_t s = ix->build_stream;   // the stream the records were inserted on: the passes see them all
  const uint64_t room = std::min(capacity, cells);   // (12 B per possible record of the range, never the table's record count)
  DevBuf dk, dt, dc;
  HIPCHK(dk.ensure(std::max<uint64_t>(room, 1) * 8));
  HIPCHK(dt.ensure(std::max<uint64_t>(room, 1) * 4));
  unsigned long long n = 0;
  if (!grouped) {
    // any order (or the count alone): the compacting pass of build.hip over the range
    HIPCHK(dc.ensure(8));
    HIPCHK(hipMemsetAsync(dc.p, 0, 8, s));
    launch_export_range(ix->view(), bucket0, bucket1, dk.as<int64_t>(), dt.as<int32_t>(), room, dc.as<unsigned long long>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&n, dc.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  } else {
    XrArgs A{};
    A.T = ix->view();
    A.e0 = bucket0 * LPB;
    A.n = (bucket1 - bucket0) * LPB;
    A.n_groups = (uint32_t)n_groups;
    const uint64_t tile = (uint64_t)XR_BLOCK * XR_UNROLL;
    const unsigned grid = (unsigned)std::min<uint64_t>((A.n + tile - 1) / tile, (uint64_t)grid_for(ix->device, XR_BLOCKS_PER_CU, nullptr));   // both passes: the same
    const bool lds = (long)n_groups <= xr_lds_groups();
    const size_t G = (size_t)n_groups, lds_bytes = lds ? G * 4 : 0;
    // the group counters: counts [G], offsets [G + 1], cursors [G], and on the LDS route the blocks' histograms
    DevBuf dh;
    HIPCHK(dc.ensure((3 * G + 1) * 8));
    unsigned long long *counts = dc.as<unsigned long long>(), *offsets = counts + G, *cursors = offsets + G + 1;
    HIPCHK(hipMemsetAsync(counts, 0, G * 8, s));
    if (lds) HIPCHK(dh.ensure((size_t)grid * G * 4));
    A.counts = counts;
    A.cursors = cursors;
    A.block_hist = dh.as<uint32_t>();
    A.keys = dk.as<int64_t>();
    A.taxa = dt.as<int32_t>();
    A.capacity = room;
    if (lds) hipLaunchKernelGGL(xr_count_kernel<true>, dim3(grid), dim3(XR_BLOCK), lds_bytes, s, A);
    else hipLaunchKernelGGL(xr_count_kernel<false>, dim3(grid), dim3(XR_BLOCK), 0, s, A);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(xr_scan_kernel, dim3(1), dim3(XR_SCAN_BLOCK), 0, s, counts, A.n_groups, offsets, cursors);
    HIPCHK(hipGetLastError());
    if (lds) hipLaunchKernelGGL(xr_scatter_kernel<true>, dim3(grid), dim3(XR_BLOCK), lds_bytes, s, A);
    else hipLaunchKernelGGL(xr_scatter_kernel<false>, dim3(grid), dim3(XR_BLOCK), 0, s, A);
    HIPCHK(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the offsets are copied as they are");
    HIPCHK(hipMemcpyAsync(group_offsets, offsets, (G + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    n = group_offsets[G];
  }
  *n_records = n;
  if (capacity && n > capacity) return fail(SLK_E_CAPACITY, "%llu records, capacity %llu", n, (unsigned long long)capacity);
  if (capacity && n) {
    HIPCHK(hipMemcpyAsync(keys, dk.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(taxa, dt.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return SLK_OK;
}
