// pairmap.h -- the device-wide (a << 32 | b) -> uint64 count map that bracken.hip (source, dest) and migration.hip (t1, t2) add
// into, and that coverage.hip keys by (cell << 28 | source) and by (source << 32 | depth): open addressing with linear probing over
// a power-of-two number of slots, two parallel arrays in HBM (coverage.hip keeps a third beside them), moved to a larger map by
// PairMap::grow_into.  Internal.
#pragma once
#include "hostside.h"

constexpr uint64_t PAIR_EMPTY = ~0ULL;   // free slot (no pair is all ones: the low half is a taxon found in a table, > 0)

// counts[slot of key] += n, claiming a slot if the key is new (then ++*n_pairs when given).  false: the map is full.
__device__ __forceinline__ bool pair_map_add(unsigned long long *keys, unsigned long long *counts, uint64_t mask,
                                             unsigned long long key, unsigned long long n, unsigned long long *n_pairs) {
  uint64_t h = slk::fmix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    const unsigned long long prev = atomicCAS(&keys[h], (unsigned long long)PAIR_EMPTY, key);
    if (prev == PAIR_EMPTY || prev == key) {
      atomicAdd(&counts[h], n);
      if (n_pairs != nullptr && prev == PAIR_EMPTY) atomicAdd(n_pairs, 1ULL);
      return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

// The same with two counters per key (coverage.hip: a sum and a number of distinct things): first[slot] += a, second[slot] += b.
__device__ __forceinline__ bool pair_map_add2(unsigned long long *keys, unsigned long long *first, unsigned long long *second, uint64_t mask,
                                              unsigned long long key, unsigned long long a, unsigned long long b,
                                              unsigned long long *n_pairs) {
  uint64_t h = slk::fmix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    const unsigned long long prev = atomicCAS(&keys[h], (unsigned long long)PAIR_EMPTY, key);
    if (prev == PAIR_EMPTY || prev == key) {
      atomicAdd(&first[h], a);
      atomicAdd(&second[h], b);
      if (n_pairs != nullptr && prev == PAIR_EMPTY) atomicAdd(n_pairs, 1ULL);
      return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

// every pair of an old map into a new one (which has room: it is larger); TWO: a second counter per key (old_second, second).
// A template, so that only the translation units that grow a map hold the kernel.
template <bool TWO>
__global__ void __launch_bounds__(256) pair_map_rehash_kernel(const unsigned long long *old_keys, const unsigned long long *old_first,
                                                              const unsigned long long *old_second, uint64_t old_cap,
                                                              unsigned long long *keys, unsigned long long *first,
                                                              unsigned long long *second, uint64_t mask, int32_t *status) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_cap; i += stride) {
    if (old_keys[i] == PAIR_EMPTY) continue;
    const bool ok = TWO ? pair_map_add2(keys, first, second, mask, old_keys[i], old_first[i], old_second[i], nullptr)
                        : pair_map_add(keys, first, mask, old_keys[i], old_first[i], nullptr);
    if (!ok) atomicOr(status, 2);
  }
}

struct PairMap {
  DevBuf keys, counts;
  uint64_t cap = 0;   // slots, a power of two
  unsigned long long *k() const { return keys.as<unsigned long long>(); }
  unsigned long long *c() const { return counts.as<unsigned long long>(); }
  // an empty map of `slots` slots (whatever it held is gone), ordered on s
  int32_t reset(hipStream_t s, uint64_t slots) {
    HIPCHK(keys.ensure(slots * 8));
    HIPCHK(counts.ensure(slots * 8));
    HIPCHK(hipMemsetAsync(keys.p, 0xff, slots * 8, s));
    HIPCHK(hipMemsetAsync(counts.p, 0, slots * 8, s));
    cap = slots;
    return SLK_OK;
  }
  // Every pair of this map into `now`, a larger one that the caller has reset; TWO: with the second counters beside the two maps
  // (second, now_second; null otherwise).  A pair that finds no room sets bit 1 of *status (device memory).  Synchronises s: this
  // map can be freed.
  template <bool TWO>
  int32_t grow_into(hipStream_t s, PairMap &now, const DevBuf *second, DevBuf *now_second, int32_t *status) const {
    hipLaunchKernelGGL(pair_map_rehash_kernel<TWO>, dim3((unsigned)std::min<uint64_t>((cap + 255) / 256, 4096)), dim3(256), 0, s, k(), c(),
                       TWO ? second->as<unsigned long long>() : nullptr, cap, now.k(), now.c(),
                       TWO ? now_second->as<unsigned long long>() : nullptr, now.cap - 1, status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return SLK_OK;
  }
  // the pairs with their counts, unordered; synchronises s
  int32_t read(hipStream_t s, std::vector<uint64_t> &hk, std::vector<uint64_t> &hc) const {
    hk.resize(cap);
    hc.resize(cap);
    HIPCHK(hipMemcpyAsync(hk.data(), keys.p, cap * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hc.data(), counts.p, cap * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint64_t w = 0;
    for (uint64_t i = 0; i < cap; i++)
      if (hk[i] != PAIR_EMPTY) { hk[w] = hk[i]; hc[w] = hc[i]; w++; }
    hk.resize(w);
    hc.resize(w);
    return SLK_OK;
  }
};
