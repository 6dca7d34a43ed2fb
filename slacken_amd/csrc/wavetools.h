// wavetools.h -- the wave- and block-level pieces that the passes over a library or a sample share (build.hip, respace.hip,
// taxstats.hip, migration.hip, coverage.hip, support.hip): reductions, the rank of a lane in a ballot, the per-wave LDS queue, one
// round of "the first lane names its key", a block's LDS count map, and consecutive output slots for a wave.  gfx950, wave64.
//
// The three levels.  A pass that counts records under a key (a taxon, a pair of taxa, a (source, depth) pair) whose hot keys would
// serialise on a handful of HBM addresses counts on three levels:
//   wave    *_LEADER_ROUNDS times, the first lane still holding a key names it (leader_round); the lanes holding the same key hand
//           their numbers to it and leave, and the leader alone adds the sum
//   block   an open-addressing map key -> counters in LDS (LdsCountMap) takes those sums and the lanes left over
//   device  at the end of the block every occupied LDS slot goes to the device-wide counters (an array, or a pairmap.h map)
// A lane that finds no LDS slot within the map's probes adds to the device-wide counters itself.  Every route is an addition: the
// result does not depend on which one a record took.  What keeps a block's 32-bit LDS counters from wrapping is the caller's.
#pragma once
#include "engine.h"

namespace slk {

__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return (uint32_t)__builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1)
    v += ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o);
  return v;
}
template <class T> __device__ __forceinline__ T wave_shfl(T v, int src) {   // lane src's v, of 32 or 64 bits
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "an integer of 32 or 64 bits");
  if constexpr (sizeof(T) == 4) return (T)__shfl((int)v, src);
  else return (T)(((uint64_t)(uint32_t)__shfl((int)((uint64_t)v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src));
}
__device__ __forceinline__ int lane_rank(uint64_t mask) {  // popcount(mask & lanes lower than this one)
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// The per-wave queue that turns "a few lanes have a record at this step" into "64 lanes have one each": a ring of 128 (key, 32-bit
// payload) entries in LDS arrays of the caller's, one pair of arrays per wave.  push() and drain() are called by whole waves.  They
// hand `flush` (entry index, this lane has an entry) for every lane: the functor reads key[e] / payload[e] itself, and may go on
// as a whole wave afterwards.  n < 64 on entry of push, at most 64 arrive, and 64 leave as soon as n >= 64: the 128 entries never
// wrap onto themselves, and what drain() finds is less than 64.
template <class Payload>
struct WaveQueue {
  static_assert(sizeof(Payload) == 4, "one 32-bit payload per key");
  uint64_t *const key;
  Payload *const payload;
  const uint32_t lane;
  uint32_t head = 0, n = 0;   // wave-uniform

  __device__ __forceinline__ WaveQueue(uint64_t *key_, Payload *payload_, uint32_t lane_) : key(key_), payload(payload_), lane(lane_) {}

  template <class F> __device__ __forceinline__ void flush(uint32_t cnt, F &&f) {   // cnt <= min(n, 64)
    f((head + lane) & 127, lane < cnt);
    head = (head + cnt) & 127;
    n -= cnt;
  }
  template <class F> __device__ __forceinline__ void push(bool emit, uint64_t k, Payload p, F &&f) {
    const uint64_t mask = __ballot(emit);
    if (mask == 0) return;
    if (emit) {
      const uint32_t e = (head + n + (uint32_t)lane_rank(mask)) & 127;
      key[e] = k;
      payload[e] = p;
    }
    n += (uint32_t)__popcll(mask);
    if (n >= 64) flush(64, f);
  }
  template <class F> __device__ __forceinline__ void drain(F &&f) { if (n) flush(n, f); }
};

// One round of the wave level: the first lane that still has something names its key, and body(leader lane, the leader's key,
// same) runs in every lane -- same: this lane has something, under the leader's key.  What the lanes with `same` hand to the leader
// (a ballot's popcount, wave sums) and how many rounds are worth it is the caller's; body ends with have = have && !same.  Returns
// false, without calling body, when no lane has anything.  Called by whole waves.  (A continuation, not a returned struct: body
// then sits inside the branch that found a leader, and nothing has to be merged with the nothing-held path and tested again.)
template <class Key, class Body>
__device__ __forceinline__ bool leader_round(bool have, Key key, Body &&body) {
  const uint64_t holding = __ballot(have);
  if (holding == 0) return false;
  const int leader = __ffsll((unsigned long long)holding) - 1;
  const Key lk = wave_shfl(key, leader);
  body(leader, lk, have && key == lk);
  return true;
}

// The block level: SLOTS keys in LDS (EMPTY: a free slot), open addressing with at most PROBES linear probes.  The counters are
// LDS arrays of the caller's, indexed by the slot: found(slot) adds to them with LDS atomics, full() takes the key to the
// device-wide counters.  PEEK: the slot is read before the CAS -- a slot never changes owner, so a read that finds the key saves the
// CAS (taxstats.hip, support.hip: a handful of hot taxa; migration.hip and coverage.hip's fold issue the CAS at once).
template <class Key, Key EMPTY, uint32_t SLOTS, int PROBES, bool PEEK>
struct LdsCountMap {
  static_assert((SLOTS & (SLOTS - 1)) == 0, "a power of two");
  Key keys[SLOTS];

  // by the whole block, before the first add: zero(slot) clears the caller's counters
  template <class Z> __device__ __forceinline__ void clear(uint32_t tid, uint32_t nthreads, Z &&zero) {
    for (uint32_t s = tid; s < SLOTS; s += nthreads) { keys[s] = EMPTY; zero(s); }
    __syncthreads();
  }
  // hash: the slot to start at
  template <class Found, class Full> __device__ __forceinline__ void add(Key key, uint32_t hash, Found &&found, Full &&full) {
    uint32_t h = hash & (SLOTS - 1);
    for (int probe = 0; probe < PROBES; probe++) {
      Key prev;
      if (PEEK) {
        prev = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
        if (prev == EMPTY) prev = atomicCAS(&keys[h], EMPTY, key);
      } else {
        prev = atomicCAS(&keys[h], EMPTY, key);
      }
      if (prev == EMPTY || prev == key) { found(h); return; }
      h = (h + 1) & (SLOTS - 1);
    }
    full();
  }
  // by the whole block, after the last add: out(key, slot) for every occupied slot
  template <class Out> __device__ __forceinline__ void drain(uint32_t tid, uint32_t nthreads, Out &&out) {
    __syncthreads();
    for (uint32_t s = tid; s < SLOTS; s += nthreads)
      if (keys[s] != EMPTY) out(keys[s], s);
  }
};

// Consecutive output slots for the lanes of a wave that have something to write, with one atomic per wave: the slot of this lane
// (meaningless where !has).  Called by whole waves.
__device__ __forceinline__ unsigned long long wave_alloc_slots(bool has, unsigned long long *cursor) {
  const uint64_t mask = __ballot(has);
  if (mask == 0) return 0;
  const uint32_t before = (uint32_t)lane_rank(mask);
  unsigned long long first = 0;
  if (has && before == 0) first = atomicAdd(cursor, (unsigned long long)__popcll(mask));
  return wave_shfl(first, __ffsll((long long)mask) - 1) + before;
}

}  // namespace slk
