// compare.hip -- classifications joined with a truth mapping on a string id: the join of MappingComparison
// (S/slacken/analysis/MappingComparison.scala:157-159, 216-217, with the rows of readCustomFormat :265-274 and readKrakenFormat
// :259-263).  The reference mapping's ids stay resident: their NORMALISED bytes (every "/1" removed; rows whose id holds "/2" are
// dropped) in an arena, and an open-addressing table of entries (64-bit hash of the normalised id | arena offset, length, raw taxon,
// a "matched" flag, where the row stood in the text).  Test text streams through: every row's RAW id is hashed and looked up; hash and
// length are compared first, then the bytes against the arena (pt_equal) -- the join is exact, not "equal hashes".  Every joined row
// is counted under (refTaxon << 32 | testTaxon), raw ids, on the three levels of wavetools.h: the taxonomy stays on the host, which
// sees the distinct pairs only.
//
// Text arrives in chunks under the contract of the parser: the line starts are found by the passes of textlines.h, then
// one lane takes one line: it walks to the tabs in front of the columns it needs (never further), parses the taxon as an optional
// sign and digits, and hashes the id.  A line with too few columns, an empty field or a taxon that is no non-negative Java int
// leaves its offset in the error word (atomicMin: the lowest survives).
//   reference  cp_reference_kernel: the normalised bytes go to the arena (one atomic per wave reserves the wave's bytes), the entry
//              claims a slot by CAS on the hash word -- equal hashes are both stored, probing goes on -- and the row is counted under
//              its raw taxon.  Duplicates are NOT decided here: another lane's entry may be half written.  cp_duplicates_kernel, behind
//              the kernel boundary, lets every new entry walk from its home to its own slot looking for an entry of equal hash, length
//              and bytes; of two equal ids the one that lies later on the chain finds the other.
//   test       cp_test_kernel: on a match atomicOr on the entry's flag -- it was set already: a test id occurs twice -- and the pair count.
// The host sizes table, arena and maps before every launch from the number of lines the chunk holds (known after the line passes),
// so no kernel can run out of room; the table doubles by rehashing the stored hashes (cp_rehash_kernel).  Nothing wider than a
// workgroup barrier is used inside a kernel.  SLK_COMPARE_HASH_BITS=N (read at create) truncates the hash to N bits: with N = 2
// every chain collides, and only the byte comparison tells ids apart.
#include "textlines.h"
#include "pairmap.h"
#include "wavetools.h"

namespace {

// 256 lanes and 2048 slots of 12 bytes (24 KiB of the CU's 160 KiB LDS): six blocks, 24 waves per CU to hide the table's and the
// arena's latency behind.
constexpr int CP_BLOCK = 256;
constexpr uint32_t CP_SLOTS = 2048;
constexpr int CP_PROBES = 16;
constexpr int CP_LEADER_ROUNDS = 2;
constexpr int CP_BLOCKS_PER_CU = 6;
constexpr unsigned long long CP_EMPTY = ~0ULL;   // a free slot's hash word (no stored hash is all ones: cp_finish_hash)

// the kinds of slk_compare_error, and CP_INTERNAL: a structure the host had sized was full after all
constexpr unsigned CP_INTERNAL = 15;

struct CpEntry {   // 32 bytes, indexed by the slot
  uint64_t off;    // of the normalised id in the arena
  uint64_t src;    // of the row's line in the reference text (all chunks counted)
  uint32_t len;
  int32_t taxon;   // raw, as the text has it
  uint32_t flag;   // bit 0: a test row of the current test matched
  uint32_t pad;
};

struct CpArgs {
  const uint8_t *text;
  uint64_t n;
  const uint32_t *S;      // line starts, S[Lp] readable (textlines.h)
  uint32_t Lp;            // the lines that count
  uint32_t id_col, taxon_col;   // 0-based
  uint64_t base;          // where text[0] lies in the whole text
  unsigned long long *hash;   // the table: hash words, entries, slots - 1
  CpEntry *entries;
  uint64_t mask;
  uint8_t *arena;
  uint64_t arena_cap;
  uint64_t hash_mask;     // SLK_COMPARE_HASH_BITS
  unsigned long long *slots;   // reference: [Lp] the slot line j's entry took, CP_EMPTY = none
  unsigned long long *map_keys, *map_counts;   // the device-wide count map of this pass (reference: raw taxon; test: pair)
  uint64_t map_mask;
  unsigned long long *counters;   // [0] reference rows [1] dropped as "/2" [2] kept [3] test rows [4] joined [5] arena bytes [6] pairs [7] reference taxa
  unsigned long long *error;      // the smallest (offset << 8 | kind)
};

__device__ __forceinline__ void cp_error(const CpArgs &A, uint64_t offset, unsigned kind) {
  atomicMin(A.error, (unsigned long long)((offset << 8) | kind));
}

// The columns id_col and taxon_col of the line [s, e), fields split at TAB: false for too few columns, an empty field, or a taxon that
// Integer.parseInt refuses or that is negative.  The walk ends at the later of the two columns.
__device__ __forceinline__ bool cp_fields(const uint8_t *text, uint32_t s, uint32_t e, uint32_t id_col, uint32_t taxon_col, uint32_t &id_s,
                                          uint32_t &id_e, int32_t &taxon) {
  const uint32_t last = id_col > taxon_col ? id_col : taxon_col;
  uint32_t col = 0, fs = s, t_s = 0, t_e = 0;
  id_s = id_e = 0;
  for (uint32_t q = s;; q++) {
    if (q == e || text[q] == '\t') {
      if (col == id_col) { id_s = fs; id_e = q; }
      if (col == taxon_col) { t_s = fs; t_e = q; }
      if (col == last) break;
      if (q == e) return false;
      col++;
      fs = q + 1;
    }
  }
  if (id_e == id_s || t_e == t_s) return false;
  uint32_t p = t_s;
  bool neg = false;
  if (text[p] == '+' || text[p] == '-') { neg = text[p] == '-'; p++; }
  if (p == t_e) return false;
  uint64_t v = 0;
  for (; p < t_e; p++) {
    const uint32_t c = text[p];
    if (c < '0' || c > '9') return false;
    v = v * 10 + (c - '0');
    if (v > 2147483648ULL) return false;
  }
  if (neg ? v != 0 : v > 2147483647ULL) return false;   // ("-0" is 0; any other negative taxon is refused)
  taxon = (int32_t)v;
  return true;
}

__device__ __forceinline__ uint64_t cp_hash_byte(uint64_t h, uint32_t c) { return (h ^ c) * 0x100000001b3ULL; }   // FNV-1a
constexpr uint64_t CP_HASH_INIT = 0xcbf29ce484222325ULL;
__device__ __forceinline__ unsigned long long cp_finish_hash(uint64_t h, uint64_t hash_mask) {
  h = fmix64(h) & hash_mask;
  return h == CP_EMPTY ? h - 1 : h;
}
__device__ __forceinline__ uint64_t cp_home(unsigned long long h, uint64_t mask) { return fmix64(h) & mask; }

using CpMap = LdsCountMap<unsigned long long, PAIR_EMPTY, CP_SLOTS, CP_PROBES, false>;

// The three levels of wavetools.h for one key per lane; called by whole waves.
__device__ __forceinline__ void cp_count(const CpArgs &A, CpMap &M, unsigned int *lcounts, bool have, unsigned long long key,
                                         unsigned long long *n_keys) {
  const int lane = threadIdx.x & 63;
  auto global_add = [&](unsigned long long k, unsigned long long c) {
    if (!pair_map_add(A.map_keys, A.map_counts, A.map_mask, k, c, n_keys)) cp_error(A, 0, CP_INTERNAL);
  };
  auto block_add = [&](unsigned long long k, unsigned int c) {
    M.add(k, (uint32_t)fmix64(k), [&](uint32_t h) { atomicAdd(&lcounts[h], c); }, [&] { global_add(k, c); });
  };
  for (int round = 0; round < CP_LEADER_ROUNDS; round++) {
    const bool any = leader_round(have, key, [&](int leader, unsigned long long lk, bool same) {
      const uint64_t group = __ballot(same);
      if (lane == leader) block_add(lk, (unsigned int)__popcll(group));
      have = have && !same;
    });
    if (!any) break;
  }
  if (have) block_add(key, 1u);
}
__device__ __forceinline__ void cp_drain(const CpArgs &A, CpMap &M, unsigned int *lcounts, unsigned long long *n_keys) {
  M.drain(threadIdx.x, CP_BLOCK, [&](unsigned long long k, uint32_t s) {
    if (!pair_map_add(A.map_keys, A.map_counts, A.map_mask, k, (unsigned long long)lcounts[s], n_keys)) cp_error(A, 0, CP_INTERNAL);
  });
}

// One lane per line of reference text: fields, "/2", the hash over the id without its "/1"s, the bytes to the arena, the entry.
__global__ void __launch_bounds__(CP_BLOCK) cp_reference_kernel(CpArgs A) {
  __shared__ CpMap M;
  __shared__ unsigned int lcounts[CP_SLOTS];
  M.clear(threadIdx.x, CP_BLOCK, [&](uint32_t s) { lcounts[s] = 0; });
  const int lane = threadIdx.x & 63;
  uint64_t n_rows = 0, n_dropped = 0, n_kept = 0;   // of this wave (every lane keeps the same numbers)
  const uint64_t stride = (uint64_t)gridDim.x * CP_BLOCK;
  for (uint64_t first = (uint64_t)blockIdx.x * CP_BLOCK; first < A.Lp; first += stride) {   // block-uniform: the ballots see whole waves
    const uint64_t j = first + threadIdx.x;
    const bool in = j < A.Lp;
    bool ok = false;
    uint32_t s = 0, id_s = 0, id_e = 0;
    int32_t taxon = 0;
    if (in) {
      s = A.S[j];
      const uint32_t e = fq_line_end(A.text, s, A.S[j + 1]);
      if (e > s) {   // (empty lines are skipped)
        ok = cp_fields(A.text, s, e, A.id_col, A.taxon_col, id_s, id_e, taxon);
        if (!ok) cp_error(A, A.base + s, SLK_COMPARE_BAD_LINE);
      }
    }
    bool second = false;   // the id holds "/2": the second mate's row
    uint32_t nlen = 0;
    uint64_t h = CP_HASH_INIT;
    if (ok) {
      for (uint32_t q = id_s; q + 1 < id_e; q++)
        if (A.text[q] == '/' && A.text[q + 1] == '2') { second = true; break; }
      if (!second) {
        for (uint32_t q = id_s; q < id_e;) {   // replaceAll("/1", ""): one pass from the left, matches do not overlap
          if (A.text[q] == '/' && q + 1 < id_e && A.text[q + 1] == '1') { q += 2; continue; }
          h = cp_hash_byte(h, A.text[q]);
          nlen++;
          q++;
        }
      }
    }
    const bool keep = ok && !second;
    n_rows += (uint64_t)__popcll(__ballot(ok));
    n_dropped += (uint64_t)__popcll(__ballot(ok && second));
    n_kept += (uint64_t)__popcll(__ballot(keep));
    // the wave's bytes of the arena with one atomic: an inclusive scan of the lengths, the last lane reserves the total
    uint32_t incl = keep ? nlen : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    unsigned long long wave_off = 0;
    if (lane == 63 && incl) wave_off = atomicAdd(A.counters + 5, (unsigned long long)incl);
    wave_off = wave_shfl(wave_off, 63);
    unsigned long long slot = CP_EMPTY;
    if (keep) {
      const uint64_t off = wave_off + incl - nlen;
      if (off + nlen > A.arena_cap) {
        cp_error(A, A.base + s, CP_INTERNAL);
      } else {
        uint8_t *dst = A.arena + off;
        for (uint32_t q = id_s; q < id_e;) {
          if (A.text[q] == '/' && q + 1 < id_e && A.text[q + 1] == '1') { q += 2; continue; }
          *dst++ = A.text[q++];
        }
        const unsigned long long hh = cp_finish_hash(h, A.hash_mask);
        uint64_t pos = cp_home(hh, A.mask);
        for (uint64_t probe = 0; probe <= A.mask; probe++) {
          if (atomicCAS(&A.hash[pos], CP_EMPTY, hh) == CP_EMPTY) { slot = pos; break; }
          pos = (pos + 1) & A.mask;
        }
        if (slot == CP_EMPTY) {
          cp_error(A, A.base + s, CP_INTERNAL);
        } else {
          CpEntry en;
          en.off = off; en.src = A.base + s; en.len = nlen; en.taxon = taxon; en.flag = 0; en.pad = 0;
          A.entries[slot] = en;
        }
      }
    }
    if (in) A.slots[j] = slot;
    cp_count(A, M, lcounts, keep && slot != CP_EMPTY, (unsigned long long)(uint32_t)taxon, A.counters + 7);
  }
  if (lane == 0) {
    if (n_rows) atomicAdd(A.counters + 0, (unsigned long long)n_rows);
    if (n_dropped) atomicAdd(A.counters + 1, (unsigned long long)n_dropped);
    if (n_kept) atomicAdd(A.counters + 2, (unsigned long long)n_kept);
  }
  cp_drain(A, M, lcounts, A.counters + 7);
}

// Behind the insert's kernel boundary every entry is whole.  One lane per line: its entry walks from its home to its own slot -- every
// slot between was taken when the entry probed past it, and nothing is ever removed -- looking for an equal id.
__global__ void __launch_bounds__(CP_BLOCK) cp_duplicates_kernel(CpArgs A) {
  const uint64_t stride = (uint64_t)gridDim.x * CP_BLOCK;
  for (uint64_t j = (uint64_t)blockIdx.x * CP_BLOCK + threadIdx.x; j < A.Lp; j += stride) {
    const unsigned long long slot = A.slots[j];
    if (slot == CP_EMPTY) continue;
    const unsigned long long hh = A.hash[slot];
    const CpEntry me = A.entries[slot];
    for (uint64_t pos = cp_home(hh, A.mask); pos != slot; pos = (pos + 1) & A.mask) {
      if (A.hash[pos] != hh) continue;
      const CpEntry other = A.entries[pos];
      if (other.len == me.len && pt_equal(A.arena + other.off, A.arena + me.off, me.len)) {
        cp_error(A, me.src, SLK_COMPARE_DUPLICATE_REFERENCE);
        break;
      }
    }
  }
}

// One lane per line of test text: fields, the hash of the raw id, the probe, the flag, the pair count.
__global__ void __launch_bounds__(CP_BLOCK) cp_test_kernel(CpArgs A) {
  __shared__ CpMap M;
  __shared__ unsigned int lcounts[CP_SLOTS];
  M.clear(threadIdx.x, CP_BLOCK, [&](uint32_t s) { lcounts[s] = 0; });
  const int lane = threadIdx.x & 63;
  uint64_t n_rows = 0, n_joined = 0;
  const uint64_t stride = (uint64_t)gridDim.x * CP_BLOCK;
  for (uint64_t first = (uint64_t)blockIdx.x * CP_BLOCK; first < A.Lp; first += stride) {
    const uint64_t j = first + threadIdx.x;
    bool ok = false;
    uint32_t s = 0, id_s = 0, id_e = 0;
    int32_t taxon = 0;
    if (j < A.Lp) {
      s = A.S[j];
      const uint32_t e = fq_line_end(A.text, s, A.S[j + 1]);
      if (e > s) {
        ok = cp_fields(A.text, s, e, A.id_col, A.taxon_col, id_s, id_e, taxon);
        if (!ok) cp_error(A, A.base + s, SLK_COMPARE_BAD_LINE);
      }
    }
    bool joined = false;
    int32_t ref_taxon = 0;
    if (ok) {
      const uint32_t len = id_e - id_s;
      uint64_t h = CP_HASH_INIT;
      for (uint32_t q = id_s; q < id_e; q++) h = cp_hash_byte(h, A.text[q]);
      const unsigned long long hh = cp_finish_hash(h, A.hash_mask);
      uint64_t pos = cp_home(hh, A.mask);
      for (uint64_t probe = 0; probe <= A.mask; probe++) {
        const unsigned long long hv = A.hash[pos];
        if (hv == CP_EMPTY) break;
        if (hv == hh) {
          const CpEntry en = A.entries[pos];
          if (en.len == len && pt_equal(A.arena + en.off, A.text + id_s, len)) {
            joined = true;
            ref_taxon = en.taxon;
            if (atomicOr(&A.entries[pos].flag, 1u) & 1u) cp_error(A, A.base + s, SLK_COMPARE_DUPLICATE_TEST);
            break;
          }
        }
        pos = (pos + 1) & A.mask;
      }
    }
    n_rows += (uint64_t)__popcll(__ballot(ok));
    n_joined += (uint64_t)__popcll(__ballot(joined));
    // (both taxa are non-negative: no key is all ones)
    cp_count(A, M, lcounts, joined, ((unsigned long long)(uint32_t)ref_taxon << 32) | (uint32_t)taxon, A.counters + 6);
  }
  if (lane == 0) {
    if (n_rows) atomicAdd(A.counters + 3, (unsigned long long)n_rows);
    if (n_joined) atomicAdd(A.counters + 4, (unsigned long long)n_joined);
  }
  cp_drain(A, M, lcounts, A.counters + 6);
}

// every entry of an old table into a new, larger one, from the stored hashes
__global__ void __launch_bounds__(256) cp_rehash_kernel(const unsigned long long *old_hash, const CpEntry *old_entries, uint64_t old_slots,
                                                        unsigned long long *hash, CpEntry *entries, uint64_t mask, unsigned long long *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_slots; i += stride) {
    const unsigned long long hh = old_hash[i];
    if (hh == CP_EMPTY) continue;
    uint64_t pos = cp_home(hh, mask);
    bool placed = false;
    for (uint64_t probe = 0; probe <= mask; probe++) {
      if (atomicCAS(&hash[pos], CP_EMPTY, hh) == CP_EMPTY) { entries[pos] = old_entries[i]; placed = true; break; }
      pos = (pos + 1) & mask;
    }
    if (!placed) atomicMin(error, (unsigned long long)CP_INTERNAL);
  }
}

__global__ void __launch_bounds__(256) cp_clear_flags_kernel(const unsigned long long *hash, CpEntry *entries, uint64_t slots) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride)
    if (hash[i] != CP_EMPTY) entries[i].flag = 0;
}

uint64_t pow2_at_least(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

}  // namespace

struct slk_compare {
  slk_index *ix = nullptr;       // the owner of the stream given at create: names the device
  int32_t device = 0;
  DevBuf hash, entries;          // the table: `slots` hash words and entries
  uint64_t slots = 0;
  DevBuf arena;
  uint64_t arena_cap = 0;
  PairMap pairs, ref_taxa;       // (refTaxon << 32 | testTaxon) -> joined rows of the current test; raw reference taxon -> kept rows
  DevBuf counters, error, status;   // CpArgs.counters (8 x uint64), CpArgs.error, the maps' grow status
  DevBuf scratch, line_slots, text;   // the line passes' tiles and starts; the reference lines' slots; a host call's chunk
  uint64_t hash_mask = ~0ULL;
  unsigned blocks = 0;
  uint64_t ref_base = 0, test_base = 0;   // bytes consumed so far
  unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the counters as last read
  unsigned long long err = ~0ULL;     // the error word as last read
  bool spent = false;            // a HIP call failed, or a bad line or a duplicate ended the run: the counts are incomplete
};

static const char *CP_SPENT = "compare: an earlier call of this handle failed (slk_compare_error says where a bad line or a duplicate stood); destroy it";

// table, arena and the reference lines' slots for `lines` more ids of `bytes` more bytes
static int32_t cp_make_room(slk_compare *h, hipStream_t s, uint64_t lines, uint64_t bytes) {
  const uint64_t need = pow2_at_least(std::max<uint64_t>(2 * (h->c[2] + lines), 1024));
  if (need > h->slots) {
    DevBuf nh, ne;
    HIPCHK(nh.ensure(need * 8));
    HIPCHK(ne.ensure(need * sizeof(CpEntry)));
    HIPCHK(hipMemsetAsync(nh.p, 0xff, need * 8, s));
    if (h->slots) {
      hipLaunchKernelGGL(cp_rehash_kernel, dim3((unsigned)std::min<uint64_t>((h->slots + 255) / 256, 4096)), dim3(256), 0, s,
                         h->hash.as<unsigned long long>(), h->entries.as<CpEntry>(), h->slots, nh.as<unsigned long long>(), ne.as<CpEntry>(),
                         need - 1, h->error.as<unsigned long long>());
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));   // (the old table is freed by the moves below)
    h->hash = std::move(nh);
    h->entries = std::move(ne);
    h->slots = need;
  }
  if (h->c[5] + bytes > h->arena_cap) {
    const uint64_t cap = std::max<uint64_t>(2 * h->arena_cap, h->c[5] + bytes);
    DevBuf na;
    HIPCHK(na.ensure(cap));
    if (h->c[5]) HIPCHK(hipMemcpyAsync(na.p, h->arena.p, h->c[5], hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    h->arena = std::move(na);
    h->arena_cap = cap;
  }
  HIPCHK(h->line_slots.ensure(lines * 8));
  return SLK_OK;
}

// room for `lines` more keys in a count map that holds `have`
static int32_t cp_map_room(slk_compare *h, hipStream_t s, PairMap &map, uint64_t have, uint64_t lines) {
  const uint64_t need = pow2_at_least(std::max<uint64_t>(2 * (have + lines), 1024));
  if (need <= map.cap) return SLK_OK;
  if (!map.cap || !have) return map.reset(s, need);
  PairMap old = std::move(map);
  map = PairMap();
  const int32_t rc = map.reset(s, need);
  if (rc) return rc;
  return old.grow_into<false>(s, map, nullptr, nullptr, h->status.as<int32_t>());   // (old is freed on return)
}

// One chunk of text on the device: the line passes, then the pass over the lines.  Synchronises s.
static int32_t cp_add(slk_compare *h, hipStream_t s, const uint8_t *d_text, uint64_t n, uint32_t id_col, uint32_t taxon_col, bool final,
                      bool reference, uint64_t *consumed) {
  *consumed = 0;
  if (n == 0) return SLK_OK;
  TpArgs L{};
  L.text = d_text;
  L.n = n;
  L.final = final ? 1 : 0;
  L.ntiles = (uint32_t)((n + TL_TILE - 1) / TL_TILE);
  HIPCHK(h->scratch.ensure(4 * ((uint64_t)L.ntiles + 1 + n + 2)));
  L.tiles = h->scratch.as<uint32_t>();
  L.S = L.tiles + ((uint64_t)L.ntiles + 1);
  const dim3 grid(std::min<unsigned>(L.ntiles, TL_MAX_GRID)), block(TL_BLOCK);
  hipLaunchKernelGGL(fq_lines_kernel<0>, grid, block, 0, s, L);
  hipLaunchKernelGGL(tp_scan_kernel, dim3(1), dim3(TL_SCAN_BLOCK), 0, s, L.tiles, (uint64_t)0, L.ntiles, (const uint32_t *)nullptr, 1u, 0u);
  hipLaunchKernelGGL(fq_lines_kernel<1>, grid, block, 0, s, L);
  HIPCHK(hipGetLastError());
  uint32_t M = 0, last_start = 0;
  uint8_t last = 0;
  HIPCHK(hipMemcpyAsync(&M, L.tiles + L.ntiles, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&last, d_text + (n - 1), 1, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (M == 0 || M > n) return fail(SLK_E_HIP, "compare: the line passes left %u lines for %llu bytes", M, (unsigned long long)n);
  // the lines that count: all of a final chunk; otherwise those whose terminator is inside and decided (a \r on the last byte is not)
  const bool whole = final || last == '\n';
  const uint32_t Lp = whole ? M : M - 1;
  uint64_t cons = n;
  if (!whole) {
    HIPCHK(hipMemcpyAsync(&last_start, L.S + (M - 1), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    cons = last_start;
  }
  if (Lp == 0) return SLK_OK;   // (consumed 0: the chunk must grow)
  int32_t rc = reference ? cp_make_room(h, s, Lp, n) : h->slots ? SLK_OK : cp_make_room(h, s, 0, 0);   // (a test without reference rows probes an empty table)
  if (!rc) rc = reference ? cp_map_room(h, s, h->ref_taxa, h->c[7], Lp) : cp_map_room(h, s, h->pairs, h->c[6], Lp);
  if (rc) return rc;
  CpArgs A{};
  A.text = d_text; A.n = n; A.S = L.S; A.Lp = Lp;
  A.id_col = id_col; A.taxon_col = taxon_col;
  A.base = reference ? h->ref_base : h->test_base;
  A.hash = h->hash.as<unsigned long long>(); A.entries = h->entries.as<CpEntry>(); A.mask = h->slots - 1;
  A.arena = h->arena.as<uint8_t>(); A.arena_cap = h->arena_cap;
  A.hash_mask = h->hash_mask;
  A.slots = h->line_slots.as<unsigned long long>();
  PairMap &map = reference ? h->ref_taxa : h->pairs;
  A.map_keys = map.k(); A.map_counts = map.c(); A.map_mask = map.cap - 1;
  A.counters = h->counters.as<unsigned long long>();
  A.error = h->error.as<unsigned long long>();
  const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)Lp + CP_BLOCK - 1) / CP_BLOCK, h->blocks);
  if (reference) {
    hipLaunchKernelGGL(cp_reference_kernel, dim3(blocks), dim3(CP_BLOCK), 0, s, A);
    hipLaunchKernelGGL(cp_duplicates_kernel, dim3(blocks), dim3(CP_BLOCK), 0, s, A);
  } else {
    hipLaunchKernelGGL(cp_test_kernel, dim3(blocks), dim3(CP_BLOCK), 0, s, A);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h->c, h->counters.p, sizeof h->c, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&h->err, h->error.p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (h->err != ~0ULL) {
    const unsigned kind = (unsigned)(h->err & 0xff);
    const unsigned long long at = h->err >> 8;
    if (kind == CP_INTERNAL) return fail(SLK_E_HIP, "compare: a structure sized for the chunk was full (internal)");
    if (kind == SLK_COMPARE_BAD_LINE)
      return fail(SLK_E_INVALID, "compare: the line at byte %llu of the %s text has too few columns, an empty id or taxon, or a taxon that is no "
                  "non-negative int", at, reference ? "reference" : "test");
    return fail(SLK_E_INVALID, "compare: the id of the line at byte %llu of the %s text occurs twice%s", at, reference ? "reference" : "test",
                reference ? " among the kept reference rows" : " among the joined test rows");
  }
  (reference ? h->ref_base : h->test_base) += cons;
  *consumed = cons;
  return SLK_OK;
}

static int32_t cp_check_text(uint64_t n, int32_t id_col, int32_t taxon_col) {
  if (n >= (1ULL << 32)) return fail(SLK_E_INVALID, "a compare call takes less than 2^32 bytes of text (%llu given): cut it into chunks", (unsigned long long)n);
  if (id_col < 1 || taxon_col < 1 || id_col == taxon_col) return fail(SLK_E_INVALID, "id column %d and taxon column %d must be two columns, counted from 1", id_col, taxon_col);
  return SLK_OK;
}

// device text (16-byte aligned)
static int32_t cp_add_device(slk_compare *h, slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t id_col, int32_t taxon_col, int32_t final,
                             bool reference, uint64_t *consumed) {
  if (!consumed) return fail(SLK_E_INVALID, "null argument");
  *consumed = 0;
  int32_t rc = enter_handle(h, CP_SPENT);
  if (rc) return rc;
  if (!st || (n && !d_text)) return fail(SLK_E_INVALID, "null argument");
  if (st->ix->device != h->device) return fail(SLK_E_INVALID, "the stream runs on another device than the handle");
  if ((rc = cp_check_text(n, id_col, taxon_col))) return rc;
  if ((uintptr_t)d_text % TL_LANE_BYTES) return fail(SLK_E_INVALID, "d_text must be aligned to %d bytes", TL_LANE_BYTES);
  rc = cp_add(h, st->s, d_text, n, (uint32_t)id_col - 1, (uint32_t)taxon_col - 1, final != 0, reference, consumed);
  return leave_handle(h, rc, rc != SLK_OK);
}

// host text
static int32_t cp_add_host(slk_compare *h, slk_stream *st, const uint8_t *text, uint64_t n, int32_t id_col, int32_t taxon_col, int32_t final,
                           bool reference, uint64_t *consumed) {
  if (!consumed) return fail(SLK_E_INVALID, "null argument");
  *consumed = 0;
  int32_t rc = enter_handle(h, CP_SPENT);
  if (rc) return rc;
  if (!st || (n && !text)) return fail(SLK_E_INVALID, "null argument");
  if (st->ix->device != h->device) return fail(SLK_E_INVALID, "the stream runs on another device than the handle");
  if ((rc = cp_check_text(n, id_col, taxon_col))) return rc;
  DrainOnExit drain(st);
  auto run = [&]() -> int32_t {
    HIPCHK(h->text.ensure(std::max<uint64_t>(n, 16)));
    int32_t r = copy_in(st, h->text.p, text, n);
    if (r == SLK_OK) r = cp_add(h, st->s, h->text.as<uint8_t>(), n, (uint32_t)id_col - 1, (uint32_t)taxon_col - 1, final != 0, reference, consumed);
    return r;
  };
  rc = run();
  return leave_handle(h, rc, rc != SLK_OK);
}

// the keys of a count map with their counts, ascending by key
static int32_t cp_read_map(slk_compare *h, const PairMap &map, std::vector<std::pair<uint64_t, uint64_t>> &rows) {
  rows.clear();
  if (!map.cap) return SLK_OK;
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint64_t> keys, counts;
  const int32_t rc = map.read(nullptr, keys, counts);
  if (rc) return rc;
  rows.resize(keys.size());
  for (size_t i = 0; i < keys.size(); i++) rows[i] = {keys[i], counts[i]};
  std::sort(rows.begin(), rows.end());
  return SLK_OK;
}

extern "C" {

int32_t slk_compare_create(slk_stream *st, slk_compare **out) {
  if (!out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (!st) return fail(SLK_E_INVALID, "null handle");
  int32_t rc = set_device(st->ix);
  if (rc) return rc;
  std::unique_ptr<slk_compare> h(new slk_compare());   // (released into *out on success only)
  h->ix = st->ix;
  h->device = st->ix->device;
  // SLK_COMPARE_BLOCKS: the grid (tests: a few blocks see more pairs than their LDS maps hold)
  h->blocks = grid_for(h->device, CP_BLOCKS_PER_CU, "SLK_COMPARE_BLOCKS");
  const long bits = std::min(64L, std::max(1L, env_long("SLK_COMPARE_HASH_BITS", 64)));
  h->hash_mask = bits >= 64 ? ~0ULL : (1ULL << bits) - 1;
  hipError_t e = h->counters.ensure(64);
  if (e == hipSuccess) e = h->error.ensure(8);
  if (e == hipSuccess) e = h->status.ensure(8);
  if (e == hipSuccess) e = hipMemset(h->counters.p, 0, 64);
  if (e == hipSuccess) e = hipMemset(h->error.p, 0xff, 8);
  if (e == hipSuccess) e = hipMemset(h->status.p, 0, 8);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(SLK_E_HIP, "compare: %s", hipGetErrorString(e)); }
  *out = h.release();
  return SLK_OK;
}

int32_t slk_compare_add_reference(slk_compare *h, slk_stream *st, const uint8_t *text, uint64_t n, int32_t id_col, int32_t taxon_col,
                                  int32_t final, uint64_t *consumed) {
  return cp_add_host(h, st, text, n, id_col, taxon_col, final, true, consumed);
}
int32_t slk_compare_add_reference_device(slk_compare *h, slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t id_col, int32_t taxon_col,
                                         int32_t final, uint64_t *consumed) {
  return cp_add_device(h, st, d_text, n, id_col, taxon_col, final, true, consumed);
}

int32_t slk_compare_begin_test(slk_compare *h) {
  int32_t rc = enter_handle(h, CP_SPENT);
  if (rc) return rc;
  auto run = [&]() -> int32_t {
    HIPCHK(hipDeviceSynchronize());   // whatever stream the adds were queued on
    if (h->slots) {
      hipLaunchKernelGGL(cp_clear_flags_kernel, dim3((unsigned)std::min<uint64_t>((h->slots + 255) / 256, 4096)), dim3(256), 0, nullptr,
                         h->hash.as<unsigned long long>(), h->entries.as<CpEntry>(), h->slots);
      HIPCHK(hipGetLastError());
    }
    if (h->pairs.cap) {
      const int32_t r = h->pairs.reset(nullptr, h->pairs.cap);
      if (r) return r;
    }
    h->c[3] = h->c[4] = h->c[6] = 0;
    HIPCHK(hipMemcpy(h->counters.p, h->c, sizeof h->c, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    h->test_base = 0;
    return SLK_OK;
  };
  rc = run();
  return leave_handle(h, rc, rc != SLK_OK);
}

int32_t slk_compare_add_test(slk_compare *h, slk_stream *st, const uint8_t *text, uint64_t n, int32_t final, uint64_t *consumed) {
  return cp_add_host(h, st, text, n, 2, 3, final, false, consumed);
}
int32_t slk_compare_add_test_device(slk_compare *h, slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t final, uint64_t *consumed) {
  return cp_add_device(h, st, d_text, n, 2, 3, final, false, consumed);
}

int32_t slk_compare_pairs(slk_compare *h, uint64_t *n, int32_t *ref_taxon, int32_t *test_taxon, uint64_t *count, uint64_t cap) {
  if (!n) return fail(SLK_E_INVALID, "null argument");
  *n = 0;
  if (cap && (!ref_taxon || !test_taxon || !count)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = enter_handle(h, CP_SPENT);
  if (rc) return rc;
  std::vector<std::pair<uint64_t, uint64_t>> rows;
  rc = cp_read_map(h, h->pairs, rows);
  if (rc) return leave_handle(h, rc, true);
  *n = rows.size();
  for (size_t i = 0; i < rows.size() && i < cap; i++) {
    ref_taxon[i] = (int32_t)(uint32_t)(rows[i].first >> 32);
    test_taxon[i] = (int32_t)(uint32_t)rows[i].first;
    count[i] = rows[i].second;
  }
  if (cap && cap < rows.size()) return fail(SLK_E_CAPACITY, "%llu pairs, capacity %llu", (unsigned long long)rows.size(), (unsigned long long)cap);
  return SLK_OK;
}

int32_t slk_compare_reference_taxa(slk_compare *h, uint64_t *n, int32_t *taxa, uint64_t *count, uint64_t cap) {
  if (!n) return fail(SLK_E_INVALID, "null argument");
  *n = 0;
  if (cap && (!taxa || !count)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = enter_handle(h, CP_SPENT);
  if (rc) return rc;
  std::vector<std::pair<uint64_t, uint64_t>> rows;
  rc = cp_read_map(h, h->ref_taxa, rows);
  if (rc) return leave_handle(h, rc, true);
  *n = rows.size();
  for (size_t i = 0; i < rows.size() && i < cap; i++) {
    taxa[i] = (int32_t)(uint32_t)rows[i].first;
    count[i] = rows[i].second;
  }
  if (cap && cap < rows.size()) return fail(SLK_E_CAPACITY, "%llu taxa, capacity %llu", (unsigned long long)rows.size(), (unsigned long long)cap);
  return SLK_OK;
}

int32_t slk_compare_totals(slk_compare *h, uint64_t *reference_rows, uint64_t *dropped_second, uint64_t *kept_ids, uint64_t *test_rows,
                           uint64_t *joined_rows) {
  if (!h) return fail(SLK_E_INVALID, "null handle");
  if (reference_rows) *reference_rows = h->c[0];
  if (dropped_second) *dropped_second = h->c[1];
  if (kept_ids) *kept_ids = h->c[2];
  if (test_rows) *test_rows = h->c[3];
  if (joined_rows) *joined_rows = h->c[4];
  return SLK_OK;
}

int32_t slk_compare_error(slk_compare *h, uint64_t *byte_offset, int32_t *kind) {
  if (!h) return fail(SLK_E_INVALID, "null handle");
  const bool have = h->err != ~0ULL && (h->err & 0xff) != CP_INTERNAL;
  if (byte_offset) *byte_offset = have ? h->err >> 8 : 0;
  if (kind) *kind = have ? (int32_t)(h->err & 0xff) : SLK_COMPARE_NO_ERROR;
  return SLK_OK;
}

void slk_compare_destroy(slk_compare *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}

}  // extern "C"
