// capi.hip -- what the C ABI declared in include/slacken_amd.h has beside its two halves (index.hip: the library side; stream.hip,
// classify.hip, shardstep.hip, hostcalls.hip: the classify side): error text, version, pinned host memory, the device count, and host arithmetic exported for tests.
// There is NO CPU fallback: without a gfx950 device every compute entry point fails with SLK_E_NO_GPU / SLK_E_HIP.
#include "hostside.h"
#include "../host/pack.hpp"

// (The slk_* functions below have C linkage from their declarations in include/slacken_amd.h; everything else is internal.)

const char *slk_last_error(void) { return g_err.c_str(); }
const char *slk_version(void) { return "slacken_amd 0.1 (gfx950)"; }

// Pinned host memory: buffers the host entry points can DMA from and to directly, without the staging copy.
int32_t slk_host_alloc(size_t bytes, void **out) {
  if (!out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  void *p = nullptr;   // (the caller's from here on: slk_host_free)
  HIPCHK(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault));
  pinned().add(p, bytes ? bytes : 1, true);
  *out = p;
  return SLK_OK;
}
int32_t slk_host_register(void *ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(SLK_E_INVALID, "null argument");
  HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  pinned().add(ptr, bytes, false);
  return SLK_OK;
}
int32_t slk_host_free(void *ptr) {  // memory of slk_host_alloc is freed, memory of slk_host_register is unpinned
  if (!ptr) return SLK_OK;
  bool owned = false;
  if (!pinned().remove(ptr, &owned)) return fail(SLK_E_INVALID, "not a pointer of slk_host_alloc / slk_host_register");
  if (owned) HIPCHK(hipHostFree(ptr));
  else HIPCHK(hipHostUnregister(ptr));
  return SLK_OK;
}

int32_t slk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// The table's range reduction and its inverse as plain host arithmetic (engine.h: table_slot / table_hash_of), for tests.
static TableGeom geom_for_tests(uint64_t nbuckets) {
  TableGeom g{};
  g.nbuckets = nbuckets;
  g.q = std::max(5, ceil_log2_u64(nbuckets));
  g.rem_mask = (1ULL << (64 - g.q)) - 1;
  return g;
}
int32_t slk_table_slot(uint64_t nbuckets, uint64_t hash, uint32_t *home, uint64_t *rem) {
  if (nbuckets < 32 || nbuckets > (1ULL << 32) || !home || !rem) return fail(SLK_E_INVALID, "32 <= nbuckets <= 2^32");
  table_slot(geom_for_tests(nbuckets), hash, *home, *rem);
  return SLK_OK;
}
int32_t slk_table_hash_of(uint64_t nbuckets, uint32_t home, uint64_t rem, uint64_t *hash) {
  if (nbuckets < 32 || nbuckets > (1ULL << 32) || home >= nbuckets || !hash) return fail(SLK_E_INVALID, "32 <= nbuckets <= 2^32, home < nbuckets");
  *hash = table_hash_of(geom_for_tests(nbuckets), home, rem);
  return SLK_OK;
}

uint32_t slk_shard_of(int64_t key, uint32_t n_shards) {
  return n_shards ? (uint32_t)(fmix64((uint64_t)key) % n_shards) : 0;
}


// rows of the batch log (engine.h: ShardIO.batch_base) a batch needs: tile t starts at row floor(span_region(64 t) / 64) + t
uint64_t slk_shard_batch_rows(uint64_t total_bases, uint64_t total_mate_bases, uint64_t R, int32_t paired) {
  return (span_slots(total_bases, total_mate_bases, R, paired != 0) >> 6) + (R + 63) / 64 + 2;
}

// entries a wave reserves at a time in an owner's send region (engine.h: ShardIO.chunk): one atomic per chunk and owner on ONE
// address per owner, so the fewer owners the larger the chunk (an owner's keys come 1 / n_shards as fast); what stays unwritten at
// the end of a launch is half a chunk per wave and owner -- 2 M entries of the 390 M of a 10 M-read batch whatever n_shards is
uint32_t slk_shard_chunk(uint32_t n_shards) {
  uint32_t c = 1024;
  while (c > 64 && c * n_shards > 1024) c >>= 1;
  return c;
}

// n bases -> codes[ceil(n / 16)], valid[ceil(n / 16)] (host/pack.hpp), on the library's copy threads.  Host arithmetic: no GPU.
int32_t slk_pack_bases(const uint8_t *bases, uint64_t n, uint32_t *codes, uint16_t *valid) {
  if (n && (!bases || !codes || !valid)) return fail(SLK_E_INVALID, "null argument");
  const uint64_t SLICE = (uint64_t)1 << 22;   // (a multiple of 32 bases: slices start on word borders)
  const uint64_t parts = (n + SLICE - 1) / SLICE;
  if (parts <= 1) { pack_bases(bases, n, codes, valid); return SLK_OK; }
  host_pool().parallel_for(parts, [&](size_t i) {
    const uint64_t a = i * SLICE, b = std::min(n, a + SLICE);
    pack_bases(bases + a, b - a, codes + a / 16, valid + a / 16);
  });
  return SLK_OK;
}

// The same codes, the validity as the list of the words that hold an invalid base (slk_reads: exc_word / exc_bits).  Large inputs
// are cut as above; a slice keeps its exceptions to itself until all are through, then they are written in order.
int32_t slk_pack_bases_sparse(const uint8_t *bases, uint64_t n, uint32_t *codes, uint32_t *exc_word, uint16_t *exc_bits, uint64_t exc_capacity,
                              uint64_t *n_exc) {
  if (!n_exc || (n && (!bases || !codes)) || (exc_capacity && (!exc_word || !exc_bits))) return fail(SLK_E_INVALID, "null argument");
  *n_exc = 0;
  if ((n + 15) / 16 > (1ULL << 32)) return fail(SLK_E_INVALID, "exception words are 32-bit indices: at most 2^36 bases per call");
  const uint64_t SLICE = (uint64_t)1 << 22;
  const uint64_t parts = (n + SLICE - 1) / SLICE;
  uint64_t need = 0;
  if (parts <= 1) {
    need = pack_bases_sparse(bases, n, 0, codes, exc_word, exc_bits, 0, exc_capacity);
  } else {
    std::vector<std::vector<uint32_t>> words(parts);
    std::vector<std::vector<uint16_t>> bits(parts);
    host_pool().parallel_for(parts, [&](size_t i) {
      const uint64_t a = i * SLICE, b = std::min(n, a + SLICE);
      const uint64_t most = (b - a + 15) / 16;   // (room for every word while the slice is packed, cut back to what it listed)
      words[i].resize(most); bits[i].resize(most);
      const uint64_t cnt = pack_bases_sparse(bases + a, b - a, a / 16, codes + a / 16, words[i].data(), bits[i].data(), 0, most);
      words[i].resize(cnt); bits[i].resize(cnt);
      words[i].shrink_to_fit(); bits[i].shrink_to_fit();
    });
    for (uint64_t i = 0; i < parts; i++)
      for (size_t j = 0; j < words[i].size(); j++, need++)
        if (need < exc_capacity) { exc_word[need] = words[i][j]; exc_bits[need] = bits[i][j]; }
  }
  *n_exc = need;
  if (need > exc_capacity) return fail(SLK_E_CAPACITY, "%llu exception words, capacity is %llu", (unsigned long long)need, (unsigned long long)exc_capacity);
  return SLK_OK;
}
