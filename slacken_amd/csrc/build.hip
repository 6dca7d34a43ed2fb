// build.hip -- library construction on the device: minimizers of taxon-labelled sequences, merged by LCA, straight into the
// HBM record table.  Replaces, for one batch of sequences, the reference's
//   SplitterMinimizers.find            S/slacken/Minimizers.scala:43-76   (every super-mer's minimizer, labelled with the taxon)
//   groupBy(id columns).agg(TaxonLCA)  S/slacken/KeyValueIndex.scala:85-93, S/slacken/LowestCommonAncestor.scala:152-170
// (S/ = src/main/scala/com/jnpersson/ in the reference).  The group-by needs no sort here: the table is the group-by.  A
// record is inserted with atomicCAS, and a key that is already present has its taxon replaced by LCA(old, new) in a CAS loop.
// LCA is associative and commutative on a rooted tree, so the final taxon of every key is independent of the order in which
// lanes, waves and batches arrive; only the cell a record occupies may differ between runs, which no lookup can observe.
//
// Work decomposition: the host cuts every sequence into chunks of CHUNK_WINDOWS k-mer windows that overlap by k-1 bases (the
// same overlap the reference's indexed-FASTA reader uses, FileInputs.scala:240-262): the SET of window minimizers is unchanged.
// One lane per chunk, 64 chunks per wave in lockstep (chunkscan.h, without priming); minimizers go to a wave-shared LDS queue
// (wavetools.h: WaveQueue) and are inserted 64 at a time, one lane per record, so that the latency of the atomics is paid once per
// 64 records.
#include <hip/hip_runtime.h>

#include "chunkscan.h"
#include "tablebuild.h"

namespace slk {

namespace {

constexpr int BW = 4;  // waves per block

struct BuildLds {
  uint64_t q_key[BW][128];
  int32_t q_tax[BW][128];
};

__global__ void __launch_bounds__(BW * 64) build_kernel(ScanParams P, TableBuild T, const int32_t *__restrict__ parents,
                                                        int32_t ntax, const uint8_t *__restrict__ bases, uint64_t total_bases,
                                                        const uint64_t *__restrict__ chunk_start,
                                                        const uint32_t *__restrict__ chunk_len,
                                                        const int32_t *__restrict__ chunk_taxon, uint64_t nchunks) {
  extern __shared__ uint64_t ring[];  // [w][BW*64]: the last w keys of every lane
  __shared__ BuildLds L;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t stride = BW * 64;
  const int w = P.w;
  const uint64_t c = (uint64_t)blockIdx.x * stride + tid;
  const uint32_t len = c < nchunks ? chunk_len[c] : 0;
  const uint64_t start = c < nchunks ? chunk_start[c] : 0;
  const int32_t taxon = c < nchunks ? chunk_taxon[c] : 0;
  const uint32_t maxlen = wave_max32(len);

  ChunkScan S(w);
  WaveQueue<int32_t> Q(L.q_key[wib], L.q_tax[wib], lane);
  int created = 0, failed = 0, max_d = 0;  // per lane

  auto insert = [&](uint32_t e, bool active) {   // the queued records, one per lane
    if (!active) return;
    int r = insert_merge(T, parents, ntax, L.q_key[wib][e], L.q_tax[wib][e], max_d);
    created += (r == 1);
    failed += (r < 0);
  };

  for (uint32_t step = 0; step < maxlen; step++) {   // a new super-mer starts: one record candidate
    const bool emit = S.step(P, ring, stride, tid, bases, start, total_bases, step, len, false) == ChunkScan::FRESH;
    Q.push(emit, S.cur_val, taxon, insert);
  }
  Q.drain(insert);

  report_inserts(T, lane, created, failed, max_d);
}

// Every occupied cell back to its (key, taxon) record: the cell holds the hash remainder and its displacement, the bucket
// index gives the home bucket, and both the range reduction (engine.h: table_hash_of) and fmix64 are invertible.
__global__ void __launch_bounds__(256) export_kernel(TableView T, uint64_t cell0, uint64_t ncells, int64_t *__restrict__ keys,
                                                     int32_t *__restrict__ taxa, uint64_t capacity,
                                                     unsigned long long *__restrict__ counter) {
  uint64_t i;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t tmask = (1ULL << T.g.taxon_bits) - 1;
  for (uint64_t base = cell0 + (uint64_t)blockIdx.x * blockDim.x; base < ncells; base += step) {  // wave-uniform trip count
    i = base + threadIdx.x;
    uint64_t cell = i < ncells ? T.cells[i] : 0;
    const bool has = cell != 0;
    const unsigned long long slot = wave_alloc_slots(has, counter);   // one atomic per wave: the lanes' output slots are consecutive
    if (!has) continue;
    if (slot < capacity) {
      keys[slot] = (int64_t)cell_key(T.g, i, cell);
      taxa[slot] = ext_taxon(T, (int32_t)(cell & tmask));
    }
  }
}

}  // namespace

void launch_build(const ScanParams &P, const TableBuild &T, const int32_t *parents, int32_t ntax, const uint8_t *bases,
                  uint64_t total_bases, const uint64_t *chunk_start, const uint32_t *chunk_len, const int32_t *chunk_taxon, uint64_t nchunks,
                  hipStream_t s) {
  if (nchunks == 0) return;
  const unsigned block = BW * 64;
  size_t lds = (size_t)block * P.w * 8;
  uint64_t blocks = (nchunks + block - 1) / block;
  hipLaunchKernelGGL(build_kernel, dim3((unsigned)blocks), dim3(block), lds, s, P, T, parents, ntax, bases, total_bases,
                     chunk_start, chunk_len, chunk_taxon, nchunks);
}

void launch_export(const TableView &T, uint64_t nbuckets, int64_t *keys, int32_t *taxa, uint64_t capacity,
                   unsigned long long *counter, hipStream_t s) {
  launch_export_range(T, 0, nbuckets, keys, taxa, capacity, counter, s);
}
// the records of buckets [bucket0, bucket1) (a table that is being moved to a larger one goes there piece by piece)
void launch_export_range(const TableView &T, uint64_t bucket0, uint64_t bucket1, int64_t *keys, int32_t *taxa, uint64_t capacity,
                         unsigned long long *counter, hipStream_t s) {
  if (bucket1 <= bucket0) return;
  const uint64_t cell0 = bucket0 * CELLS, ncells = bucket1 * CELLS;
  uint64_t blocks = std::min<uint64_t>((ncells - cell0 + 255) / 256, 256 * 64);
  hipLaunchKernelGGL(export_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T, cell0, ncells, keys, taxa, capacity, counter);
}

}  // namespace slk
