// bracken.hip -- Bracken weights: BrackenWeights.buildWeights (S/slacken/BrackenWeights.scala:294-352).  Every read of length L
// at every position of every genome is classified against the index and counted by (source taxon, destination taxon).
//
// A batch of pieces (splitToMaxLength :152-164, cut on the host) goes through four launches on the slk_stream:
//   scan     slk_scan_device (getSpans): the super-mers of every piece with their k-mer counts and distinct flags
//   lookup   the staged probe (kernels.hip: launch_probe): the taxon of every super-mer, NONE when the minimizer has no record
//   expand   one lane per piece: the hit list of taxonHits (:198-233) laid out per k-mer position (taxon + hit-group flags), the
//            piece's reproduced ordinal quirk and the deficit it leaves at each chunk start
//   window   one lane per chunk of BR_CHUNK consecutive read starts: FragmentWindow (:46-137) slid over the chunk, resolveTree
//            (LowestCommonAncestor.scala:101-146) on a change only, run lengths of equal destinations added into a device hash map
// A lane whose window holds more than BR_MAPCAP taxa hands the rest of its chunk to a second launch of the same code with its map
// in HBM (capacity W + 1: a window cannot hold more taxa than k-mers).
#include "hostside.h"
#include "pairmap.h"

namespace {

constexpr int BR_BLOCK = 64;          // window kernel: one wave per block
constexpr int BR_MAPCAP = 16;         // taxa of one lane's window map in LDS
constexpr uint32_t BR_CHUNK = 512;    // read starts per lane
constexpr uint8_t KF_START = 1, KF_IN = 2, KF_END = 4;  // k-mer flags: first / any / last k-mer of a distinct non-NONE super-mer

__device__ __forceinline__ bool br_is_base(uint8_t c) {  // Supermers.nonAmbiguousRegex without whitespace (removed upstream, :311)
  switch (c | 0x20) {
    case 'a': case 'c': case 'g': case 't': case 'u': return true;
    default: return false;
  }
}

struct BrArgs {
  const uint8_t *bases;
  const uint64_t *offsets;
  uint64_t R;
  int32_t k, W, read_len;
  const int32_t *span_meta, *span_taxon, *span_count;
  int32_t *ktax;        // [total bases]: taxon of the k-mer starting there (NONE: no valid k-mer / trailing / ambiguous)
  uint8_t *kflag;       // [total bases]: KF_* of that k-mer
  int32_t *qtax;        // [R]: taxon whose entering k-mers [W, qend) are credited to NONE (0 = no quirk in this piece)
  uint32_t *qend;       // [R]
  const uint64_t *chunk0;      // [R]: first chunk of the piece
  const int32_t *source;       // [R]
  const uint32_t *chunk_piece; // [nchunks]
  uint64_t nchunks;
  int32_t *deficit;     // [nchunks]: true minus literal count of qtax at the chunk's first read start
  const uint4 *nodes;   // {parent, tin, tout, -} of the caller's ids (index.hip: build_tax_nodes)
  int32_t T;
  unsigned long long *map_keys, *map_counts;  // (source << 32 | dest) -> reads; power-of-two capacity
  uint64_t map_mask;
  uint4 *overflow;      // [nchunks]: {piece, first read start, end, deficit} handed to the HBM-map launch
  unsigned int *n_overflow;
  int32_t *status;      // bit 0: inconsistent span list, bit 1: the (source, dest) map is full
};

// ---------------------------------------------------------------------------------------------------------------
// expand: one lane per piece
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bracken_expand_kernel(BrArgs A) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.R) return;
  const uint64_t o = A.offsets[r];
  const uint32_t n = (uint32_t)(A.offsets[r + 1] - o);
  const uint8_t *seq = A.bases + o;
  int32_t *kt = A.ktax + o;
  uint8_t *kf = A.kflag + o;
  const int32_t *meta = A.span_meta + o, *stax = A.span_taxon + o;   // span_region(offsets, nullptr, r) == offsets[r]
  const int32_t ns = A.span_count[r];
  const uint32_t k = (uint32_t)A.k, W = (uint32_t)A.W;
  A.qtax[r] = 0;
  A.qend[r] = 0;
  int32_t j = 0, qt = 0;
  uint32_t qe = 0, i = 0;
  while (i < n) {
    uint32_t e = i;
    while (e < n && br_is_base(seq[e])) e++;
    if (e - i >= k) {
      // SEQUENCE segment [i, e): its super-mers tile k-mers [i, t0), then TaxonHit(false, e - i - (k-1), NONE, k-1) (:230)
      const uint32_t t0 = e - k + 1;
      uint32_t p = i, last_start = i;
      int32_t last_tax = 0;
      while (p < t0) {
        while (j < ns && meta_flag(meta[j]) != 1) j++;   // the scanner's AMBIGUOUS spans: the hits come from the positions
        if (j >= ns) { atomicOr(A.status, 1); return; }
        const int32_t m = meta[j], c = meta_kmers(m), t = stax[j];
        j++;
        if (c < 1 || (uint32_t)c > t0 - p) { atomicOr(A.status, 1); return; }
        const bool hg = meta_distinct(m) && t != 0;       // numHitGroups counts distinct && taxon != NONE (:84-90)
        for (int32_t q = 0; q < c; q++) {
          kt[p + q] = t;
          kf[p + q] = hg ? (uint8_t)((q == 0 ? KF_START : 0) | KF_IN | (q == c - 1 ? KF_END : 0)) : 0;
        }
        last_tax = t; last_start = p;
        p += (uint32_t)c;
      }
      for (; p < e; p++) { kt[p] = 0; kf[p] = 0; }
      // The trailing hit's ordinal lacks the segment's position (:230).  When it falls in the first window (hits.span, :76-80)
      // while the segment's last super-mer reaches past it, the k-mers [W, t0) of that super-mer are credited to NONE as they
      // enter (advance(), :126-131).  At most one segment of a piece can do this: the one whose last super-mer covers k-mer W.
      if (i > 0 && last_start < W && t0 > W && t0 - i < W) { qt = last_tax; qe = t0; }
    } else {
      if (e == i) while (e < n && !br_is_base(seq[e])) e++;
      for (uint32_t p = i; p < e; p++) { kt[p] = 0; kf[p] = 0; }   // AMBIGUOUS segments of any length: NONE (:232-235)
    }
    i = e;
  }
  A.qtax[r] = qt;
  A.qend[r] = qe;
  const uint32_t L = (uint32_t)A.read_len;
  if (qt == 0 || n < L) return;
  // The literal count of qt follows c <- max(c - dec, 0) + inc (the map drops a key at <= 0, :117-121); the true count does
  // not clamp.  Their difference at each chunk start seeds the window lanes.  Once it is 0 and no stolen k-mer is left to
  // enter, it stays 0 (the buffer was cleared).
  const uint32_t nr = n - L + 1;
  int32_t ct = 0, D = 0;
  for (uint32_t q = 0; q < W; q++) ct += kt[q] == qt;
  const uint64_t c0 = A.chunk0[r];
  for (uint32_t p = 0;; p++) {
    if (p % BR_CHUNK == 0) A.deficit[c0 + p / BR_CHUNK] = D;
    if (p + 1 >= nr || (D == 0 && p + W >= qe)) break;
    const int32_t dec = kt[p] == qt, inc = kt[p + W] == qt;
    const bool stolen = p + W < qe;
    int32_t cl = ct - D - dec;
    cl = (cl < 0 ? 0 : cl) + ((inc && !stolen) ? 1 : 0);
    ct += inc - dec;
    D = ct - cl;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// window: one lane per chunk of read starts
// ---------------------------------------------------------------------------------------------------------------
struct MapRef {   // Int2IntArrayMap countSummary (:59): {taxon, count, tin, tout} per slot, slot s at e[s * stride]
  int4 *e;
  uint32_t stride;
  int32_t cap, n;
  __device__ __forceinline__ int4 &at(int32_t s) { return e[(uint32_t)s * stride]; }
  __device__ __forceinline__ int32_t find(int32_t t) {
    for (int32_t s = 0; s < n; s++) if (at(s).x == t) return s;
    return -1;
  }
};

// countSummary.put(t, applyAsInt(t) + 1); false when the map is full
__device__ __forceinline__ bool br_inc(const BrArgs &A, MapRef &M, int32_t t) {
  const int32_t s = M.find(t);
  if (s >= 0) { M.at(s).y++; return true; }
  if (M.n == M.cap) return false;
  const uint4 nd = tax_node(A.nodes, A.T, t);
  M.at(M.n++) = make_int4(t, 1, (int32_t)nd.y, (int32_t)nd.z);
  return true;
}

// updated = applyAsInt(t) - 1; if (updated > 0) put else remove (:117-121)
__device__ __forceinline__ void br_dec(MapRef &M, int32_t t, int32_t by) {
  const int32_t s = M.find(t);
  if (s < 0) return;
  const int32_t c = M.at(s).y - by;
  if (c > 0) M.at(s).y = c;
  else { M.at(s) = M.at(M.n - 1); M.n--; }
}

// MapRef as resolve.h reads it (NONE is not in the map)
struct BrMapView {
  const int4 *e;
  uint32_t stride;
  int32_t len;
  __device__ __forceinline__ int n() const { return len; }
  __device__ __forceinline__ int32_t taxon(int j) const { return e[(uint32_t)j * stride].x; }
  __device__ __forceinline__ int32_t count(int j) const { return e[(uint32_t)j * stride].y; }
  __device__ __forceinline__ uint32_t tin(int j) const { return (uint32_t)e[(uint32_t)j * stride].z; }
  __device__ __forceinline__ uint32_t tout(int j) const { return (uint32_t)e[(uint32_t)j * stride].w; }
  __device__ __forceinline__ bool live(int) const { return true; }
};

// resolveTree(countSummary, 0.0) (:101-146 via :276-285): the LCA of the taxa of maximal root-path score (resolve.h, step 1); with a
// required score of 0 the lifting loop never runs.  NONE scores 0 and is not in the map.
__device__ int32_t br_resolve(const BrArgs &A, MapRef &M) {
  if (M.n == 0) return 0;
  if (M.n == 1) return M.at(0).x;
  return resolve_best(BrMapView{M.e, M.stride, M.n}, tax_tour(A.nodes, A.T)).taxon;
}

__device__ __forceinline__ void br_flush(const BrArgs &A, int32_t source, int32_t dest, uint64_t reads) {
  if (reads == 0) return;
  const unsigned long long key = ((unsigned long long)(uint32_t)source << 32) | (uint32_t)dest;
  if (!pair_map_add(A.map_keys, A.map_counts, A.map_mask, key, (unsigned long long)reads, nullptr)) atomicOr(A.status, 2);
}

// Reads [p0, p1) of piece r, starting from the literal state of read p0 (true window counts, qtax short by D0).  count_first =
// false: read p0 was counted by the lane that handed over.  Returns true when done; false when the map ran out of room, with the
// hand-over in *job: {piece, read start, p1, deficit at that read | counted << 31}.
__device__ bool br_run(const BrArgs &A, MapRef &M, uint64_t r, uint32_t p0, uint32_t p1, int32_t D0, bool count_first, uint4 *job) {
  const uint64_t o = A.offsets[r];
  const int32_t *kt = A.ktax + o;
  const uint8_t *kf = A.kflag + o;
  const uint32_t W = (uint32_t)A.W;
  const int32_t qt = A.qtax[r];
  const uint32_t qe = A.qend[r];
  const int32_t source = A.source[r];
  M.n = 0;
  int32_t hg = ((kf[p0] & KF_IN) && !(kf[p0] & KF_START)) ? 1 : 0;   // a hit group that began before the window
  for (uint32_t q = p0; q < p0 + W; q++) {
    const int32_t t = kt[q];
    hg += (kf[q] & KF_START) ? 1 : 0;
    if (t != 0 && !br_inc(A, M, t)) { *job = make_uint4((uint32_t)r, p0, p1, (uint32_t)D0 | (count_first ? 0u : 1u << 31)); return false; }
  }
  if (D0 > 0) br_dec(M, qt, D0);
  int32_t res = br_resolve(A, M);
  int32_t cur = hg >= 2 ? res : 0;                                       // classify (:276-285): minHitGroups = 2
  uint64_t run = count_first ? 1 : 0;
  for (uint32_t p = p0 + 1; p < p1; p++) {
    const uint32_t leave = p - 1, enter = p - 1 + W;
    const int32_t tl = kt[leave];
    const int32_t te = (qt != 0 && enter < qe) ? 0 : kt[enter];         // a stolen k-mer enters as NONE
    hg += ((kf[enter] & KF_START) ? 1 : 0) - ((kf[leave] & KF_END) ? 1 : 0);
    if (tl != te || (tl != 0 && tl == qt)) {
      if (te != 0 && M.n == M.cap && M.find(te) < 0) {
        // no room (perhaps: tl may still leave): hand over from read p - 1, already counted, with its deficit
        int32_t D = 0;
        if (qt != 0) {
          int32_t ct = 0;
          for (uint32_t q = leave; q < leave + W; q++) ct += kt[q] == qt;
          const int32_t s = M.find(qt);
          D = ct - (s >= 0 ? M.at(s).y : 0);
        }
        br_flush(A, source, cur, run);
        *job = make_uint4((uint32_t)r, leave, p1, (uint32_t)D | (1u << 31));
        return false;
      }
      if (tl != 0) br_dec(M, tl, 1);
      if (te != 0) br_inc(A, M, te);
      res = br_resolve(A, M);
    }
    const int32_t dest = hg >= 2 ? res : 0;
    if (dest != cur) { br_flush(A, source, cur, run); cur = dest; run = 1; }
    else run++;
  }
  br_flush(A, source, cur, run);
  return true;
}

__global__ void __launch_bounds__(BR_BLOCK) bracken_window_kernel(BrArgs A) {
  __shared__ int4 lds[BR_MAPCAP * BR_BLOCK];
  MapRef M;
  M.e = &lds[threadIdx.x];
  M.stride = BR_BLOCK;
  M.cap = BR_MAPCAP;
  const uint64_t nl = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < A.nchunks; c += nl) {
    const uint32_t r = A.chunk_piece[c];
    const uint32_t n = (uint32_t)(A.offsets[r + 1] - A.offsets[r]);
    const uint32_t nr = n - (uint32_t)A.read_len + 1;
    const uint32_t p0 = (uint32_t)(c - A.chunk0[r]) * BR_CHUNK;
    const uint32_t p1 = min(p0 + BR_CHUNK, nr);
    uint4 job;
    if (!br_run(A, M, r, p0, p1, A.deficit[c], true, &job)) A.overflow[atomicAdd(A.n_overflow, 1u)] = job;
  }
}

__global__ void __launch_bounds__(256) bracken_window_hbm_kernel(BrArgs A, uint64_t n, int4 *scratch) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 job = A.overflow[i];
  MapRef M;
  M.e = scratch + i * (uint64_t)(A.W + 1);
  M.stride = 1;
  M.cap = A.W + 1;
  uint4 again;
  (void)br_run(A, M, job.x, job.y, job.z, (int32_t)(job.w & 0x7fffffffu), (job.w >> 31) == 0, &again);   // cap W + 1: never full
}

}  // namespace

struct slk_bracken {
  slk_index *ix = nullptr;
  int32_t read_len = 0, W = 0;
  uint64_t max_fragment = 0;
  PairMap map;   // (source << 32 | dest) -> reads
  DevBuf status;
  DevBuf bases, offsets, span_keys, span_meta, span_taxon, span_count, ktax, kflag, qtax, qend, chunk0, source, chunk_piece,
      deficit, overflow, n_overflow, scratch;
  uint64_t batch_bytes = 1ULL << 30;   // bases per batch (SLK_BRACKEN_BATCH_MB): about 22 bytes of HBM each
  // the batch being assembled on the host
  std::vector<uint8_t> h_bases;
  std::vector<uint64_t> h_offsets, h_chunk0;
  std::vector<int32_t> h_source;
  std::vector<uint32_t> h_chunk_piece;
  bool spent = false;   // a batch failed: the map holds part of it, so no count of this handle can be trusted any more
};

static void br_clear_batch(slk_bracken *b) {
  b->h_bases.clear();
  b->h_offsets.assign(1, 0);
  b->h_chunk0.clear();
  b->h_source.clear();
  b->h_chunk_piece.clear();
}

static int32_t br_run_batch_device(slk_bracken *b, slk_stream *st) {
  const uint64_t R = b->h_source.size();
  if (R == 0) return SLK_OK;
  slk_index *ix = b->ix;
  hipStream_t s = st->s;
  const uint64_t total = b->h_offsets[R];
  const uint64_t nchunks = b->h_chunk_piece.size();
  HIPCHK(b->bases.ensure(total + 16));
  HIPCHK(b->offsets.ensure((R + 1) * 8));
  HIPCHK(b->span_keys.ensure((total + 1) * 8));
  HIPCHK(b->span_meta.ensure((total + 1) * 4));
  HIPCHK(b->span_taxon.ensure((total + 1) * 4));
  HIPCHK(b->span_count.ensure(R * 4));
  HIPCHK(b->ktax.ensure(total * 4 + 4));
  HIPCHK(b->kflag.ensure(total + 16));
  HIPCHK(b->qtax.ensure(R * 4));
  HIPCHK(b->qend.ensure(R * 4));
  HIPCHK(b->chunk0.ensure(R * 8));
  HIPCHK(b->source.ensure(R * 4));
  HIPCHK(b->chunk_piece.ensure(nchunks * 4 + 4));
  HIPCHK(b->deficit.ensure(nchunks * 4 + 4));
  HIPCHK(b->overflow.ensure(nchunks * 16 + 16));
  HIPCHK(b->n_overflow.ensure(8));
  HIPCHK(hipMemcpyAsync(b->bases.p, b->h_bases.data(), total, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b->offsets.p, b->h_offsets.data(), (R + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b->chunk0.p, b->h_chunk0.data(), R * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b->source.p, b->h_source.data(), R * 4, hipMemcpyHostToDevice, s));
  if (nchunks) HIPCHK(hipMemcpyAsync(b->chunk_piece.p, b->h_chunk_piece.data(), nchunks * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(b->deficit.p, 0, nchunks * 4 + 4, s));
  HIPCHK(hipMemsetAsync(b->n_overflow.p, 0, 8, s));

  BrArgs A{};
  A.bases = b->bases.as<uint8_t>(); A.offsets = b->offsets.as<uint64_t>(); A.R = R;
  A.k = ix->params.k; A.W = b->W; A.read_len = b->read_len;
  A.span_meta = b->span_meta.as<int32_t>(); A.span_taxon = b->span_taxon.as<int32_t>(); A.span_count = b->span_count.as<int32_t>();
  A.ktax = b->ktax.as<int32_t>(); A.kflag = b->kflag.as<uint8_t>(); A.qtax = b->qtax.as<int32_t>(); A.qend = b->qend.as<uint32_t>();
  A.chunk0 = b->chunk0.as<uint64_t>(); A.source = b->source.as<int32_t>(); A.chunk_piece = b->chunk_piece.as<uint32_t>();
  A.nchunks = nchunks; A.deficit = b->deficit.as<int32_t>();
  A.nodes = ix->d_nodes_orig; A.T = ix->T;
  A.map_keys = b->map.k(); A.map_counts = b->map.c(); A.map_mask = b->map.cap - 1;
  A.overflow = b->overflow.as<uint4>(); A.n_overflow = b->n_overflow.as<unsigned int>(); A.status = b->status.as<int32_t>();

  // getSpans as slk_scan_device computes it (the fused wave-per-fragment scan where the window allows, else kernels.hip's)
  int32_t rc = slk_scan_device(ix, st, A.bases, A.offsets, nullptr, nullptr, R, b->span_keys.as<uint64_t>(), b->span_meta.as<int32_t>(),
                               b->span_count.as<int32_t>());
  if (rc) return rc;
  launch_probe(ix->view(), A.offsets, nullptr, R, b->span_keys.as<uint64_t>(), A.span_meta, A.span_count, b->span_taxon.as<int32_t>(), s);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(bracken_expand_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, A);
  HIPCHK(hipGetLastError());
  if (nchunks) {
    uint64_t blocks = (nchunks + BR_BLOCK - 1) / BR_BLOCK;
    if (blocks > 256 * 40) blocks = 256 * 40;
    hipLaunchKernelGGL(bracken_window_kernel, dim3((unsigned)blocks), dim3(BR_BLOCK), 0, s, A);
    HIPCHK(hipGetLastError());
  }
  unsigned int nov = 0;
  int32_t status = 0;
  HIPCHK(hipMemcpyAsync(&nov, b->n_overflow.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&status, b->status.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (status & 1) return fail(SLK_E_HIP, "bracken: the scanner's spans do not tile a piece (internal error)");
  if (nov) {
    HIPCHK(b->scratch.ensure((uint64_t)nov * (uint64_t)(b->W + 1) * 16));
    hipLaunchKernelGGL(bracken_window_hbm_kernel, dim3((unsigned)((nov + 255) / 256)), dim3(256), 0, s, A, (uint64_t)nov,
                       b->scratch.as<int4>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&status, b->status.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (status & 2)
    return fail(SLK_E_CAPACITY, "bracken: more (source, dest) pairs than the map holds (%llu; SLK_BRACKEN_MAP_LOG2)",
                (unsigned long long)b->map.cap);
  return SLK_OK;
}

// Runs the batch assembled on the host and empties it, whatever the outcome.  A batch that failed has added an unknown part of its
// runs to the map: the handle is spent, and slk_bracken_add / slk_bracken_result refuse it from then on.
static int32_t br_run_batch(slk_bracken *b, slk_stream *st) {
  const int32_t rc = br_run_batch_device(b, st);
  br_clear_batch(b);
  if (rc) b->spent = true;
  return rc;
}

static int32_t br_check_spent(const slk_bracken *b) {
  if (b->spent) return fail(SLK_E_STATE, "bracken: an earlier slk_bracken_add failed, the counts of this handle are incomplete");
  return SLK_OK;
}

extern "C" {

int32_t slk_bracken_create(slk_index *ix, int32_t read_len, uint64_t max_fragment, slk_bracken **out) {
  if (!out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (!ix) return fail(SLK_E_INVALID, "null handle");
  if (!ix->finalized) return fail(SLK_E_STATE, "index is not finalized");
  if (!ix->d_parents) return fail(SLK_E_STATE, "taxonomy not set");
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "Bracken weights support minimizers of up to 32 nt (one id column)");
  if (!ix->d_nodes_orig) return fail(SLK_E_UNSUPPORTED, "Bracken weights need a taxonomy of at most 2^26 ids");
  if (read_len < ix->params.k) return fail(SLK_E_INVALID, "read_len %d < k %d", read_len, ix->params.k);
  if (max_fragment == 0) max_fragment = 1024 * 1024;   // FRAGMENT_MAX (BrackenWeights.scala:303)
  if (max_fragment < (uint64_t)read_len || max_fragment > 0x7fffffffULL)
    return fail(SLK_E_INVALID, "max_fragment must lie in [read_len, 2^31)");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  std::unique_ptr<slk_bracken> b(new slk_bracken());   // (released into *out on success only)
  b->ix = ix;
  b->read_len = read_len;
  b->W = read_len - ix->params.k + 1;   // kmersInRead (:263)
  b->max_fragment = max_fragment;
  b->batch_bytes = (uint64_t)std::max(1L, env_long("SLK_BRACKEN_BATCH_MB", 1L << 10)) << 20;
  b->batch_bytes = std::max<uint64_t>(b->batch_bytes, max_fragment);
  b->h_offsets.assign(1, 0);
  hipError_t e = b->status.ensure(8);
  if (e == hipSuccess) e = hipMemset(b->status.p, 0, 8);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(SLK_E_HIP, "bracken: %s", hipGetErrorString(e)); }
  // 2^22 = 4 M pairs (64 MiB): a standard library has a few hundred thousand
  const int map_log2 = (int)std::min(32L, std::max(10L, env_long("SLK_BRACKEN_MAP_LOG2", 22)));
  rc = b->map.reset(nullptr, 1ULL << map_log2);
  if (rc == SLK_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SLK_E_HIP, "bracken: map setup failed");
  if (rc) return rc;
  *out = b.release();
  return SLK_OK;
}

int32_t slk_bracken_add(slk_bracken *b, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *source_taxa,
                        uint64_t R) {
  if (!b) return fail(SLK_E_INVALID, "null handle");
  int32_t rc = br_check_spent(b);
  if (rc) return rc;
  rc = check_ready(b->ix, st, true);
  if (rc) return rc;
  if (R && (!bases || !offsets || !source_taxa)) return fail(SLK_E_INVALID, "null argument");
  for (uint64_t r = 0; r < R; r++) {
    if (offsets[r + 1] < offsets[r]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (record %llu)", (unsigned long long)r);
    if (source_taxa[r] < 0) return fail(SLK_E_INVALID, "record %llu: source taxon %d", (unsigned long long)r, source_taxa[r]);
  }
  rc = set_device(b->ix);
  if (rc) return rc;
  const uint64_t L = (uint64_t)b->read_len, F = b->max_fragment;
  for (uint64_t r = 0; r < R; r++) {
    const uint64_t o = offsets[r], n = offsets[r + 1] - o;
    if (n < L) continue;   // Iterator.range(0, len - readLen + 1) is empty (:265)
    // splitToMaxLength(FRAGMENT_MAX, readLen) (:152-164): pieces of at most F, consecutive pieces overlap by readLen - 1
    const uint64_t step = F - (L - 1);
    for (uint64_t start = 0; start < n - L + 1; start += step) {
      const uint64_t end = (n <= F) ? n : std::min(start + F, n);
      const uint64_t len = end - start;
      if (b->h_bases.size() + len > b->batch_bytes && !b->h_source.empty()) {
        rc = br_run_batch(b, st);
        if (rc) return rc;
      }
      const uint64_t piece = b->h_source.size();
      const uint64_t nr = len - L + 1;
      b->h_chunk0.push_back(b->h_chunk_piece.size());
      for (uint64_t c = 0; c < (nr + BR_CHUNK - 1) / BR_CHUNK; c++) b->h_chunk_piece.push_back((uint32_t)piece);
      b->h_bases.insert(b->h_bases.end(), bases + o + start, bases + o + end);
      b->h_offsets.push_back(b->h_bases.size());
      b->h_source.push_back(source_taxa[r]);
      if (n <= F) break;
    }
  }
  return br_run_batch(b, st);
}

int32_t slk_bracken_result(slk_bracken *b, uint64_t *n, int32_t *dest, int32_t *source, uint64_t *count, uint64_t cap) {
  if (!b || !n) return fail(SLK_E_INVALID, "null argument");
  if (cap && (!dest || !source || !count)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = br_check_spent(b);
  if (rc) return rc;
  rc = set_device(b->ix);
  if (rc) return rc;
  std::vector<uint64_t> keys, counts;
  rc = b->map.read(nullptr, keys, counts);
  if (rc) return rc;
  std::vector<size_t> order(keys.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  auto dest_of = [&](size_t i) { return (int32_t)(uint32_t)keys[i]; };
  auto src_of = [&](size_t i) { return (int32_t)(uint32_t)(keys[i] >> 32); };
  std::sort(order.begin(), order.end(), [&](size_t a, size_t c) {
    return dest_of(a) != dest_of(c) ? dest_of(a) < dest_of(c) : src_of(a) < src_of(c);
  });
  *n = order.size();
  for (size_t i = 0; i < order.size() && i < cap; i++) {
    dest[i] = dest_of(order[i]);
    source[i] = src_of(order[i]);
    count[i] = counts[order[i]];
  }
  if (cap && cap < order.size()) return fail(SLK_E_CAPACITY, "%llu triples, capacity %llu", (unsigned long long)order.size(), (unsigned long long)cap);
  return SLK_OK;
}

void slk_bracken_destroy(slk_bracken *b) {
  if (!b) return;
  (void)hipSetDevice(b->ix->device);
  delete b;
}

}  // extern "C"
