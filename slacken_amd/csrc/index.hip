// index.hip -- the library side of the C ABI (include/slacken_amd.h): the record table's shape and sizing, create, append with a
// table that grows, merge, the taxonomy and its Euler tours, library construction from sequences, export, respace, finalize.
// Host-side only: the kernels it launches are in kernels.hip, build.hip, wide.hip, respace.hip and merge.hip.  (slk_index_export_range lives
// beside its kernels in export.hip, as slk_index_taxon_counts does in taxstats.hip.)
#include "chunkcut.h"
#include "hostside.h"
#include "laneplan.h"

// Geometry of the record table.  Any number of buckets (engine.h: the multiply-shift range reduction); a cell holds
//   [flag] remainder (64 - q, + 1 unless the count is a power of two) | displacement | taxon     in 64 bits,
// so the displacement field gets what the other fields leave (8 bits at most are used: 255 buckets of linear probing; a table
// filled to 0.8 has chains of over 63 full buckets), and the buckets' "a record went past" flag exists where a bit is left for it.
struct TableShape { uint64_t nb; int q, disp; bool flag; };
static const int DISP_MIN = CELLS == 16 ? 3 : 4;
static TableShape shape_of(uint64_t nb, int tb) {
  TableShape sh{std::max<uint64_t>(nb, 32), 0, 0, false};
  sh.q = ceil_log2_u64(sh.nb);
  const bool pow2 = sh.nb == (1ULL << sh.q);
  const int avail = 64 - tb - (64 - sh.q + (pow2 ? 0 : 1));
  static const bool no_flag = env_on("SLK_NO_BUCKET_FLAG");   // (A/B switch)
  sh.flag = avail - 1 >= DISP_MIN && !no_flag;
  sh.disp = std::min(8, avail - (sh.flag ? 1 : 0));
  return sh;
}
static uint64_t grow_buckets(uint64_t nb) { const int q = ceil_log2_u64(nb); return nb == (1ULL << q) ? nb * 2 : (1ULL << q); }
// displacement bits a table filled to `load` needs: the chains of full buckets grow with the load (measured maxima at 1e5..1e10
// records: load 0.55: 14 buckets, 0.70: 32, 0.80: over 63)
static int need_disp_bits(double load) { return load <= 0.50 ? 4 : load <= 0.62 ? 5 : load <= 0.72 ? 6 : load <= 0.80 ? 7 : 8; }
// `records` records in at least `nb` buckets: the table is made larger (to the next power of two: one bit back from the remainder)
// until its cells leave a displacement field long enough for the load it will then have.  ok = false: no such table below 2^32 buckets.
static TableShape settle_shape(uint64_t nb, uint64_t records, int tb, bool *ok) {
  TableShape sh = shape_of(nb, tb);
  while (sh.disp < DISP_MIN && sh.nb < (1ULL << 33)) sh = shape_of(grow_buckets(sh.nb), tb);
  while (sh.nb < (1ULL << 32) && sh.disp < std::max(DISP_MIN, need_disp_bits((double)records / ((double)sh.nb * CELLS)))) sh = shape_of(grow_buckets(sh.nb), tb);
  *ok = !(sh.nb > (1ULL << 32) || sh.disp < DISP_MIN);
  return sh;
}

// the build stream and the build counters of a new index, and its table (either kind) zeroed
static int32_t start_build_state(slk_index *ix, void *table, size_t table_bytes) {
  HIPCHK(hipStreamCreate(ix->build_stream.put()));
  HIPCHK(hipMemsetAsync(table, 0, table_bytes, ix->build_stream));
  HIPCHK(hipMalloc((void **)ix->d_max_disp.put(), sizeof(int32_t)));
  HIPCHK(hipMalloc((void **)ix->d_counters.put(), 4 * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(ix->d_max_disp, 0, sizeof(int32_t), ix->build_stream));
  HIPCHK(hipMemsetAsync(ix->d_counters, 0, 4 * sizeof(unsigned long long), ix->build_stream));
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  return SLK_OK;
}

// the one-word scan and space masks of a splitter (slk_index_create; slk_index_respace recomputes them for its new `spaces`)
static void set_scan_params(slk_index *ix, const slk_params *p, int W) {
  ScanParams &sp = ix->sp;
  sp.k = p->k; sp.m = p->m; sp.w = p->k - p->m + 1; sp.canonical = p->canonical ? 1 : 0;
  sp.sh = W == 1 ? (32 - p->m) * 2 : 0;   // (the one-word fields are unused with several id columns)
  sp.keep = (sp.sh == 0) ? ~0ULL : (~0ULL << sp.sh);
  // RandomXOR.mask (MinimizerPriorities.scala:146-160): one word; partial word => xorMask << (64 - (m%32)*2)
  sp.xmask = (p->m % 32 != 0) ? (p->xor_mask << (64 - (p->m % 32) * 2)) : p->xor_mask;
  // SpacedSeed.spaceMask (:285-300): fill(-1, m), then s times { <<= 4 ; |= 3 << (64 - (m%32)*2) }
  uint64_t sm = sp.keep;
  uint64_t finalBits = 3ULL << ((64 - (p->m % 32) * 2) & 63);
  for (int i = 0; i < p->spaces; i++) sm = (sm << 4) | finalBits;
  sp.smask = sm;
}

// The geometry of a one-word table for `expected_records` records with taxon fields of tb bits: load factor, buckets, cell layout.
static void adopt_shape(slk_index *ix, const TableShape &sh, int tb) {
  ix->bucket_bits = sh.q;
  ix->taxon_bits = tb;
  ix->disp_bits = sh.disp;
  ix->bucket_flag = sh.flag;
  ix->nbuckets = sh.nb;
}
static int32_t size_table(slk_index *ix, uint64_t expected_records, float load_factor, int tb) {
  // Load factor.  Given: as given (at most 0.95).  Default: the table takes the memory the device has.  Filled to 0.55 while that
  // costs at most 55 % of the HBM; then fuller, up to 0.70, at that size; then 0.70 with a larger table, up to 80 % of the HBM
  // (2.0e10 records on a 288 GB part: 229 GB); beyond that fuller again, 0.85 at most.  Measured at 1.0e10 records, 64-byte
  // buckets (profiles/r03_bucket_geometry.txt): load 0.45 1 124 M reads/s, 0.55 1 118, 0.70 1 028 -- what a fuller table costs is
  // second-bucket probes.
  const bool default_lf = !(load_factor > 0);
  const uint64_t expected = std::max<uint64_t>(expected_records, 1);
  double lf = load_factor;
  if (default_lf) {
    // (the memory that is FREE now, not the part's total: several tables may share a device -- `--shard-table --devices 0,0`, a
    //  dynamic library beside its base -- and each then takes its share of what the earlier ones left)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) { (void)hipGetLastError(); free_b = total_b = (size_t)288 << 30; }
    const double cell_bytes = (double)expected * 8.0, t = (double)std::min(total_b, free_b + ((size_t)2 << 30));
    if (cell_bytes / 0.55 <= 0.55 * t) lf = 0.55;
    else if (cell_bytes / 0.70 <= 0.55 * t) lf = cell_bytes / (0.55 * t);
    else if (cell_bytes / 0.70 <= 0.80 * t) lf = 0.70;
    else lf = std::min(0.85, cell_bytes / (0.80 * t));
  }
  if (lf > 0.95) lf = 0.95;
  // (a record that finds no cell within reach of its displacement field all the same makes the table grow: grow_table)
  const uint64_t cells_needed = (uint64_t)((double)expected / lf) + CELLS;
  bool shape_ok = false;
  const TableShape sh = settle_shape((cells_needed + CELLS - 1) / CELLS, expected, tb, &shape_ok);
  if (!shape_ok) { return fail(SLK_E_CAPACITY, "a table of %llu buckets is too large", (unsigned long long)sh.nb); }
  ix->load_target = (float)lf;
  adopt_shape(ix, sh, tb);
  return SLK_OK;
}

int32_t slk_index_create(const slk_params *p, const slk_table_config *cfg, int32_t device, slk_index **out) {
  if (!p || !cfg || !out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  if (p->m < 1 || p->k < p->m || p->spaces < 0 || p->spaces > p->m / 2)
    return fail(SLK_E_INVALID, "invalid splitter parameters k=%d m=%d spaces=%d", p->k, p->m, p->spaces);
  const int W = (p->m + 31) / 32;
  if (W > WIDE_MAXW) return fail(SLK_E_UNSUPPORTED, "minimizer width m=%d: at most %d nt (%d id columns)", p->m, 32 * WIDE_MAXW, WIDE_MAXW);
  if (p->id_longs != W) return fail(SLK_E_INVALID, "id_longs=%d but m=%d needs %d id columns", p->id_longs, p->m, W);
  if (p->k - p->m + 1 > 512) return fail(SLK_E_UNSUPPORTED, "k - m + 1 = %d > 512 m-mers per window", p->k - p->m + 1);
  if (W > 1 && (p->k - p->m + 1) * W > 128)
    return fail(SLK_E_UNSUPPORTED, "k - m + 1 = %d m-mers per window with %d id columns: at most %d", p->k - p->m + 1, W, 128 / W);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SLK_E_NO_GPU, "no HIP device available; this engine has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(SLK_E_INVALID, "device %d out of range (%d devices)", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SLK_E_NO_GPU, "device %d is %s; this library holds gfx950 (MI355X) code objects only", device,
                prop.gcnArchName);
  // (one id column: the staged scan's ring of a wave, 512 bytes per m-mer of the window, has to fit a workgroup's LDS -- laneplan.h: plan_scan)
  if (W == 1 && p->k - p->m + 1 > scan_max_window(prop.sharedMemPerBlock))
    return fail(SLK_E_UNSUPPORTED, "k - m + 1 = %d m-mers per window: the scan's ring needs %zu bytes of LDS, a workgroup of this device has %zu (at most %d m-mers)",
                p->k - p->m + 1, plan_scan(p->k - p->m + 1).lds, (size_t)prop.sharedMemPerBlock, scan_max_window(prop.sharedMemPerBlock));

  std::unique_ptr<slk_index> ix(new slk_index());   // (released into *out on success only)
  ix->device = device;
  ix->params = *p;
  set_scan_params(ix.get(), p, W);
  if (W > 1) {
    // several id columns: the staged kernels of wide.hip over an open-addressing table of (W key words, taxon) slots
    ix->W = W;
    WideParams &wp = ix->wp;
    wp.k = p->k; wp.m = p->m; wp.w = p->k - p->m + 1; wp.canonical = p->canonical ? 1 : 0; wp.W = W;
    wp.last_sh = ((32 - p->m % 32) % 32) * 2;
    for (int i = 0; i < W; i++) {   // RandomXOR.mask :146-160; NTBitArray.fill(-1, m) for the space mask
      wp.xmask[i] = (i == W - 1 && p->m % 32 != 0) ? (p->xor_mask << (64 - (p->m % 32) * 2)) : p->xor_mask;
      wp.smask[i] = ~0ULL;
    }
    if (wp.last_sh) wp.smask[W - 1] = ~0ULL << wp.last_sh;
    const uint64_t fb = 3ULL << ((64 - (p->m % 32) * 2) & 63);
    for (int s = 0; s < p->spaces; s++) {   // SpacedSeed.spaceMask :285-300: s times { <<= 4 over all words ; |= finalBits }
      for (int i = 0; i < W; i++) wp.smask[i] = (wp.smask[i] << 4) | (i + 1 < W ? wp.smask[i + 1] >> 60 : 0);
      wp.smask[W - 1] |= fb;
    }
    uint64_t cap = 1ULL << ceil_log2_u64(std::max<uint64_t>(cfg->expected_records, 8) * 2);
    ix->wt.mask = cap - 1;
    ix->taxon_bits = 31;
    hipError_t e1 = hipMalloc((void **)ix->wide_keys.put(), cap * W * 8);
    hipError_t e2 = e1 == hipSuccess ? hipMalloc((void **)ix->wide_taxa.put(), cap * 4) : e1;
    if (e2 != hipSuccess) {
      (void)hipGetLastError();
      return fail(SLK_E_HIP, "hipMalloc of the %llu-slot table failed: %s", (unsigned long long)cap, hipGetErrorString(e2));
    }
    ix->wt.keys = ix->wide_keys;
    ix->wt.taxa = ix->wide_taxa;
    ix->nbuckets = cap;
    int32_t rc = start_build_state(ix.get(), ix->wt.taxa, cap * 4);
    if (rc) return rc;
    *out = ix.release();
    return SLK_OK;
  }
  int32_t max_taxon = cfg->max_taxon > 0 ? cfg->max_taxon : ((1 << 22) - 1);
  int tb = 1;
  while (tb < 31 && (1LL << tb) <= (long long)max_taxon) tb++;
  int32_t rc = size_table(ix.get(), cfg->expected_records, cfg->load_factor, tb);
  if (rc) return rc;
  size_t bytes = (size_t)ix->nbuckets * CELLS * 8;
  hipError_t e = hipMalloc((void **)ix->cells.put(), bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(SLK_E_HIP, "hipMalloc of %zu table bytes failed: %s", bytes, hipGetErrorString(e));
  }
  rc = start_build_state(ix.get(), ix->cells, bytes);
  if (rc) return rc;
  *out = ix.release();
  return SLK_OK;
}

static int32_t read_build_counters(slk_index *ix) {
  unsigned long long c[3];
  int32_t md;
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  HIPCHK(hipMemcpy(c, ix->d_counters, sizeof(c), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&md, ix->d_max_disp, sizeof(md), hipMemcpyDeviceToHost));
  ix->records = c[0];
  ix->dups = c[1];
  ix->max_disp = md;
  ix->unplaced = c[2];
  if (c[2] != 0 && ix->W > 1) return fail(SLK_E_CAPACITY, "%llu records found no free slot: raise expected_records", c[2]);
  return SLK_OK;   // (one-word table: records that found no cell within reach are the caller's to settle -- insert_growing)
}

// Several id columns: what the insert kernel leaves after a call.  Records with a negative taxon were skipped there and counted
// (the device entry's taxa are checked nowhere else); the count belongs to this call alone and is cleared with the reading.
static int32_t read_wide_insert(slk_index *ix) {
  unsigned long long bad = 0;
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  HIPCHK(hipMemcpy(&bad, ix->d_counters + 3, sizeof(bad), hipMemcpyDeviceToHost));
  if (bad != 0) HIPCHK(hipMemset(ix->d_counters + 3, 0, sizeof(bad)));
  const int32_t rc = read_build_counters(ix);
  if (rc) return rc;
  if (bad != 0) return fail(SLK_E_INVALID, "%llu records with a negative taxon were not stored", bad);
  return SLK_OK;
}

static TableBuild build_view(slk_index *ix) {
  TableBuild t;
  t.cells = ix->cells;
  t.g = ix->geom();
  t.disp_limit = (1 << ix->disp_bits) - 1;
  t.shard = ix->shard;
  t.n_shards = ix->n_shards;
  t.max_disp = ix->d_max_disp;
  t.n_inserted = ix->d_counters;
  t.n_duplicate = ix->d_counters + 1;
  t.n_overflow = ix->d_counters + 2;
  return t;
}

// A record that found no cell within reach of its cells' displacement field -- a chain of full buckets longer than the field can
// count; the sizing keeps that from happening at the loads it chooses, a load_factor given by the caller or a library that outgrew
// its expected_records may not -- does NOT fail the load (a library is hours of Parquet streaming by then): the table moves to
// the next larger geometry (twice the buckets: the load halves and the remainder gives a bit to the displacement), piece by piece
// through a bounded staging buffer -- on the device while both tables fit its memory, through host memory otherwise --, and the
// insert that hit the limit runs again (records it had placed are found again as duplicates of themselves: the caller corrects
// the count).  Replaces KeyValueIndex.loadRecords' "it is a table scan: any size works" (S/slacken/KeyValueIndex.scala:150-159).
//
// When this fails.  Before the old table is touched -- no larger geometry, no memory for the pieces -- and on the device route
// throughout, the index keeps its old table, intact, and the call that needed the room fails alone.  The host route has to free the
// old table before it can allocate the new one: from there on a failure loses the records, the index is marked spent, and every
// later entry that takes it (set_device) says that the load must be repeated.
// buckets [b0, b1) of a table as records in dk / dt (room for `cap`), *n of them; complete on return
static int32_t export_piece(slk_index *ix, const TableView &from, uint64_t b0, uint64_t b1, DevBuf &dk, DevBuf &dt, DevBuf &dc, uint64_t cap,
                            unsigned long long *n) {
  HIPCHK(hipMemsetAsync(dc.p, 0, 8, ix->build_stream));
  launch_export_range(from, b0, b1, dk.as<int64_t>(), dt.as<int32_t>(), cap, dc.as<unsigned long long>(), ix->build_stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(n, dc.p, 8, hipMemcpyDeviceToHost, ix->build_stream));
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  return SLK_OK;
}
static int32_t grow_table(slk_index *ix) {
  bool ok = false;
  const TableShape sh = settle_shape(grow_buckets(ix->nbuckets), std::max<uint64_t>(ix->records, 1), ix->taxon_bits, &ok);
  if (!ok) return fail(SLK_E_CAPACITY, "the table cannot grow beyond %llu buckets", (unsigned long long)ix->nbuckets);
  const size_t new_bytes = (size_t)sh.nb * CELLS * 8;
  const uint64_t CH = (uint64_t)1 << 24;   // buckets per piece (at most 2^27 records: 1.5 GB of staging)
  DevBuf dk, dt, dc;
  HIPCHK(dc.ensure(8));
  DevPtr<uint64_t> new_cells;
  // (SLK_GROW_VIA_HOST=1: take the host route although both tables would fit the device -- how the tests reach it)
  const bool on_device = !env_on("SLK_GROW_VIA_HOST") && hipMalloc((void **)new_cells.put(), new_bytes) == hipSuccess;
  if (!on_device) (void)hipGetLastError();
  const uint64_t cap = std::min<uint64_t>(CH, ix->nbuckets) * CELLS;
  HIPCHK(dk.ensure(cap * 8));
  HIPCHK(dt.ensure(cap * 4));
  // scratch state of the move: inserted, duplicate, unplaced (the index's own counters keep counting the caller's records) and, in a
  // fourth word, the new table's maximum displacement (the index keeps the old table's until the new one is adopted)
  DevPtr<unsigned long long> d_scratch;
  HIPCHK(hipMalloc((void **)d_scratch.put(), 4 * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(d_scratch, 0, 4 * sizeof(unsigned long long), ix->build_stream));
  const TableView old_view = [&] { TableView v = ix->view(); v.to_orig = nullptr; return v; }();
  const uint64_t old_nb = ix->nbuckets;
  TableBuild nb = build_view(ix);   // the new table
  nb.g = slk_index::geom_of(sh.nb, sh.q, sh.flag, ix->taxon_bits, sh.disp);
  nb.disp_limit = (1 << sh.disp) - 1;
  nb.shard = 0; nb.n_shards = 0;   // (what is in the table is this shard's already)
  nb.max_disp = (int32_t *)(d_scratch + 3);
  nb.n_inserted = d_scratch; nb.n_duplicate = d_scratch + 1; nb.n_overflow = d_scratch + 2;
  auto insert_piece = [&](const int64_t *k, const int32_t *t, uint64_t n) -> int32_t {
    nb.cells = new_cells;
    launch_table_insert(nb, k, t, n, ix->build_stream);
    HIPCHK(hipGetLastError());
    return SLK_OK;
  };
  if (on_device) {
    HIPCHK(hipMemsetAsync(new_cells, 0, new_bytes, ix->build_stream));
    for (uint64_t b0 = 0; b0 < old_nb; b0 += CH) {
      unsigned long long n = 0;
      int32_t rc = export_piece(ix, old_view, b0, std::min(old_nb, b0 + CH), dk, dt, dc, cap, &n);
      if (!rc) rc = insert_piece(dk.as<int64_t>(), dt.as<int32_t>(), n);
      if (rc) return rc;
    }
  } else {
    // both tables do not fit the device: the records wait in host memory (12 bytes each) while the old table makes room
    std::vector<int64_t> h_keys;
    std::vector<int32_t> h_taxa;
    for (uint64_t b0 = 0; b0 < old_nb; b0 += CH) {
      unsigned long long n = 0;
      int32_t rc = export_piece(ix, old_view, b0, std::min(old_nb, b0 + CH), dk, dt, dc, cap, &n);
      if (rc) return rc;
      const size_t at = h_keys.size();
      h_keys.resize(at + n); h_taxa.resize(at + n);
      if (n) {
        HIPCHK(hipMemcpy(h_keys.data() + at, dk.p, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_taxa.data() + at, dt.p, n * 4, hipMemcpyDeviceToHost));
      }
    }
    ix->spent = true;   // (until the new table is adopted, below: the records are in h_keys / h_taxa only)
    ix->cells.reset();
    // (SLK_GROW_LOSE_TABLE=1: this allocation counts as failed -- how the tests reach a spent index)
    if (env_on("SLK_GROW_LOSE_TABLE") || hipMalloc((void **)new_cells.put(), new_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(SLK_E_HIP, "hipMalloc of %zu table bytes failed while the table was growing (the records are lost: load the library again "
                  "with a larger slk_table_config.expected_records)", new_bytes);
    }
    HIPCHK(hipMemsetAsync(new_cells, 0, new_bytes, ix->build_stream));
    for (uint64_t o = 0; o < h_keys.size(); o += cap) {
      const uint64_t n = std::min<uint64_t>(cap, h_keys.size() - o);
      HIPCHK(hipMemcpyAsync(dk.p, h_keys.data() + o, n * 8, hipMemcpyHostToDevice, ix->build_stream));
      HIPCHK(hipMemcpyAsync(dt.p, h_taxa.data() + o, n * 4, hipMemcpyHostToDevice, ix->build_stream));
      int32_t rc = insert_piece(dk.as<int64_t>(), dt.as<int32_t>(), n);
      if (rc) return rc;
      HIPCHK(hipStreamSynchronize(ix->build_stream));
    }
  }
  unsigned long long c[3] = {0, 0, 0};
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  HIPCHK(hipMemcpy(c, d_scratch, sizeof(c), hipMemcpyDeviceToHost));
  if (c[2] != 0 || c[1] != 0) return fail(SLK_E_HIP, "moving the table to a larger one lost records (%llu unplaced, %llu collided)", c[2], c[1]);
  HIPCHK(hipMemcpy(ix->d_max_disp, d_scratch + 3, sizeof(int32_t), hipMemcpyDeviceToDevice));
  ix->cells = std::move(new_cells);   // (the old table, if it is still there, is freed here)
  ix->nbuckets = sh.nb; ix->bucket_bits = sh.q; ix->disp_bits = sh.disp; ix->bucket_flag = sh.flag;
  ix->spent = false;
  ix->grown++;
  static const bool verbose = getenv("SLK_DEBUG_GROW") != nullptr;
  if (verbose) fprintf(stderr, "[slk] table grown to %llu buckets (%d displacement bits), %llu records moved %s\n", (unsigned long long)sh.nb, sh.disp,
                       c[0], on_device ? "on the device" : "through host memory");
  return SLK_OK;
}

// Runs `insert` (which queues one batch of records on the build stream; re-runnable) until every record of the batch has a cell,
// moving the table to a larger one in between if need be.  counts_dups: the insert counts keys that are present already (the plain
// record insert; the library builder merges them instead): a re-run then counts the records the first run placed as duplicates of
// themselves, which is taken out again.
static int32_t insert_growing(slk_index *ix, bool counts_dups, const std::function<int32_t()> &insert) {
  int32_t rc = read_build_counters(ix);   // (the state before this batch)
  if (rc) return rc;
  const uint64_t ins0 = ix->records, dup0 = ix->dups;
  for (int attempt = 0;; attempt++) {
    const uint64_t ins_before = ix->records;
    rc = insert();
    if (rc) return rc;
    rc = read_build_counters(ix);
    if (rc) return rc;
    if (ix->unplaced == 0) {
      if (counts_dups && attempt > 0) {
        // this run saw every record of the batch: new ones it inserted, all others it counted -- among them the (ins_before - ins0)
        // records earlier runs had placed
        const uint64_t dups = dup0 + (ix->dups - dup0) - (ins_before - ins0);
        const unsigned long long v = dups;
        HIPCHK(hipMemcpy(ix->d_counters + 1, &v, sizeof(v), hipMemcpyHostToDevice));
        ix->dups = dups;
      }
      return SLK_OK;
    }
    if (ix->W > 1) return fail(SLK_E_CAPACITY, "%llu records found no free slot: raise expected_records", (unsigned long long)ix->unplaced);
    if (attempt >= 6) return fail(SLK_E_CAPACITY, "%llu records could not be placed after the table had grown %d times", (unsigned long long)ix->unplaced, attempt);
    rc = grow_table(ix);
    if (rc) return rc;
    // the next run starts from this batch's beginning: its duplicate count too
    const unsigned long long z[2] = {dup0, 0};
    HIPCHK(hipMemcpy(ix->d_counters + 1, &z[0], sizeof(unsigned long long), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_counters + 2, &z[1], sizeof(unsigned long long), hipMemcpyHostToDevice));
    ix->dups = dup0;
  }
}

// Table-sharded libraries (BASELINE configs[3]): the index keeps the records whose key falls to `shard` of `n_shards`
// (slk_shard_of) and drops the others where they arrive -- in slk_index_append[_device] and in slk_index_add_sequences[_device] --
// so that every rank can be handed the same record stream or the same genomes.  Before the first record.
int32_t slk_index_set_shard(slk_index *ix, uint32_t shard, uint32_t n_shards) {
  if (!ix) return fail(SLK_E_INVALID, "null argument");
  if (ix->spent) return check_spent(ix);
  if (n_shards < 1 || n_shards > 64 || shard >= n_shards) return fail(SLK_E_INVALID, "shard %u of %u", shard, n_shards);
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "the sharded entry points support minimizers of up to 32 nt (one id column)");
  if (ix->finalized || ix->records != 0) return fail(SLK_E_STATE, "slk_index_set_shard must precede the first record");
  ix->shard = shard;
  ix->n_shards = n_shards;
  return SLK_OK;
}

// n records that are on the device into the one-word table, which grows if it must
static int32_t insert_records(slk_index *ix, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n) {
  return insert_growing(ix, true, [&]() -> int32_t {
    launch_table_insert(build_view(ix), d_keys, d_taxa, n, ix->build_stream);
    HIPCHK(hipGetLastError());
    return SLK_OK;
  });
}

int32_t slk_index_append_device(slk_index *ix, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n) {
  if (!ix || (n && (!d_keys || !d_taxa))) return fail(SLK_E_INVALID, "null argument");
  if (ix->finalized) return fail(SLK_E_STATE, "index is finalized");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  if (ix->W > 1) {
    launch_wide_insert(ix->wt, ix->W, d_keys, d_taxa, n, ix->d_counters, ix->build_stream);
    HIPCHK(hipGetLastError());
    return read_wide_insert(ix);
  }
  return insert_records(ix, d_keys, d_taxa, n);
}

int32_t slk_index_append(slk_index *ix, const int64_t *keys, const int32_t *taxa, uint64_t n) {
  if (!ix || (n && (!keys || !taxa))) return fail(SLK_E_INVALID, "null argument");
  if (ix->finalized) return fail(SLK_E_STATE, "index is finalized");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  const uint64_t CH = 1ULL << 24;
  if (ix->W > 1) {  // keys: n rows of W words (id1..idW)
    const int W = ix->W;
    for (uint64_t o = 0; o < n; o += CH) {
      uint64_t c = std::min(CH, n - o);
      for (uint64_t i = 0; i < c; i++)
        if (taxa[o + i] < 0) return fail(SLK_E_INVALID, "record %llu: negative taxon %d", (unsigned long long)(o + i), taxa[o + i]);
      HIPCHK(ix->stage_keys.ensure(c * 8 * W));
      HIPCHK(ix->stage_taxa.ensure(c * 4));
      rc = copy_in(&ix->staging, ix->build_stream, ix->stage_keys.p, keys + o * W, c * 8 * W);
      if (!rc) rc = copy_in(&ix->staging, ix->build_stream, ix->stage_taxa.p, taxa + o, c * 4);
      if (rc) return rc;
      launch_wide_insert(ix->wt, W, ix->stage_keys.as<int64_t>(), ix->stage_taxa.as<int32_t>(), c, ix->d_counters, ix->build_stream);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ix->build_stream));
    }
    return read_wide_insert(ix);
  }
  for (uint64_t o = 0; o < n; o += CH) {
    uint64_t c = std::min(CH, n - o);
    HIPCHK(ix->stage_keys.ensure(c * 8));
    HIPCHK(ix->stage_taxa.ensure(c * 4));
    int32_t max_t = (1 << ix->taxon_bits) - 1;
    for (uint64_t i = 0; i < c; i++)
      if (taxa[o + i] < 0 || taxa[o + i] > max_t)
        return fail(SLK_E_INVALID, "record %llu: taxon %d outside [0, %d] (slk_table_config.max_taxon)",
                    (unsigned long long)(o + i), taxa[o + i], max_t);
    rc = copy_in(&ix->staging, ix->build_stream, ix->stage_keys.p, keys + o, c * 8);
    if (!rc) rc = copy_in(&ix->staging, ix->build_stream, ix->stage_taxa.p, taxa + o, c * 4);
    if (rc) return rc;
    rc = insert_records(ix, ix->stage_keys.as<int64_t>(), ix->stage_taxa.as<int32_t>(), c);
    if (rc) return rc;
  }
  return read_build_counters(ix);
}

// ---- slk_index_merge_*: records united with what the table holds, per key by LCA (merge.hip) ---------------------------------------
// what every merge entry asks of its destination
static int32_t check_merge_dst(slk_index *ix) {
  int32_t rc = set_device(ix);   // (a spent index: SLK_E_STATE)
  if (rc) return rc;
  if (ix->W > 1) return fail(SLK_E_UNSUPPORTED, "slk_index_merge_* supports minimizers of up to 32 nt (one id column)");
  if (ix->finalized) return fail(SLK_E_STATE, "index is finalized");
  if (!ix->d_parents) return fail(SLK_E_STATE, "slk_index_merge_* needs the destination's taxonomy (LCA merging): call slk_index_set_taxonomy first");
  if (!ix->d_merge_bad) HIPCHK(hipMalloc((void **)ix->d_merge_bad.put(), 2 * sizeof(unsigned long long)));
  return SLK_OK;
}

// the records a call refused, summed over its passes
struct MergeRefused {
  unsigned long long n = 0;
  int32_t smallest = INT32_MAX;
  int32_t result() const {
    return n == 0 ? SLK_OK
                  : fail(SLK_E_INVALID, "%llu records name a taxon the destination's taxonomy does not define (smallest: %d)", n, smallest);
  }
};

// One pass of records into the table, which grows if it must.  `launch` queues the pass on the build stream and can be run again:
// the merge is idempotent, and the counters of the refused records belong to the attempt that completes.
static int32_t merge_growing(slk_index *ix, MergeRefused *refused, const std::function<void(const MergeCheck &)> &launch) {
  const MergeCheck check{ix->d_merge_remap, ix->n_merge_remap, ix->d_parents, ix->T, ix->d_merge_bad};
  int32_t rc = insert_growing(ix, false, [&]() -> int32_t {
    HIPCHK(hipMemsetAsync(ix->d_merge_bad, 0, sizeof(unsigned long long), ix->build_stream));
    HIPCHK(hipMemsetAsync(ix->d_merge_bad + 1, 0xff, sizeof(unsigned long long), ix->build_stream));
    launch(check);
    HIPCHK(hipGetLastError());
    return SLK_OK;
  });
  if (rc) return rc;
  unsigned long long bad[2];   // (insert_growing has synchronised the stream)
  HIPCHK(hipMemcpy(bad, ix->d_merge_bad, sizeof(bad), hipMemcpyDeviceToHost));
  if (bad[0]) {
    refused->n += bad[0];
    refused->smallest = std::min(refused->smallest, (int32_t)((uint32_t)bad[1] ^ 0x80000000u));
  }
  return SLK_OK;
}

int32_t slk_index_set_merge_remap(slk_index *ix, const int32_t *remap, int32_t n) {
  if (!ix || n < 0 || (n > 0 && !remap)) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  ix->d_merge_remap.reset();
  ix->n_merge_remap = 0;
  if (!remap || n == 0) return SLK_OK;
  HIPCHK(hipMalloc((void **)ix->d_merge_remap.put(), (size_t)n * sizeof(int32_t)));
  HIPCHK(hipMemcpy(ix->d_merge_remap, remap, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  ix->n_merge_remap = n;
  return SLK_OK;
}

int32_t slk_index_merge_records_device(slk_index *ix, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n) {
  if (!ix || (n && (!d_keys || !d_taxa))) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = check_merge_dst(ix);
  if (rc) return rc;
  MergeRefused refused;
  rc = merge_growing(ix, &refused, [&](const MergeCheck &c) { launch_merge_records(build_view(ix), c, d_keys, d_taxa, n, ix->build_stream); });
  return rc ? rc : refused.result();
}

int32_t slk_index_merge_records(slk_index *ix, const int64_t *keys, const int32_t *taxa, uint64_t n) {
  if (!ix || (n && (!keys || !taxa))) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = check_merge_dst(ix);
  if (rc) return rc;
  const uint64_t CH = 1ULL << 24;
  MergeRefused refused;
  for (uint64_t o = 0; o < n; o += CH) {
    const uint64_t c = std::min(CH, n - o);
    HIPCHK(ix->stage_keys.ensure(c * 8));
    HIPCHK(ix->stage_taxa.ensure(c * 4));
    rc = copy_in(&ix->staging, ix->build_stream, ix->stage_keys.p, keys + o, c * 8);
    if (!rc) rc = copy_in(&ix->staging, ix->build_stream, ix->stage_taxa.p, taxa + o, c * 4);
    if (!rc)
      rc = merge_growing(ix, &refused, [&](const MergeCheck &mc) {
        launch_merge_records(build_view(ix), mc, ix->stage_keys.as<int64_t>(), ix->stage_taxa.as<int32_t>(), c, ix->build_stream);
      });
    if (rc) {   // (nothing queued may still read the caller's memory)
      if (hipStreamSynchronize(ix->build_stream) != hipSuccess) (void)hipGetLastError();
      return rc;
    }
  }
  rc = read_build_counters(ix);
  return rc ? rc : refused.result();
}

int32_t slk_index_merge_index(slk_index *dst, const slk_index *src) {
  if (!dst || !src) return fail(SLK_E_INVALID, "null argument");
  if (src == dst) return fail(SLK_E_INVALID, "an index cannot be merged into itself");
  int32_t rc = check_spent(src);
  if (!rc) rc = check_merge_dst(dst);
  if (rc) return rc;
  if (src->W > 1) return fail(SLK_E_UNSUPPORTED, "slk_index_merge_index supports minimizers of up to 32 nt (one id column)");
  if (src->device != dst->device) return fail(SLK_E_INVALID, "the source is on device %d, the destination on device %d", src->device, dst->device);
  const slk_params &a = src->params, &b = dst->params;
  if (a.k != b.k || a.m != b.m || a.spaces != b.spaces || (a.canonical != 0) != (b.canonical != 0) || a.xor_mask != b.xor_mask)
    return fail(SLK_E_INVALID, "the splitters differ: source k=%d m=%d spaces=%d canonical=%d xor_mask=%016llx, destination k=%d m=%d spaces=%d "
                "canonical=%d xor_mask=%016llx", a.k, a.m, a.spaces, a.canonical, (unsigned long long)a.xor_mask, b.k, b.m, b.spaces, b.canonical,
                (unsigned long long)b.xor_mask);
  HIPCHK(hipStreamSynchronize(src->build_stream));   // the pass runs on the destination's stream: the source's records are all in
  MergeRefused refused;
  rc = merge_growing(dst, &refused, [&](const MergeCheck &c) { launch_merge_index(src->view(), build_view(dst), c, dst->build_stream); });
  return rc ? rc : refused.result();
}

// The taxonomy as the interval resolvers read it, on the device: resolve.h's build_tour of the forest (nothing for fewer than two ids
// or more than max_n: those callers walk)
static int32_t build_tax_nodes(const int32_t *parents, int32_t n, int32_t max_n, DevPtr<uint4> &out) {
  out.reset();
  if (n < 2 || n > max_n) return SLK_OK;
  const std::vector<TourNode> nodes = build_tour(parents, n);
  HIPCHK(hipMalloc((void **)out.put(), (size_t)n * sizeof(uint4)));
  HIPCHK(hipMemcpy(out, nodes.data(), (size_t)n * sizeof(uint4), hipMemcpyHostToDevice));
  return SLK_OK;
}

int32_t slk_index_set_taxonomy(slk_index *ix, const int32_t *parents, int32_t T) {
  if (!ix || !parents || T < 2) return fail(SLK_E_INVALID, "taxonomy needs parents[] with at least ROOT (T >= 2)");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  // The reference's parent walks terminate only on a forest (Taxonomy.scala:151-156); reject cycles up front.
  {
    std::vector<uint8_t> state((size_t)T, 0);  // 0 new, 1 on the current path, 2 done
    std::vector<int32_t> path;
    for (int32_t t = 1; t < T; t++) {
      int32_t x = t;
      path.clear();
      while (x != 0 && state[x] == 0) {
        if (parents[x] < 0 || parents[x] >= T) return fail(SLK_E_INVALID, "parents[%d] = %d out of range", x, parents[x]);
        state[x] = 1;
        path.push_back(x);
        x = parents[x];
      }
      if (x != 0 && state[x] == 1) return fail(SLK_E_INVALID, "taxonomy has a cycle through taxon %d", x);
      for (int32_t y : path) state[y] = 2;
    }
  }
  if (ix->D) return fail(SLK_E_STATE, "this finalized index stores dense taxon ids derived from its taxonomy: the taxonomy cannot be replaced");
  HIPCHK(hipMalloc((void **)ix->d_parents.put(), (size_t)T * sizeof(int32_t)));
  HIPCHK(hipMemcpy(ix->d_parents, parents, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice));
  ix->T = T;
  ix->h_parents.assign(parents, parents + T);
  // Euler tours: for the fused kernels (ids of at most 22 bits take the lane kernel; wider ones are renumbered at finalize, which
  // builds that tour then) and, in the caller's ids, for the staged classify kernel (up to 2^26 ids: 1 GiB of node records)
  ix->d_nodes = nullptr;
  rc = build_tax_nodes(parents, T, 1 << 26, ix->d_nodes_orig);
  if (rc) return rc;
  if (T <= (1 << 22) + 1) ix->d_nodes = ix->d_nodes_orig;   // (one tour serves both)
  return SLK_OK;
}

// Library construction with several id columns (minimizers of 33..128 nt): the staged kernels of wide.hip.  Groups of about 64 MiB
// of sequence are cut into chunks of BUILD_CHUNK_WINDOWS k-mer windows (overlapping by k - 1 bases: the same minimizer SET), the
// chunks are scanned as a batch of fragments, and their SEQUENCE-flag spans are inserted / LCA-merged one lane per span.
static int32_t add_sequences_wide(slk_index *ix, const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa, uint64_t S, bool bases_on_device) {
  const uint32_t k = (uint32_t)ix->wp.k, CW = BUILD_CHUNK_WINDOWS;
  for (uint64_t i = 0; i < S; i++) {
    if (offsets[i + 1] < offsets[i]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)i);
    if (taxa[i] < 0) return fail(SLK_E_INVALID, "sequence %llu: negative taxon %d", (unsigned long long)i, taxa[i]);
  }
  std::vector<uint8_t> host_copy;
  if (bases_on_device && S) {   // (this path stages its chunks on the host)
    host_copy.resize(offsets[S]);
    HIPCHK(hipMemcpy(host_copy.data(), bases, offsets[S], hipMemcpyDeviceToHost));
    bases = host_copy.data();
  }
  const uint64_t GROUP = 64ULL << 20;
  DevBuf d_bases, d_off, d_tax, d_keys, d_meta, d_count;
  std::vector<uint8_t> cb;
  std::vector<uint64_t> coff;
  std::vector<int32_t> ctax;
  auto flush = [&]() -> int32_t {
    if (ctax.empty()) return SLK_OK;
    const uint64_t nc = ctax.size(), total = cb.size();
    HIPCHK(d_bases.ensure(total + 16));
    HIPCHK(d_off.ensure((nc + 1) * 8));
    HIPCHK(d_tax.ensure(nc * 4));
    HIPCHK(d_keys.ensure((total + 1) * 8 * ix->W));
    HIPCHK(d_meta.ensure((total + 1) * 4));
    HIPCHK(d_count.ensure((nc + 1) * 4));
    int32_t rc = copy_in(&ix->staging, ix->build_stream, d_bases.p, cb.data(), total);
    if (!rc) rc = copy_in(&ix->staging, ix->build_stream, d_off.p, coff.data(), (nc + 1) * 8);
    if (!rc) rc = copy_in(&ix->staging, ix->build_stream, d_tax.p, ctax.data(), nc * 4);
    if (rc) return rc;
    launch_wide_scan(ix->wp, d_bases.as<uint8_t>(), d_off.as<uint64_t>(), nullptr, nullptr, nc, d_keys.as<uint64_t>(), d_meta.as<int32_t>(),
                     d_count.as<int32_t>(), ix->build_stream);
    launch_wide_build_insert(ix->wt, ix->W, ix->d_parents, ix->T, d_off.as<uint64_t>(), nc, d_keys.as<uint64_t>(), d_meta.as<int32_t>(),
                             d_count.as<int32_t>(), d_tax.as<int32_t>(), ix->d_counters, ix->build_stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ix->build_stream));
    cb.clear(); coff.assign(1, 0); ctax.clear();
    return SLK_OK;
  };
  coff.assign(1, 0);
  for (uint64_t q = 0; q < S; q++) {
    const uint64_t len = offsets[q + 1] - offsets[q];
    if (taxa[q] == 0 || len < k) continue;
    const uint64_t windows = len - k + 1;
    for (uint64_t w0 = 0; w0 < windows; w0 += CW) {
      const uint64_t nw = std::min<uint64_t>(CW, windows - w0);
      const uint8_t *src = bases + offsets[q] + w0;
      cb.insert(cb.end(), src, src + nw + k - 1);
      coff.push_back(cb.size());
      ctax.push_back(taxa[q]);
      if (cb.size() >= GROUP) { int32_t rc = flush(); if (rc) return rc; }
    }
  }
  int32_t rc = flush();
  if (rc) return rc;
  return read_build_counters(ix);
}

// bases_on_device: `bases` is resident on the index's GPU and is scanned where it lies
static int32_t add_sequences(slk_index *ix, const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa, uint64_t S,
                             bool bases_on_device) {
  if (!ix || (S && (!bases || !offsets || !taxa))) return fail(SLK_E_INVALID, "null argument");
  if (ix->finalized) return fail(SLK_E_STATE, "index is finalized");
  if (!ix->d_parents) return fail(SLK_E_STATE, "slk_index_add_sequences needs the taxonomy (LCA merging): call slk_index_set_taxonomy first");
  if (ix->W == 1 && ix->sp.w > BUILD_MAX_W) return fail(SLK_E_UNSUPPORTED, "library construction supports windows of up to %d m-mers (k - m + 1 = %d)", BUILD_MAX_W, ix->sp.w);
  int32_t rc = set_device(ix);
  if (rc) return rc;
  if (ix->W > 1) return add_sequences_wide(ix, bases, offsets, taxa, S, bases_on_device);
  const int32_t max_t = (int32_t)((1LL << ix->taxon_bits) - 1);
  const uint32_t k = (uint32_t)ix->sp.k, CW = BUILD_CHUNK_WINDOWS;
  for (uint64_t i = 0; i < S; i++) {
    if (offsets[i + 1] < offsets[i]) return fail(SLK_E_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)i);
    if (taxa[i] < 0 || taxa[i] > max_t)
      return fail(SLK_E_INVALID, "sequence %llu: taxon %d outside [0, %d] (slk_table_config.max_taxon)", (unsigned long long)i, taxa[i], max_t);
  }
  // groups of whole sequences of about 1 GiB; each is cut into chunks of CW windows overlapping by k-1 bases
  const uint64_t GROUP = 1ULL << 30;
  DevBuf d_bases, d_start, d_len, d_tax;
  std::vector<uint64_t> cstart;
  std::vector<uint32_t> clen;
  std::vector<int32_t> ctax;
  for (uint64_t i = 0, j; i < S; i = j) {
    j = group_end(offsets, i, S, GROUP);
    const uint64_t g0 = offsets[i], gbytes = offsets[j] - g0;
    cstart.clear(); clen.clear(); ctax.clear();
    cut_chunks(offsets, i, j, k, CW, false, [&](uint64_t q) { return taxa[q] == 0; }, [&](uint64_t q, uint64_t start, uint32_t len, uint32_t) {
      cstart.push_back(start);
      clen.push_back(len);
      ctax.push_back(taxa[q]);
    });
    if (!cstart.empty()) {
      uint64_t nc = cstart.size();
      HIPCHK(d_start.ensure(nc * 8));
      HIPCHK(d_len.ensure(nc * 4));
      HIPCHK(d_tax.ensure(nc * 4));
      const uint8_t *src = bases + g0;
      if (!bases_on_device) {
        HIPCHK(d_bases.ensure(gbytes));
        rc = copy_in(&ix->staging, ix->build_stream, d_bases.p, bases + g0, gbytes);
        if (rc) return rc;
        src = d_bases.as<uint8_t>();
      }
      rc = copy_in(&ix->staging, ix->build_stream, d_start.p, cstart.data(), nc * 8);
      if (!rc) rc = copy_in(&ix->staging, ix->build_stream, d_len.p, clen.data(), nc * 4);
      if (!rc) rc = copy_in(&ix->staging, ix->build_stream, d_tax.p, ctax.data(), nc * 4);
      if (rc) return rc;
      // (re-runnable: the merge by LCA is idempotent, so a group that ran into the table's limit is simply scanned again)
      rc = insert_growing(ix, false, [&]() -> int32_t {
        launch_build(ix->sp, build_view(ix), ix->d_parents, ix->T, src, gbytes, d_start.as<uint64_t>(),
                     d_len.as<uint32_t>(), d_tax.as<int32_t>(), nc, ix->build_stream);
        HIPCHK(hipGetLastError());
        return SLK_OK;
      });
      if (rc) return rc;
    }
  }
  return read_build_counters(ix);
}

int32_t slk_index_add_sequences(slk_index *ix, const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa,
                                uint64_t S) {
  return add_sequences(ix, bases, offsets, taxa, S, false);
}

int32_t slk_index_add_sequences_device(slk_index *ix, const uint8_t *d_bases, const uint64_t *offsets, const int32_t *taxa,
                                       uint64_t S) {
  return add_sequences(ix, d_bases, offsets, taxa, S, true);
}

int32_t slk_index_export(const slk_index *ix, int64_t *keys, int32_t *taxa, uint64_t capacity, uint64_t *n_records) {
  if (!ix || !n_records || (capacity && (!keys || !taxa))) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  DevBuf dk, dt, dc;
  HIPCHK(dk.ensure(std::max<uint64_t>(capacity, 1) * 8 * ix->W));
  HIPCHK(dt.ensure(std::max<uint64_t>(capacity, 1) * 4));
  HIPCHK(dc.ensure(8));
  HIPCHK(hipMemset(dc.p, 0, 8));
  if (ix->W > 1) {
    launch_wide_export(ix->wt, ix->W, dk.as<int64_t>(), dt.as<int32_t>(), capacity, dc.as<unsigned long long>(), ix->build_stream);
  } else {
    launch_export(ix->view(), ix->nbuckets, dk.as<int64_t>(), dt.as<int32_t>(), capacity, dc.as<unsigned long long>(), ix->build_stream);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  unsigned long long n = 0;
  HIPCHK(hipMemcpy(&n, dc.p, 8, hipMemcpyDeviceToHost));
  *n_records = n;
  uint64_t got = std::min<uint64_t>(n, capacity);
  if (got) {
    HIPCHK(hipMemcpy(keys, dk.p, got * 8 * ix->W, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(taxa, dt.p, got * 4, hipMemcpyDeviceToHost));
  }
  if (n > capacity && capacity) return fail(SLK_E_CAPACITY, "%llu records, capacity %llu", n, (unsigned long long)capacity);
  return SLK_OK;
}

// ---- slk_index_respace: KeyValueIndex.respace (S/slacken/KeyValueIndex.scala:353-384) on the device (respace.hip) -----------------
template <class T> static int32_t clone_device(DevPtr<T> &dst, const DevPtr<T> &src, size_t n, hipStream_t s) {
  if (!src.get() || n == 0) return SLK_OK;
  HIPCHK(hipMalloc((void **)dst.put(), n * sizeof(T)));
  HIPCHK(hipMemcpyAsync(dst.get(), src.get(), n * sizeof(T), hipMemcpyDeviceToDevice, s));
  return SLK_OK;
}

int32_t slk_index_respace(const slk_index *src, int32_t spaces, const slk_table_config *cfg, slk_index **out) {
  if (!src || !out) return fail(SLK_E_INVALID, "null argument");
  *out = nullptr;
  int32_t rc = set_device(src);   // (a spent index: SLK_E_STATE)
  if (rc) return rc;
  if (!src->finalized) return fail(SLK_E_STATE, "slk_index_respace needs a finalized index");
  if (!src->d_parents) return fail(SLK_E_STATE, "slk_index_respace needs the taxonomy (LCA merging): call slk_index_set_taxonomy first");
  if (spaces <= src->params.spaces)   // the reference's wording (KeyValueIndex.scala:358)
    return fail(SLK_E_INVALID, "Respacing to a smaller or identical number of spaces is not meaningful. (was %d, requested %d)",
                src->params.spaces, spaces);
  if (spaces > src->params.m / 2)     // SpacedSeed's assert (MinimizerPriorities.scala)
    return fail(SLK_E_INVALID, "%d spaces in minimizers of %d nt: at most %d", spaces, src->params.m, src->params.m / 2);
  if (src->W > 1) return fail(SLK_E_UNSUPPORTED, "slk_index_respace supports minimizers of up to 32 nt (one id column)");
  if (src->n_shards > 1)
    return fail(SLK_E_UNSUPPORTED, "a shard of a table-sharded library cannot be respaced: the owner of a key is fmix64(key) mod n, and the key changes");
  hipStream_t s = src->build_stream;   // the stream the source's records were inserted on: the pass sees them all

  std::unique_ptr<slk_index> ix(new slk_index());   // (released into *out on success only; the source's device is selected)
  ix->device = src->device;
  ix->params = src->params;
  ix->params.spaces = spaces;
  set_scan_params(ix.get(), &ix->params, 1);
  // the source's taxonomy and, where it has them, its dense-id tables: the cells of the new table hold the ids the source's hold
  ix->T = src->T;
  ix->D = src->D;
  ix->h_parents = src->h_parents;
  rc = clone_device(ix->d_parents, src->d_parents, (size_t)src->T, s);
  if (!rc) rc = clone_device(ix->d_to_dense, src->d_to_dense, (size_t)src->T, s);
  if (!rc) rc = clone_device(ix->d_nodes_orig, src->d_nodes_orig, (size_t)src->T, s);
  if (!rc) rc = clone_device(ix->d_parents_dense, src->d_parents_dense, (size_t)src->D + 1, s);
  if (!rc) rc = clone_device(ix->d_to_orig, src->d_to_orig, (size_t)src->D + 1, s);
  if (!rc) rc = clone_device(ix->d_nodes_dense, src->d_nodes_dense, (size_t)src->D + 1, s);
  if (rc) return rc;
  ix->d_nodes = src->d_nodes == nullptr ? nullptr : src->d_nodes == src->d_nodes_dense.get() ? ix->d_nodes_dense.get() : ix->d_nodes_orig.get();

  // every record of the source could keep a key of its own: its record count bounds the new table's
  const uint64_t expected = cfg && cfg->expected_records ? cfg->expected_records : std::max<uint64_t>(src->records, 1);
  rc = size_table(ix.get(), expected, cfg ? cfg->load_factor : 0.0f, src->taxon_bits);
  if (rc) return rc;
  // SLK_RESPACE_BUCKETS: the first table has this many buckets (or the fewest its cell layout allows, if that is more) whatever the
  // record count -- how the tests reach the repeat below
  const long forced = env_long("SLK_RESPACE_BUCKETS", 0);
  if (forced > 0) {
    bool ok = false;
    const TableShape sh = settle_shape((uint64_t)forced, 1, src->taxon_bits, &ok);
    if (!ok) return fail(SLK_E_CAPACITY, "SLK_RESPACE_BUCKETS=%ld: no such table", forced);
    adopt_shape(ix.get(), sh, src->taxon_bits);
  }
  HIPCHK(hipStreamCreate(ix->build_stream.put()));
  HIPCHK(hipMalloc((void **)ix->d_max_disp.put(), sizeof(int32_t)));
  HIPCHK(hipMalloc((void **)ix->d_counters.put(), 4 * sizeof(unsigned long long)));
  for (int attempt = 0;; attempt++) {
    const size_t bytes = (size_t)ix->nbuckets * CELLS * 8;
    const hipError_t e = hipMalloc((void **)ix->cells.put(), bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(SLK_E_HIP, "hipMalloc of %zu table bytes beside the source's table failed: %s", bytes, hipGetErrorString(e));
    }
    HIPCHK(hipMemsetAsync(ix->cells, 0, bytes, s));
    HIPCHK(hipMemsetAsync(ix->d_max_disp, 0, sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(ix->d_counters, 0, 4 * sizeof(unsigned long long), s));
    launch_respace(src->view(), build_view(ix.get()), ix->sp.smask, src->kernel_parents(), src->kernel_ntax(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    rc = read_build_counters(ix.get());
    if (rc) return rc;
    if (ix->unplaced == 0) break;
    // A record found no cell within reach of the displacement field.  The source is untouched and the pass idempotent: the table is
    // dropped and the pass repeated into twice the buckets (the taxon-count map of taxstats.hip does the same).
    if (attempt >= 8)
      return fail(SLK_E_CAPACITY, "%llu records could not be placed after the pass had been repeated %d times", (unsigned long long)ix->unplaced, attempt);
    ix->cells.reset();
    bool ok = false;
    const TableShape sh = settle_shape(grow_buckets(ix->nbuckets), 1, src->taxon_bits, &ok);
    if (!ok) return fail(SLK_E_CAPACITY, "the table cannot grow beyond %llu buckets", (unsigned long long)ix->nbuckets);
    adopt_shape(ix.get(), sh, src->taxon_bits);
    ix->grown++;
  }
  ix->unplaced = 0;
  ix->dups = 0;   // (merges are the purpose here, not a contract violation)
  ix->finalized = true;
  *out = ix.release();
  return SLK_OK;
}

// Dense taxon ids.  The lane-per-fragment kernel keeps a fragment's taxon -> count map as one LDS word per entry
// (taxon << 10 | count): taxon ids of up to 22 bits.  NCBI's ids pass 2^22 = 4 194 304 within a few releases, but the NODES of
// the taxonomy are far fewer than the id range; so when the caller's ids do not fit, the cells are rewritten once, here, to hold
// the rank of their taxon among the taxonomy's nodes (in increasing id order, ROOT = 1 stays 1), the fused kernels walk a
// parents array in those ranks, and ids are translated back where taxa leave the engine (engine.h: ext_taxon).  Needs the
// taxonomy to be set before finalize and every record's taxon to be one of its nodes; otherwise the ids stay as given and
// fragments take the wave-per-fragment kernel, as before.
static int32_t make_dense_taxa(slk_index *ix) {
  if (ix->W > 1 || ix->taxon_bits <= 22 || ix->h_parents.empty() || ix->D) return SLK_OK;
  const int32_t T = ix->T;
  std::vector<int32_t> to_dense((size_t)T, 0), to_orig(1, 0);
  for (int32_t t = 1; t < T; t++)
    if (t == 1 || ix->h_parents[t] != 0) { to_dense[t] = (int32_t)to_orig.size(); to_orig.push_back(t); }
  const int32_t D = (int32_t)to_orig.size() - 1;
  if (D < 1 || D >= (1 << 22)) return SLK_OK;
  std::vector<int32_t> pd((size_t)D + 1, 0);
  for (int32_t d = 1; d <= D; d++) pd[d] = to_dense[ix->h_parents[to_orig[d]]];  // (parent of ROOT is NONE = 0)
  DevPtr<int32_t> d_td, d_to, d_pd;
  DevPtr<unsigned long long> d_bad;
  unsigned long long bad = 0;
  HIPCHK(hipMalloc((void **)d_td.put(), (size_t)T * 4));
  HIPCHK(hipMalloc((void **)d_bad.put(), 8));
  HIPCHK(hipMemcpy(d_td, to_dense.data(), (size_t)T * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d_bad, 0, 8));
  launch_remap_cells(ix->cells, ix->nbuckets * CELLS, ix->taxon_bits, d_td, T, d_bad, false, ix->build_stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  HIPCHK(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
  if (bad != 0) return SLK_OK;  // records whose taxon is not a node of this taxonomy: keep the ids as they are
  launch_remap_cells(ix->cells, ix->nbuckets * CELLS, ix->taxon_bits, d_td, T, d_bad, true, ix->build_stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ix->build_stream));
  HIPCHK(hipMalloc((void **)d_to.put(), ((size_t)D + 1) * 4));
  HIPCHK(hipMalloc((void **)d_pd.put(), ((size_t)D + 1) * 4));
  HIPCHK(hipMemcpy(d_to, to_orig.data(), ((size_t)D + 1) * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_pd, pd.data(), ((size_t)D + 1) * 4, hipMemcpyHostToDevice));
  ix->d_to_dense = std::move(d_td); ix->d_to_orig = std::move(d_to); ix->d_parents_dense = std::move(d_pd); ix->D = D;
  ix->d_nodes = nullptr;   // (the tour of the ids as given stays with the staged kernel)
  const int32_t rc = build_tax_nodes(pd.data(), D + 1, (1 << 22) + 1, ix->d_nodes_dense);
  ix->d_nodes = ix->d_nodes_dense;
  return rc;
}

int32_t slk_index_finalize(slk_index *ix) {
  if (!ix) return fail(SLK_E_INVALID, "null argument");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  rc = read_build_counters(ix);
  if (rc) return rc;
  ix->stage_keys.release();
  ix->stage_taxa.release();
  ix->staging.release();
  if (!ix->finalized) {
    rc = make_dense_taxa(ix);
    if (rc) return rc;
  }
  ix->finalized = true;
  return SLK_OK;
}

int32_t slk_index_get_info(const slk_index *ix, slk_index_info *out) {
  if (!ix || !out) return fail(SLK_E_INVALID, "null argument");
  memset(out, 0, sizeof(*out));
  if (ix->spent) return check_spent(ix);
  out->records = ix->records;
  out->buckets = ix->nbuckets;
  out->table_bytes = ix->W > 1 ? ix->nbuckets * (8 * ix->W + 4) : ix->nbuckets * CELLS * 8;
  out->bucket_bits = ix->bucket_bits;
  out->taxon_bits = ix->taxon_bits;
  out->disp_bits = ix->disp_bits;
  out->max_displacement = ix->max_disp;
  out->duplicate_keys = ix->dups;
  out->taxonomy_size = ix->T;
  out->device = ix->device;
  out->dense_taxa = ix->D;
  out->bucket_cells = ix->W > 1 ? 1 : CELLS;
  out->load_factor = ix->load_target;
  out->grown = (int32_t)ix->grown;
  return SLK_OK;
}

int32_t slk_index_lookup(const slk_index *ix, const int64_t *keys, uint64_t n, int32_t *out_taxa) {
  if (!ix || (n && (!keys || !out_taxa))) return fail(SLK_E_INVALID, "null argument");
  if (!ix->finalized) return fail(SLK_E_STATE, "index is not finalized");
  int32_t rc = set_device(ix);
  if (rc) return rc;
  if (n == 0) return SLK_OK;
  DevBuf k, o;
  HIPCHK(k.ensure(n * 8 * ix->W));
  HIPCHK(o.ensure(n * 4));
  HIPCHK(hipMemcpy(k.p, keys, n * 8 * ix->W, hipMemcpyHostToDevice));
  if (ix->W > 1) launch_wide_lookup(ix->wt, ix->W, k.as<int64_t>(), n, o.as<int32_t>(), nullptr);
  else launch_table_lookup(ix->view(), k.as<int64_t>(), n, o.as<int32_t>(), nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out_taxa, o.p, n * 4, hipMemcpyDeviceToHost));
  return SLK_OK;
}

void slk_index_destroy(slk_index *ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  delete ix;
}
