/*
 * slacken_amd.h -- C ABI of the MI355X-native classify engine (libslacken_amd.so).
 *
 * Drop-in boundary for the hot path of JNP-Solutions/Slacken:
 *   minimizer scan -> minimizer->taxon lookup -> per-read LCA ("resolveTree") classification.
 *
 * The reference has NO native/FFI interface (it is Scala on Spark).  The seam this ABI sits
 * behind is therefore method-level; each entry point cites the reference method(s) it replaces, relative to
 * /root/reference/src/main/scala/com/jnpersson/ (abbreviated S/).  INTEGRATION.md shows the JNI binding a
 * maintainer would add on the Scala side.
 *
 * Conventions
 *   - every function returns int32 status: 0 = ok, negative = error (SLK_E_*); slk_last_error() gives the text
 *     (thread-local);
 *   - no exceptions, no callbacks, no ownership transfer: the caller owns every buffer it passes; the library owns
 *     only the opaque handles it created;
 *   - plain pointers and sizes only.  "host" entry points take host pointers and do their own H2D/D2H; "_device"
 *     entry points take pointers to memory already resident on the index's GPU and are asynchronous on the
 *     slk_stream (call slk_stream_synchronize before reading results);
 *   - a buffer of bases is exactly offsets[R] (mate_offsets[R]) bytes: nothing past it is read, no padding is needed
 *     (the kernels stream 16-byte blocks and assemble a buffer's last block from byte loads);
 *   - an slk_index is immutable after slk_index_finalize() and may be shared by many threads; an slk_stream holds
 *     one HIP stream plus the scratch of ONE in-flight batch: use one per calling thread.
 *   - minimizers of up to 128 nt (id_longs = ceil(m/32) <= 4 key words per record, row-major) are supported by
 *     slk_index_create / append / lookup / add_sequences / export, slk_spans_batch_wide and the classify entry points; the staged
 *     device entries and the sharded ones take one-word keys (m <= 32) and return SLK_E_UNSUPPORTED otherwise.
 */
#ifndef SLACKEN_AMD_H
#define SLACKEN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLK_OK 0
#define SLK_E_INVALID (-1)     /* bad argument */
#define SLK_E_UNSUPPORTED (-2) /* e.g. m > 32 */
#define SLK_E_HIP (-3)         /* HIP runtime error (text in slk_last_error) */
#define SLK_E_NO_GPU (-4)      /* no usable gfx950 device: there is NO CPU fallback */
#define SLK_E_CAPACITY (-5)    /* output buffer or table capacity exceeded */
#define SLK_E_STATE (-6)       /* call order violated (e.g. classify before finalize / taxonomy) */

/* S/slacken/package.scala:30-39 and S/slacken/Taxonomy.scala:30-31 */
#define SLK_TAXON_NONE 0
#define SLK_TAXON_ROOT 1
#define SLK_TAXON_AMBIGUOUS (-1)
#define SLK_TAXON_MATE_PAIR_BORDER (-2)
#define SLK_FLAG_SEQUENCE 1
#define SLK_FLAG_AMBIGUOUS 2
#define SLK_FLAG_MATE_PAIR_BORDER 3
/* S/kmers/minimizer/package.scala:32 */
#define SLK_DEFAULT_TOGGLE_MASK 0xe37e28c4271b5a2dULL

typedef struct slk_index slk_index;
typedef struct slk_stream slk_stream;

/* The splitter parameters of an index: S/kmers/IndexParams.scala:30-47 (k, m), S/kmers/SplitterFormat.scala:42-64
 * (randomXOR mask, canonical, minimizerSpaces).  Defaults of `slacken build`: k=35, m=31, spaces=7,
 * xor_mask=SLK_DEFAULT_TOGGLE_MASK, canonical=1 (S/slacken/Slacken.scala:126-136). */
typedef struct {
  int32_t k;
  int32_t m;
  int32_t spaces;
  int32_t canonical;
  uint64_t xor_mask;
  int32_t id_longs; /* ceil(m/32) <= 4, S/slacken/KeyValueIndex.scala:49: key words per record */
  int32_t reserved;
} slk_params;

/* Sizing of the HBM-resident record table (the engine's replacement for the bucketed Parquet table scanned by the
 * join at S/slacken/Classifier.scala:84). */
typedef struct {
  uint64_t expected_records; /* upper bound on records that will be appended.  One id column: a bound that proves too low makes
                                the table grow.  Several id columns (m > 32): the table does NOT grow; it has as many slots as
                                the power of two at or above 2 x expected_records (16 at least), takes records until every
                                slot is used, and fails with SLK_E_CAPACITY beyond that (see slk_index_append) */
  int32_t max_taxon;         /* largest taxon id that will be appended (0 = derive from nothing: 2^22-1) */
  float load_factor;         /* target cells-used fraction, 0 = default: 0.55 while the table then takes at most 55 % of the device's
                                FREE memory, more for larger libraries (0.85 at most); less for tables whose cells leave a short
                                displacement field */
} slk_table_config;

typedef struct {
  uint64_t records;       /* records stored (taxon != NONE) */
  uint64_t buckets;       /* buckets of bucket_cells 8-byte cells (any number: not a power of two) */
  uint64_t table_bytes;
  int32_t bucket_bits, taxon_bits, disp_bits; /* bucket_bits = ceil(log2(buckets)) */
  int32_t max_displacement; /* largest bucket displacement in use (0 = every record in its home bucket) */
  uint64_t duplicate_keys;  /* appended records whose key was already present (contract violation; first kept) -- tables with
                               one and with several id columns alike; of two such records in ONE call either may be the first */
  int32_t taxonomy_size;
  int32_t device;
  int32_t dense_taxa;       /* > 0: taxon ids beyond 22 bits were renumbered internally at slk_index_finalize (the number of
                               taxonomy nodes); every taxon that crosses this ABI is still the caller's id */
  int32_t bucket_cells;     /* 8-byte cells per bucket: 8 (64-byte buckets; a build option makes it 16) */
  float load_factor;        /* the load the table was sized for: slk_table_config.load_factor, or what the default chose from the
                               device's free memory (runs on parts with different memory are comparable by this) */
  int32_t grown;            /* times the table moved to a larger geometry because a record found no cell within reach
                               (more records than expected_records: the load never fails for that).  Always 0 with several id
                               columns: those tables do not grow */
} slk_index_info;

/* OrdinalSpan (S/slacken/package.scala:61-62) without the title; ordinal = position in the read's span list.
 * For flag != SLK_FLAG_SEQUENCE the reference draws a random minimizer (S/slacken/Supermers.scala:34-42,53-56)
 * that can never be observed; this engine writes key = 0. */
typedef struct {
  int64_t key; /* left-aligned, exactly the value of Parquet column id1 */
  int32_t kmers;
  int8_t flag;
  uint8_t distinct;
  uint16_t pad;
} slk_span;

/* TaxonHit (S/slacken/KeyValueIndex.scala:436-441); distinct/ordinal are implied by position. */
typedef struct {
  int32_t taxon;
  int32_t count;
} slk_hit;

int32_t slk_device_count(void);
const char *slk_last_error(void);
const char *slk_version(void);

/* Pinned host memory.  The host entry points accept any host memory; buffers that come from slk_host_alloc (or were
 * registered with slk_host_register: long-lived caller buffers, e.g. a JVM direct ByteBuffer) are DMA'd from and to
 * directly, at PCIe rate, instead of being copied through the stream's staging buffers.  A pointer anywhere inside such a
 * buffer qualifies.  slk_host_free takes the pointer slk_host_alloc returned / slk_host_register was given. */
int32_t slk_host_alloc(size_t bytes, void **out);
int32_t slk_host_register(void *ptr, size_t bytes);
int32_t slk_host_free(void *ptr);

/* ---- index: replaces KeyValueIndex.load / loadRecords (S/slacken/KeyValueIndex.scala:150-159,413-426) ----
 * Windows: k - m + 1 m-mers, at most 512 -- and with one id column at most what a workgroup's LDS holds of the staged scan's ring, 512
 * bytes per m-mer of the window: 320 m-mers on MI355X (160 KiB).  A wider window is refused here (SLK_E_UNSUPPORTED, the numbers in
 * the message), not at the first classify call. */
int32_t slk_index_create(const slk_params *params, const slk_table_config *cfg, int32_t device, slk_index **out);
/* Append records (id1: int64 left-aligned minimizer, taxon: int32) -- the rows of the Parquet table, in any order
 * and any chunking (one call per bucket file is the intended use).  Keys are unique (guaranteed by makeRecords'
 * groupBy, KeyValueIndex.scala:85-93).  Records with taxon == NONE are skipped (indistinguishable from a miss).
 * A table that runs out of reach for a record grows (twice the buckets) and the call goes on.  If the growth fails, one of two
 * things holds.  While both tables fit the device, and whenever the failure comes before the old table is touched (no larger
 * geometry, no memory for the pieces), the index keeps its old table intact and only this call fails.  When the records had to
 * wait in host memory -- the old table is freed before the new one can be allocated -- they are lost with the failure: the
 * index is SPENT, every later call that takes it except slk_index_destroy returns SLK_E_STATE, and the load must be repeated
 * (with a larger slk_table_config.expected_records).  The same holds for the other calls that add records.
 * Several id columns (m > 32; keys: id_longs words per record, row-major): the table does not grow.  It takes records up to its
 * number of slots, the power of two at or above 2 x expected_records (slk_index_info: buckets x bucket_cells); a record beyond
 * that finds no slot, the call returns SLK_E_CAPACITY -- the records that found a slot stay --, and so does every later call that
 * adds records and slk_index_finalize: the load must be repeated with a larger expected_records.  duplicate_keys counts, and the
 * first record of a key is kept, as with one id column.  A negative taxon is SLK_E_INVALID: slk_index_append then stores nothing
 * of the call's chunk; slk_index_append_device, whose taxa the host never sees, skips those records on the device, stores the
 * others and returns SLK_E_INVALID. */
int32_t slk_index_append(slk_index *ix, const int64_t *keys, const int32_t *taxa, uint64_t n);
int32_t slk_index_append_device(slk_index *ix, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n);
/* Table-sharded libraries (a table beyond one GPU's memory; BASELINE.json configs[3], the exchange that replaces the shuffle of
 * the join at S/slacken/Classifier.scala:84): this index keeps only the records whose key falls to `shard` of `n_shards`
 * (slk_shard_of) and drops the others where they arrive, in slk_index_append[_device] and slk_index_add_sequences[_device] alike --
 * every rank / device is handed the same record stream or the same genomes and ends up with its share.  Call before the first
 * record; slk_table_config.expected_records then bounds this shard's records. */
int32_t slk_index_set_shard(slk_index *ix, uint32_t shard, uint32_t n_shards);
/* parents[t] = parent taxon, parents[ROOT] = NONE, unused ids = NONE: Taxonomy.parents (S/slacken/Taxonomy.scala:81-109,159);
 * replaces the bcTaxonomy broadcast (KeyValueIndex.scala:44-47). */
int32_t slk_index_set_taxonomy(slk_index *ix, const int32_t *parents, int32_t T);
/* Library construction from taxon-labelled sequences (BASELINE config 5, the dynamic 2-step library): every super-mer's
 * minimizer of every sequence, labelled with the sequence's taxon, merged per minimizer by LCA -- SplitterMinimizers.find
 * (S/slacken/Minimizers.scala:43-76) + groupBy(id).agg(TaxonLCA) (KeyValueIndex.makeRecords, KeyValueIndex.scala:85-93;
 * LowestCommonAncestor.scala:152-170).  Sequences are split around anything that is not ACGTU (either case), as
 * InputReader.removeInvalid does for library input (S/kmers/input/InputReader.scala:60-72); they must be free of
 * whitespace.  Sequence i is bases[offsets[i] .. offsets[i+1]) with taxon taxa[i]; sequences with taxon NONE are
 * skipped (the reference filters on Taxonomy.isDefined, KeyValueIndex.scala:118-120 -- the caller applies that filter).
 * Needs the taxonomy (slk_index_set_taxonomy) and an unfinalized index whose slk_table_config.expected_records bounds
 * the number of distinct minimizers.  May be called any number of times, also mixed with slk_index_append of records
 * whose keys do not occur in the sequences; the result does not depend on the order or batching of the calls.  Records whose keys
 * may occur in the sequences go in through slk_index_merge_records, which merges by LCA as this call does. */
int32_t slk_index_add_sequences(slk_index *ix, const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa,
                                uint64_t n_sequences);
/* The same with the bases already resident on the index's GPU (d_bases: device pointer to offsets[n_sequences] bytes;
 * offsets and taxa: host arrays).  The sequences are scanned where they lie. */
int32_t slk_index_add_sequences_device(slk_index *ix, const uint8_t *d_bases, const uint64_t *offsets, const int32_t *taxa,
                                       uint64_t n_sequences);
/* Ends the build.  If the taxon ids need more than 22 bits (slk_table_config.max_taxon >= 2^22), the taxonomy has been set
 * and every record's taxon is one of its nodes, the table is renumbered here to dense internal ids (one pass over the
 * cells) so that the fast kernels apply; ids crossing the ABI are unaffected.  Set the taxonomy BEFORE finalizing to get
 * this; it cannot be replaced afterwards on such an index. */
int32_t slk_index_finalize(slk_index *ix);
/* The table's records as (key, taxon) arrays -- what KeyValueIndex.writeRecords would persist (KeyValueIndex.scala:125-139);
 * keys: id_longs words per record, row-major.  The order is unspecified (a set).  *n_records receives the number of records; if it exceeds capacity only the first
 * `capacity` were written and SLK_E_CAPACITY is returned.  keys/taxa may be NULL with capacity 0 to query the count. */
int32_t slk_index_export(const slk_index *ix, int64_t *keys, int32_t *taxa, uint64_t capacity, uint64_t *n_records);
/* The records of table buckets [bucket0, bucket1), optionally grouped by Spark's bucket: the device half of
 * KeyValueIndex.writeRecords (KeyValueIndex.scala:125-139), which persists the records CLUSTERED BY (id1) INTO n BUCKETS.  A table
 * leaves the device piece by piece through this call (slk_index_export stages the whole record set on the device and again on
 * the host): slk_index_info.buckets and bucket_cells bound the range and the count -- (bucket1 - bucket0) * bucket_cells records
 * is an upper bound, and a caller who sizes by it never sees SLK_E_CAPACITY.  Records and taxa as slk_index_export gives them (the
 * caller's ids, also on an index renumbered by slk_index_finalize); the pieces of a tiling of [0, buckets) hold every record once.
 *   n_groups == 0   any order; group_offsets is ignored (may be NULL).
 *   n_groups >= 1   the records are ordered by g = pmod(Murmur3_x86_32.hashLong(key, seed 42), n_groups), the bucket Spark computes
 *                   for a long column; group_offsets[0 .. n_groups] receives where each group starts, group_offsets[n_groups] ==
 *                   *n_records.  The order inside a group is unspecified.  A grouped call covers at most 2^32 cells
 *                   (SLK_E_INVALID beyond: pieces are the intended use).
 *   capacity        *n_records is always the full count of the range.  If it exceeds a capacity > 0, SLK_E_CAPACITY is returned and
 *                   only the count means anything.  keys / taxa may be NULL with capacity 0 to query the count (group_offsets is
 *                   not written then).  An empty range is SLK_OK with 0 records.
 *   errors          SLK_E_INVALID: bucket0 > bucket1, bucket1 > buckets, n_groups < 0, a grouped call over more than 2^32 cells;
 *                   SLK_E_UNSUPPORTED: several id columns; SLK_E_STATE: a spent index.
 * Works before and after slk_index_finalize, after the table has grown, and on a dynamic library (slk_index_add_sequences); a shard
 * of a table-sharded library (slk_index_set_shard) exports its own share.  The index is not changed.  Two passes over the range's
 * cells and a scan on the device (export.hip); device staging is what the range needs -- 12 bytes per possible record and the group
 * counters --, never the table's record count.  Up to SLK_EXPORT_LDS_GROUPS groups (environment; default 4096) are counted in the
 * blocks' LDS.  Synchronous, on the build stream; not to be called while another thread adds records to the same index. */
int32_t slk_index_export_range(const slk_index *ix, uint64_t bucket0, uint64_t bucket1, int32_t n_groups, int64_t *keys, int32_t *taxa,
                               uint64_t capacity, uint64_t *group_offsets, uint64_t *n_records);
/* Records per taxon of the resident table: replaces records.groupBy("taxon").agg(count("*")) -- KeyValueIndex.scala:241
 * (showIndexStats) and :278 (report); the depth histograms (:326-336) are sums of the same pairs.  One streaming pass over the
 * table on the device (taxstats.hip); nothing but the pairs crosses to the host.  (taxa[i], counts[i]) for i < *n_taxa, ascending
 * taxon, ids as the caller gave them (also on an index renumbered to dense ids by slk_index_finalize); *n_records (nullable) = the
 * sum of the counts.  The capacity protocol of slk_index_export: taxa/counts may be NULL with capacity 0 to query *n_taxa; if
 * *n_taxa exceeds a capacity > 0 the first `capacity` pairs were written and SLK_E_CAPACITY is returned.  Works before and after
 * slk_index_finalize, after the table has grown, and on a dynamic library (slk_index_add_sequences); a shard of a table-sharded
 * library (slk_index_set_shard) counts its own share.  The index is not changed.  One id column only (SLK_E_UNSUPPORTED
 * otherwise, as the staged device entries); a spent index returns SLK_E_STATE.  Synchronous; not to be called while another
 * thread adds records to the same index. */
int32_t slk_index_taxon_counts(const slk_index *ix, int32_t *taxa, uint64_t *counts, uint64_t capacity, uint64_t *n_taxa,
                               uint64_t *n_records);
/* A library with more mask spaces from a resident one: replaces KeyValueIndex.respace (S/slacken/KeyValueIndex.scala:353-384; the loop
 * of respaceMultiple :390-404 is the caller's) -- every record's minimizer ANDed with the space mask of `spaces` spaces and the
 * records regrouped by minimizer with the LCA of their taxa (:370-379), without a second look at the genomes.  One pass over the
 * source's table on the device (respace.hip): no record crosses to the host.  *out is a NEW index on the source's device: the source's
 * slk_params with `spaces` replaced, the source's taxonomy, finalized -- ready for slk_stream_create, slk_index_export,
 * slk_index_taxon_counts -- and independent of the source (either may be destroyed first).  The source is not changed.
 *   cfg         NULL: the table is sized for the source's record count (an upper bound), at the default load factor.  Otherwise
 *               expected_records (0: as NULL) and load_factor are taken; max_taxon is ignored: the taxon field is the source's.
 *   info        records = the distinct masked minimizers; duplicate_keys = 0 (merging is the purpose); grown = how often the pass was
 *               repeated into twice the buckets because a record found no cell within reach (the source is only read and the pass
 *               is idempotent, so it simply runs again).  SLK_RESPACE_BUCKETS (environment) sets the buckets of the first table.
 *   errors      SLK_E_STATE: source not finalized, without a taxonomy, or spent; SLK_E_INVALID: spaces <= the source's (the reference
 *               throws "not meaningful") or > m / 2 (SpacedSeed's assert); SLK_E_UNSUPPORTED: several id columns, or a shard of a
 *               table-sharded library (a key's owner is fmix64(key) mod n and the key changes: a respaced shard is no shard of the
 *               respaced library); SLK_E_HIP: e.g. both tables do not fit the device.  On every failure *out is NULL and the source
 *               is as it was.
 * The reference's remark that the result equals a library built at `spaces` from the genomes is not exact: this is
 * respace, not build.  Synchronous, on the source's build stream; not to be called while another thread adds records to the source. */
int32_t slk_index_respace(const slk_index *src, int32_t spaces, const slk_table_config *cfg /* nullable */, slk_index **out);
/* Libraries united: records merged into what the table holds, per key by LCA.  A record's taxon is the LCA of the taxa of all
 * sequences that hold its minimizer (KeyValueIndex.makeRecords, S/slacken/KeyValueIndex.scala:85-93: groupBy(id).agg(TaxonLCA);
 * LowestCommonAncestor.scala:152-170), and LCA is associative, commutative and idempotent.  So after ANY sequence of
 * slk_index_merge_records[_device], slk_index_merge_index and slk_index_add_sequences[_device] calls the table holds, per key, the
 * LCA of every taxon that arrived for it -- in any order of the calls, any chunking, and with keys repeated inside one call.  Under
 * one taxonomy the merge of build(A) and build(B) is therefore the record set of build(A u B).  slk_index_info.records
 * counts the distinct keys; duplicate_keys is not touched (merging is the purpose, as in the builder).
 *   destination   one id column, not finalized, with its taxonomy set (slk_index_set_taxonomy).  A shard (slk_index_set_shard) merges
 *                 its share and drops the rest.  The table grows when a record finds no cell within reach, as with slk_index_append:
 *                 no call fails for an expected_records that was too low.
 *   taxa          taxon NONE is skipped, as slk_index_append skips it.  Every other taxon t is translated as remap[t] where a remap
 *                 is set (slk_index_set_merge_remap: t >= n or remap[t] == 0 means the destination has no such node; NULL / 0 clears
 *                 it; the table is copied to the device once, there) and must then be a node the destination's taxonomy defines
 *                 (1 <= t' < T, ROOT or with a parent) that fits the taxon field (slk_table_config.max_taxon).  Records that fail --
 *                 a negative taxon among them -- are not stored; the call stores all others and then returns SLK_E_INVALID with
 *                 "N records name a taxon the destination's taxonomy does not define (smallest: T)", T in the caller's ids.  The
 *                 index stays usable.
 *   merge_records keys / taxa in host memory, staged in chunks as slk_index_append stages them; _device: arrays on the index's GPU.
 *   merge_index   the records of another resident index on the same device: its table is walked where it lies (merge.hip; the walk
 *                 of slk_index_respace) and no record crosses to the host.  The source may be finalized or not, renumbered to dense
 *                 ids by slk_index_finalize or not (its taxa travel as the caller's ids), a dynamic library or a shard.  It is only
 *                 read.
 *   errors        SLK_E_STATE: destination finalized or without a taxonomy; either index spent.  SLK_E_UNSUPPORTED: several id
 *                 columns on either side, as slk_index_respace and slk_index_export_range.  SLK_E_INVALID for merge_index: src == dst,
 *                 different devices, splitters that differ in k, m, spaces, canonical or xor_mask.  n == 0 is SLK_OK.
 * Synchronous, on the destination's build stream; not to be called while another thread adds records to either index. */
int32_t slk_index_set_merge_remap(slk_index *ix, const int32_t *remap /* nullable */, int32_t n);
int32_t slk_index_merge_records(slk_index *ix, const int64_t *keys, const int32_t *taxa, uint64_t n);
int32_t slk_index_merge_records_device(slk_index *ix, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n);
int32_t slk_index_merge_index(slk_index *dst, const slk_index *src);
int32_t slk_index_get_info(const slk_index *ix, slk_index_info *out);
/* The table's bucket choice as host arithmetic (no GPU): the range reduction of a 64-bit hash onto ANY number of buckets
 * (32 <= nbuckets <= 2^32) -- home = (top q bits of hash) * nbuckets >> q, q = ceil(log2(nbuckets)) -- with the remainder a cell
 * keeps so that (home, rem) still identifies the hash (the table is lossless, unlike a compact hash table with truncated keys),
 * and its inverse.  For tests and for tools that lay out tables offline. */
int32_t slk_table_slot(uint64_t nbuckets, uint64_t hash, uint32_t *home, uint64_t *rem);
int32_t slk_table_hash_of(uint64_t nbuckets, uint32_t home, uint64_t rem, uint64_t *hash);
/* Point lookups (host arrays), for tests and tooling: taxon or NONE per key -- the left join + spanToHit's
 * otherwise(NONE) (KeyValueIndex.scala:176-185). */
int32_t slk_index_lookup(const slk_index *ix, const int64_t *keys, uint64_t n, int32_t *out_taxa);
void slk_index_destroy(slk_index *ix);

int32_t slk_stream_create(slk_index *ix, slk_stream **out);
int32_t slk_stream_synchronize(slk_stream *st);
/* on != 0: the hit lists slk_classify_batch / slk_classify_batch_packed return on this stream are merged as TaxonCounts.fromHits
 * merges them (S/slacken/TaxonCounts.scala:31-48) -- adjacent TaxonHits of one taxon (AMBIGUOUS included; a MATE_PAIR_BORDER stands
 * alone) become one entry whose count is the sum of theirs -- and out_hit_offsets index the merged entries.  It is the list
 * ClassifiedRead.outputLine prints (pairsInOrderString :94-110, lengthString) at a fifth to a tenth of the bytes over the link;
 * ordinals and `distinct` of single spans are no longer implied by position, so lists that will be regrouped by title
 * (slk_classify_hits) or counted per minimizer must stay un-merged (the default).  A call that asks for the offsets alone
 * (out_hits == NULL) still counts the single spans. */
int32_t slk_stream_set_merged_hits(slk_stream *st, int32_t on);
void *slk_stream_hip_stream(slk_stream *st); /* the hipStream_t, for event timing by the caller */
void slk_stream_destroy(slk_stream *st);

/* ---- kernel-1-only entry: replaces KeyValueIndex.getSpans (S/slacken/KeyValueIndex.scala:163-173), i.e.
 * Supermers.splitFragment + Supermers.spans (S/slacken/Supermers.scala:49-97,113-125) over
 * MinSplitter.splitEncode (S/kmers/minimizer/MinSplitter.scala:98-101).
 * bases: concatenated ASCII reads WITHOUT whitespace (getSpans' precondition, KeyValueIndex.scala:162);
 * offsets[R+1]; mate_bases/mate_offsets: second mates with the same indexing, or NULL for single-end.
 * out_span_offsets[R+1]; out_spans[spans_capacity] in read order then ordinal order. */
int32_t slk_spans_batch(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets,
                        const uint8_t *mate_bases, const uint64_t *mate_offsets, uint64_t R,
                        uint64_t *out_span_offsets, slk_span *out_spans, uint64_t spans_capacity);

/* The same for any number of id columns (KeyValueIndex.scala:49: idLongs = ceil(m / 32)): out_keys[spans * id_longs] receives
 * OrdinalSpan.minimizer row by row (id1..idN, left-aligned words), out_spans[i].key = id1.  With one id column it equals
 * slk_spans_batch plus the copy of the keys. */
int32_t slk_spans_batch_wide(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets,
                             const uint8_t *mate_bases, const uint64_t *mate_offsets, uint64_t R,
                             uint64_t *out_span_offsets, slk_span *out_spans, int64_t *out_keys, uint64_t spans_capacity);

/* ---- the hot path: replaces Classifier.classify (S/slacken/Classifier.scala:114-121) =
 * collectHitsBySequence (:70-96: getSpans -> join -> spanToHit -> group) + classifyHits (:124-147) ->
 * Classifier.classify (object, :439-454) -> TaxonCounts (S/slacken/TaxonCounts.scala:31-87) ->
 * LowestCommonAncestor.resolveTree (S/slacken/LowestCommonAncestor.scala:91-146).
 * One call = one batch of R fragments and C confidence thresholds.
 *   out_taxon[C*R], out_classified[C*R]  (threshold-major): ClassifiedRead.taxon / .classified
 *   out_num_distinct[R]  hits with distinct && taxon != NONE        (Classifier.scala:94)
 *   out_total_kmers[R]   TaxonCounts.totalKmers                      (TaxonCounts.scala:84-87)
 *   out_hit_offsets[R+1], out_hits[hits_capacity] (both nullable): un-merged TaxonHits in ordinal order incl.
 *     the -1 / -2 entries.  A read with out_hit_offsets[r+1] == out_hit_offsets[r] produced no span: the reference
 *     emits NO row for it (grouping is over span rows, Classifier.scala:92) -- the host must drop it.
 *     out_hit_offsets without out_hits: the number of spans per read only (offsets[r+1] - offsets[r]); the lists are then
 *     neither built nor copied, and the call takes the kernels that do not keep span order (the fastest route).
 * The caller's buffers may be any host memory: the copies go through pinned staging buffers of the stream.
 * Synchronous, also when it fails: on every return, with an error too, nothing is queued any more that reads the caller's
 * input or writes its output, so the buffers may be freed (the same holds for slk_classify_batch_packed, slk_classify_hits
 * and slk_spans_batch[_wide]).
 * Sample-id regex, titles, duplicate-title merging and text formatting stay on the host. */
int32_t slk_classify_batch(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets,
                           const uint8_t *mate_bases, const uint64_t *mate_offsets, uint64_t R,
                           int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon,
                           uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers,
                           uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity);

/* The same call with the reads in the engine's own 3-bit form -- InputFragment.nucleotides (S/kmers/minimizer/MinSplitter.scala:31-32)
 * already encoded as BitRepresentation.charToTwobit encodes them (S/kmers/util/BitRepresentation.scala:127-135: A = 0, C = 1, G = 2,
 * T / U = 3, either case) with the isValid test (:140-143) as one bit per base -- so that a batch costs 6 bytes per 16 bases on the
 * PCIe link instead of 16: the call a JNI shim makes is bound by that link (slk_classify_batch from pinned memory: 305 M reads/s of
 * 150 bp against the kernels' 1 100 M).  Base p of the concatenated reads (the p that offsets[] counts) is described by bits
 * 2 (p % 16) .. 2 (p % 16) + 1 of codes[p / 16] and bit p % 16 of valid[p / 16]; codes of invalid bases are ignored; both arrays
 * hold ceil(offsets[R] / 16) words (mates likewise).  Results are those of slk_classify_batch on any text with the same codes and
 * validity.  slk_pack_bases makes the form from text (AVX2 + BMI2 where the CPU has them, several threads for large inputs). */
int32_t slk_classify_batch_packed(slk_index *ix, slk_stream *st, const uint32_t *codes, const uint16_t *valid, const uint64_t *offsets,
                                  const uint32_t *mate_codes, const uint16_t *mate_valid, const uint64_t *mate_offsets, uint64_t R,
                                  int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon,
                                  uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers,
                                  uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity);
int32_t slk_pack_bases(const uint8_t *bases, uint64_t n, uint32_t *codes, uint16_t *valid);

/* ---- batches in flight: a submit call and a collect call, so that ONE caller thread (a Spark task thread behind a JNI shim has no
 * callbacks) keeps several batches of Classifier.classify on the device at once -- the reads of batch i+1 go up and the rows of
 * batch i-1 come down while batch i is classified -- and a wire form that carries only what holds information.
 *
 * slk_reads: one side (the reads, or their mates) of a batch.
 *   the bases    exactly one of `bases` (ASCII, as slk_classify_batch; no validity arrays then) and `codes` (slk_pack_bases' words).
 *   validity     with codes: `valid`, the dense words of slk_classify_batch_packed; or valid == NULL: every base is valid except in
 *                the n_exc words exc_word[] (strictly ascending, each < ceil(total / 16)), whose validity bits are exc_bits[] -- the
 *                bits of a last, partial word past the side's last base are ignored.  n_exc == 0 takes NULL for both.  `valid`
 *                together with exceptions is SLK_E_INVALID.  slk_pack_bases_sparse makes this form.
 *   the lengths  exactly one of `offsets` ([R + 1], as slk_classify_batch), `lengths` ([R]) and uniform_len > 0 (every read has that
 *                many bases; nothing is sent).  The device turns lengths into offsets.
 * A side in a compact form (lengths, uniform_len or exceptions) holds fewer than 2^32 bases and the batch fewer than 2^32 reads:
 * SLK_E_INVALID beyond, before anything is queued or allocated.
 *
 * slk_pipe_create   `depth` slots (1..8), each with everything an slk_stream owns; a slot's buffers keep their size from ticket to
 *                   ticket.  One thread at a time uses a pipe; several pipes on one finalized index may be used from several threads.
 * slk_pipe_submit   queues the upload, the expansion of the compact forms, the classify kernels and the download of the result rows
 *                   into memory of the pipe, and returns WITHOUT waiting for the device; *ticket names the batch.  hits: 0 = none,
 *                   1 = the number of spans per read only, 2 = the hit lists (as slk_pipe_set_merged_hits stood at the submit).  It
 *                   writes no result buffer of the caller's -- it takes none.  With `depth` tickets uncollected it returns SLK_E_STATE,
 *                   changes nothing and does not wait for a slot.  A refused submit (SLK_E_INVALID, SLK_E_STATE) has queued nothing.
 *   input lifetime  PAGEABLE input is free again when submit returns: it has been copied into pinned staging of the pipe (a batch
 *                   larger than that staging waits for its own earlier pieces' DMA, never for a kernel).  Memory of slk_host_alloc /
 *                   slk_host_register is read by DMA, later: it must stay UNCHANGED until slk_pipe_collect of that ticket returns.
 * slk_pipe_collect  waits for that ticket only, classifies the batch again where slk_classify_batch would (a taxon map that
 *                   overflowed), builds the hit lists if they were asked for, copies everything out and frees the slot.  Tickets may
 *                   be collected in any order.  Results: those of slk_classify_batch on the same reads, thresholds and
 *                   min_hit_groups, bit for bit (out_taxon[C*R] .. as there; out_num_distinct, out_total_kmers, out_hit_offsets and
 *                   out_hits nullable).  A collected or unknown ticket: SLK_E_STATE.  hits_capacity too small: SLK_E_CAPACITY with
 *                   out_hit_offsets filled -- the ticket STAYS collectable, come back with a larger buffer.  A device-side failure
 *                   of the batch (SLK_E_HIP; SLK_E_INVALID: lengths that no longer sum to what submit saw) is reported here, and the
 *                   slot is freed.
 * slk_pipe_pending  the number of uncollected tickets.
 * slk_pipe_destroy  drains what is pending and frees everything. */
typedef struct slk_pipe slk_pipe;
typedef struct {
  const uint8_t *bases;
  const uint32_t *codes;
  const uint16_t *valid;
  const uint32_t *exc_word;
  const uint16_t *exc_bits;
  uint64_t n_exc;
  const uint64_t *offsets;
  const uint32_t *lengths;
  uint32_t uniform_len;
} slk_reads;
int32_t slk_pipe_create(slk_index *ix, int32_t depth, slk_pipe **out);
int32_t slk_pipe_set_merged_hits(slk_pipe *p, int32_t on); /* as slk_stream_set_merged_hits, for the tickets submitted from now on */
int32_t slk_pipe_submit(slk_pipe *p, uint64_t R, const slk_reads *reads, const slk_reads *mates /* nullable */, int32_t min_hit_groups,
                        const double *thresholds, int32_t C, int32_t hits, uint64_t *ticket);
int32_t slk_pipe_collect(slk_pipe *p, uint64_t ticket, int32_t *out_taxon, uint8_t *out_classified, int32_t *out_num_distinct,
                         int32_t *out_total_kmers, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t hits_capacity);
int32_t slk_pipe_pending(const slk_pipe *p, int32_t *n_pending);
void slk_pipe_destroy(slk_pipe *p);
/* slk_pack_bases with the validity as slk_reads takes it: the same codes[ceil(n / 16)]; word w is an exception iff some base p < n of
 * it is invalid, and its bits are the dense word's.  More exceptions than exc_capacity: SLK_E_CAPACITY with *n_exc = the number
 * needed (the first exc_capacity are written, the codes in full). */
int32_t slk_pack_bases_sparse(const uint8_t *bases, uint64_t n, uint32_t *codes, uint32_t *exc_word, uint16_t *exc_bits,
                              uint64_t exc_capacity, uint64_t *n_exc);

/* ---- FASTA / FASTQ text parsed on the device: replaces FastaTextInput and FastqTextInput (S/kmers/input/FileInputs.scala:155-183,
 * 188-221) -- the records of a text as the layout the classify entry points take (bases without whitespace, offsets[R+1]) plus
 * where every record's title lies in the text.  Per byte:
 *   FASTQ  a line ends at \n, \r\n or a lone \r; a last line without a terminator is a line, the empty piece after the last
 *          terminator is not.  Line i starts a record iff its first byte is '@', line i+2 exists and its first byte is '+' (the
 *          window slides by ONE line, :204-221); the sequence is line i+1 verbatim, the title line i after the '@' up to the first
 *          space.
 *   FASTA  the text is cut at every '>' (:166); the title is what precedes the piece's first \n or \r, up to the first space; the
 *          sequence every later byte of the piece that is neither \n nor \r; a piece is a record iff its sequence is not empty.
 *   final = 0  the text is a chunk of a longer one: a FASTQ line counts only when its terminator lies inside the chunk (a \r on
 *          the last byte is undecided) and a record only when lines i, i+1 and i+2 are all there; a FASTA record only when the '>'
 *          that ends it is inside the chunk.  consumed = the first byte that no taken record or skipped line owns (FASTQ: the start
 *          of the first line whose window could not be decided; FASTA: the '>' that opens the first record not taken, 0 if the chunk
 *          holds none): the caller puts text[consumed, n) in front of the next chunk, and any sequence of such calls, the last one
 *          with final = 1, yields the records of the whole text in order.  consumed == 0 on a non-final chunk: the chunk must grow.
 * Limits: n < 2^32 per call (SLK_E_INVALID beyond); two mate files go through the paired entries below.  title_pos[r] is a position in `text` (FASTQ: behind the '@'),
 * title_len[r] the bytes of the title.  The counts record is four uint64: records, bases, consumed, overflow.
 *   slk_parse_device  every pointer on the stream's device, d_text aligned to 16 bytes, nothing past text[n) is read; asynchronous
 *                     on st.  d_offsets holds records_capacity + 1 entries.  More records than records_capacity or more bases than
 *                     bases_capacity: overflow = 1, records and bases say what was needed, consumed = 0, and none of the output
 *                     arrays is written.  Scratch is the stream's, sized from n (FASTQ 8 bytes per byte of text, FASTA 20 bytes per
 *                     4 KiB) -- no other allocation.
 *   slk_parse_text    the same from and to host memory, synchronous: the parser alone.  Overflow is SLK_E_CAPACITY, with
 *                     *out_records and *out_n_bases what the capacities would have to be.
 *   slk_classify_text uploads the text, parses it on the device and classifies the records where they lie, as
 *                     slk_classify_batch_device would: what slk_classify_batch returns for the parsed reads (out_taxon and
 *                     out_classified are [C * *out_records], threshold-major with stride *out_records; hit lists follow
 *                     slk_stream_set_merged_hits) plus out_offsets[R+1] and the titles' positions.  Every per-record array holds
 *                     records_capacity entries (out_offsets and out_hit_offsets one more); more records is SLK_E_CAPACITY with
 *                     *out_records the number needed.  Synchronous on every return, as slk_classify_batch.  One id column only
 *                     (SLK_E_UNSUPPORTED otherwise).
 *   slk_parse_tile_bytes  the bytes of text one workgroup takes at a time (tests place record borders on its multiples). */
#define SLK_FORMAT_FASTA 0
#define SLK_FORMAT_FASTQ 1
uint32_t slk_parse_tile_bytes(void);
int32_t slk_parse_device(slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t format, int32_t final, uint8_t *d_bases,
                         uint64_t bases_capacity, uint64_t *d_offsets, uint64_t *d_title_pos, uint32_t *d_title_len,
                         uint64_t records_capacity, uint64_t *d_counts);
int32_t slk_parse_text(slk_stream *st, const uint8_t *text, uint64_t n, int32_t format, int32_t final, uint8_t *out_bases,
                       uint64_t *out_offsets, uint64_t *out_title_pos, uint32_t *out_title_len, uint64_t bases_capacity,
                       uint64_t records_capacity, uint64_t *out_records, uint64_t *out_n_bases, uint64_t *out_consumed);
int32_t slk_classify_text(slk_index *ix, slk_stream *st, const uint8_t *text, uint64_t n, int32_t format, int32_t final,
                          int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *out_taxon, uint8_t *out_classified,
                          int32_t *out_num_distinct, int32_t *out_total_kmers, uint64_t *out_offsets, uint64_t *out_title_pos,
                          uint32_t *out_title_len, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t records_capacity,
                          uint64_t hits_capacity, uint64_t *out_records, uint64_t *out_consumed);

/* ---- two mate texts paired on the device: replaces PairedInputReader.getFragments (S/kmers/input/InputReader.scala:105-131) while
 * both files list their mates in the same order.  The reference inner-joins the two files' records on the header with
 * one trailing "/1" removed in file 1 and one trailing "/2" in file 2; this is the lockstep walk of that join.  With R1, R2 the records
 * the parser above takes from text1 / text2 (each with its own format and final flag) and M = min(R1, R2):
 *   key1(i)   the title of record i of text 1 without ONE trailing "/1" ("a/1/1" -> "a/1", "/1" -> ""); key2(i) the same with "/2".
 *             A "/2" in text 1 or a "/1" in text 2 stays.  Keys are equal iff their lengths and bytes are.
 *   pairs     P = the number of leading i < M with key1(i) == key2(i); mismatch = (P < M).  Fragments 0 .. P-1 are record i of text 1
 *             as the read and record i of text 2 as its mate.
 *   consumed  where the next chunk of either text starts: R_i > P -- the byte that opens record P of text i (title_pos_i[P] - 1, or 0
 *             for a FASTA record that opens the text without '>'); R_i == P -- the single-text parser's consumed.  Both record rules
 *             are local, so parsing on from a record's opener yields the same records.  P == 0 without a mismatch: a side has no
 *             record; if it is not final its chunk must grow, if it is final the file pair is finished (the inner join drops what the
 *             other file still holds).
 * slk_pair_record is also the layout of the eight uint64 the device writes.  With SLK_E_CAPACITY records1 / records2 / bases1 / bases2
 * say what the capacities would have to be and the rest is 0.
 *   slk_pair_device        every pointer on the stream's device, asynchronous on st (InputReader.scala:105-131): the compare and
 *                          finish passes over the outputs of two slk_parse_device calls that did not overflow; R1, R2 are their
 *                          record counts, d_counts1 / d_counts2 their counts records, d_pair eight uint64.  d_title_len1 is
 *                          rewritten: every record of text 1 loses its "/1".  Nothing outside text1[0, n1), text2[0, n2) is read.
 *   slk_parse_text_paired  from and to host memory, synchronous (InputReader.scala:105-131): the two parses and the pairing alone.
 *                          out_bases / out_offsets[P+1] and out_mate_bases / out_mate_offsets[P+1] hold the P pairs, out_title_pos /
 *                          out_title_len the (stripped) titles of all R1 records of text 1 -- the caller needs those beyond P when
 *                          text 2 is exhausted.  More records or bases than a capacity on either side: SLK_E_CAPACITY, no output
 *                          array is written.
 *   slk_classify_text_paired  uploads both texts, parses, pairs and classifies the P fragments where they lie, mates included, by
 *                          the route of slk_classify_text (InputReader.scala:105-131): what slk_classify_text returns for P records
 *                          (stride P) plus out_mate_offsets[P+1], the titles of all R1 records and the pair record.  records_capacity
 *                          bounds the records of EITHER text.  A mismatch is not an error: SLK_OK, the flag set, P pairs classified.
 *                          Synchronous on every return; SLK_E_CAPACITY, SLK_E_UNSUPPORTED and SLK_E_INVALID as slk_classify_text. */
typedef struct slk_pair_record {
  uint64_t pairs, mismatch, consumed1, consumed2, records1, records2;
  uint64_t bases1, bases2;   /* offsets1[pairs], offsets2[pairs]: the bases of the reads and of the mates */
} slk_pair_record;
int32_t slk_pair_device(slk_stream *st, const uint8_t *d_text1, uint64_t n1, const uint64_t *d_title_pos1, uint32_t *d_title_len1,
                        const uint64_t *d_offsets1, const uint64_t *d_counts1, uint64_t R1, const uint8_t *d_text2, uint64_t n2,
                        const uint64_t *d_title_pos2, const uint32_t *d_title_len2, const uint64_t *d_offsets2, const uint64_t *d_counts2,
                        uint64_t R2, uint64_t *d_pair);
int32_t slk_parse_text_paired(slk_stream *st, const uint8_t *text1, uint64_t n1, int32_t format1, int32_t final1, const uint8_t *text2,
                              uint64_t n2, int32_t format2, int32_t final2, uint8_t *out_bases, uint64_t *out_offsets,
                              uint8_t *out_mate_bases, uint64_t *out_mate_offsets, uint64_t *out_title_pos, uint32_t *out_title_len,
                              uint64_t bases_capacity1, uint64_t records_capacity1, uint64_t bases_capacity2, uint64_t records_capacity2,
                              slk_pair_record *out_pair);
int32_t slk_classify_text_paired(slk_index *ix, slk_stream *st, const uint8_t *text1, uint64_t n1, int32_t format1, int32_t final1,
                                 const uint8_t *text2, uint64_t n2, int32_t format2, int32_t final2, int32_t min_hit_groups,
                                 const double *thresholds, int32_t C, int32_t *out_taxon, uint8_t *out_classified, int32_t *out_num_distinct,
                                 int32_t *out_total_kmers, uint64_t *out_offsets, uint64_t *out_mate_offsets, uint64_t *out_title_pos,
                                 uint32_t *out_title_len, uint64_t *out_hit_offsets, slk_hit *out_hits, uint64_t records_capacity,
                                 uint64_t hits_capacity, slk_pair_record *out_pair);

/* ---- kernel-3-only entry: Classifier.classify (object, S/slacken/Classifier.scala:439-454) on hit lists the caller holds
 * (host pointers; synchronous): TaxonCounts.toMap/totalKmers + resolveTree + the minHitGroups test for R lists of un-merged
 * hits in ordinal order.  This is what the host uses to reproduce the reference's regrouping by TITLE
 * (groupBy("seqTitle") + collect_list, Classifier.scala:92; sorted by ordinal :136): fragments that share a title are one
 * read there, so the host concatenates their hit lists, sorts them stably by ordinal and classifies the merged list here.
 *   hits[hit_offsets[r] .. hit_offsets[r+1])   list r; taxon AMBIGUOUS / MATE_PAIR_BORDER entries as slk_classify_batch
 *                                              returns them
 *   distinct[i] (nullable)                     OrdinalSpan.distinct of hit i (slk_span.distinct of the same ordinal);
 *                                              NULL = no hit counts as distinct
 *   out_num_distinct[R], out_total_kmers[R]    nullable */
int32_t slk_classify_hits(slk_index *ix, slk_stream *st, uint64_t R, const uint64_t *hit_offsets, const slk_hit *hits,
                          const uint8_t *distinct, int32_t min_hit_groups, const double *thresholds, int32_t C,
                          int32_t *out_taxon, uint8_t *out_classified, int32_t *out_num_distinct, int32_t *out_total_kmers);

/* Same computation with every pointer (bases, offsets, mates, thresholds excepted: host) resident on the index's
 * GPU; asynchronous on st.  d_out_num_hits[R] (nullable) receives the span count per read (0 => no row);
 * d_out_num_probes[R] (nullable) the number of SEQUENCE_FLAG spans = table lookups (the P_r of SURVEY.md 8d).
 * total_bases / total_mate_bases = offsets[R] / mate_offsets[R] (the caller knows them; avoids a D2H sync). */
int32_t slk_classify_batch_device(slk_index *ix, slk_stream *st, const uint8_t *d_bases, const uint64_t *d_offsets,
                                  const uint8_t *d_mate_bases, const uint64_t *d_mate_offsets, uint64_t R,
                                  uint64_t total_bases, uint64_t total_mate_bases, int32_t min_hit_groups,
                                  const double *thresholds, int32_t C, int32_t *d_out_taxon,
                                  uint8_t *d_out_classified, int32_t *d_out_num_distinct,
                                  int32_t *d_out_total_kmers, int32_t *d_out_num_hits,
                                  int32_t *d_out_num_probes);

/* ---- staged device entry points: the same three steps as separate calls, for the TABLE-SHARDED mode (the record
 * table exceeds one GPU's HBM: each rank holds the records whose hash falls to it, minimizers are exchanged with an
 * all-to-all between slk_scan_device and slk_classify_hits_device; SURVEY.md 8e, BASELINE.json configs[3]) and for an
 * index build from sequences.  All pointers are device pointers; asynchronous on st.
 *   span slot of fragment r, span j:  offsets[r] (+ mate_offsets[r] + r when paired) + j   (at most L-k+1 [+1+L2-k+1]
 *   spans per fragment, so slots never overlap); d_span_* must hold total_bases (+ total_mate_bases + R) + 1 entries. */
/* getSpans (KeyValueIndex.scala:163-173): d_span_keys (left-aligned minimizers, 0 for flagged spans),
 * d_span_meta (kmers << 4 | flag << 1 | distinct), d_span_count[R]. */
int32_t slk_scan_device(slk_index *ix, slk_stream *st, const uint8_t *d_bases, const uint64_t *d_offsets,
                        const uint8_t *d_mate_bases, const uint64_t *d_mate_offsets, uint64_t R,
                        uint64_t *d_span_keys, int32_t *d_span_meta, int32_t *d_span_count);
/* the join (Classifier.scala:84): taxon or NONE for n minimizers against THIS index's records */
int32_t slk_lookup_device(slk_index *ix, slk_stream *st, const int64_t *d_keys, uint64_t n, int32_t *d_out_taxa);
/* Which rank owns a minimizer in table-sharded mode: fmix64(key) mod n_shards (host helper; the device side of the
 * Python host uses the same bijective mixer) */
uint32_t slk_shard_of(int64_t key, uint32_t n_shards);
/* The fast form of the table-sharded path for fragments of up to 1000 bases (both mates together): ONE scan per batch, and nothing
 * but 8-byte keys and 4-byte taxa on the links -- no span arrays in HBM, no per-probe return addresses, no compaction of the lists.
 * It replaces the shuffle behind the reference's join (S/slacken/Classifier.scala:84-95).  A batch passes through three JOBS, and one
 * slk_shard_step_device call launches up to three jobs of three different batches as ONE kernel, so that the latency-bound ones hide
 * behind the scan the way the probes of slk_classify_batch_device do:
 *   EMIT    scans the batch's fragments and appends every minimizer to the send region of its owner (slk_shard_of): d_send_keys is
 *           [n_shards][capacity_per_owner], filled from the front without holes -- what travels to owner g is
 *           d_send_keys[g * capacity .. + d_cursors[g]) as it stands (d_cursors[0 .. n_shards) after the step; a multiple of
 *           slk_shard_chunk(n_shards): the last few entries are zero keys whose answers nobody reads).  A cursor beyond the capacity
 *           means the region was too small: slk_stream_synchronize reports SLK_E_CAPACITY, emit the batch again with larger regions.
 *           What the APPLY of the same batch needs stays on this rank, in the other arrays of slk_shard_lists.
 *   LOOKUP  the OWNER's side: taxon or NONE for the n keys this rank received (any batch, any ranks), as slk_lookup_device.
 *   APPLY   replays the batch's probe log -- no second scan --, takes each probe's taxon from d_taxa ([n_shards][capacity_per_owner]:
 *           the owners' answers at the positions the keys had) and classifies: the outputs of slk_classify_batch_device.
 * (between the jobs: all-to-all of keys, all-to-all of taxa back into the same positions -- the caller's, e.g. RCCL.)
 * Any of emit / lookup / apply may be NULL.  A step without an EMIT runs the other jobs as kernels of their own.
 * d_defer[R] of a batch (zeroed by its EMIT) is 1 after its APPLY for the fragments this path does not take (longer than 1000
 * bases, more than 12 distinct taxa): classify those with the staged calls above.  SLK_E_UNSUPPORTED if the index's splitter is
 * outside the fused kernel's range (window wider than 32 m-mers, or taxon ids beyond 22 bits that slk_index_finalize could not
 * renumber): use the staged calls. */
typedef struct {
  const uint8_t *d_bases;       /* the batch (EMIT only; the APPLY reads d_offsets / d_mate_offsets when hit lists are written) */
  const uint64_t *d_offsets;
  const uint8_t *d_mate_bases;  /* nullable */
  const uint64_t *d_mate_offsets;
  uint64_t R;
  uint64_t total_bases;         /* d_offsets[R] / d_mate_offsets[R]: the caller knows them (spares a copy back to the host) */
  uint64_t total_mate_bases;
  uint32_t n_shards;
  uint32_t reserved;
  uint64_t capacity_per_owner;  /* entries of each owner's region: a multiple of slk_shard_chunk(n_shards), below 2^32 */
  int64_t *d_send_keys;         /* [n_shards][capacity_per_owner] */
  uint32_t *d_send_meta;        /* [n_shards][capacity_per_owner]: the span behind every key */
  uint64_t *d_cursors;          /* [n_shards + 3] (zeroed by the EMIT): [g] = entries to send to owner g; [n_shards + 2] = after the
                                   APPLY, the number of fragments flagged in d_defer */
  uint32_t *d_batch_log;        /* [slk_shard_batch_rows(..)][n_shards][4]: per batch of 64 probes, where each owner's keys went */
  uint32_t *d_tile_rows;        /* [ceil(R / 64)][2] */
  int32_t *d_read_info;         /* [R][2]: k-mers and spans of a fragment */
  int32_t *d_defer;             /* [R] */
  int32_t *d_span_meta;         /* hit lists (all three or none; span slots as for slk_scan_device): the EMIT writes the flagged spans, */
  int32_t *d_span_taxon;        /* the APPLY the hits; gather them with d_span_count[r] entries per fragment */
  int32_t *d_span_count;
} slk_shard_lists;
typedef struct {
  const int64_t *d_keys;
  uint64_t n;
  int32_t *d_out_taxa;
} slk_shard_lookup;
typedef struct {
  const int32_t *d_taxa;        /* [n_shards][capacity_per_owner] of the batch's lists */
  int32_t min_hit_groups;
  int32_t C;
  const double *thresholds;     /* host, [C] */
  int32_t *d_out_taxon;         /* [C * R] threshold-major */
  uint8_t *d_out_classified;
  int32_t *d_out_num_distinct;  /* nullable */
  int32_t *d_out_total_kmers;   /* nullable */
  int32_t *d_out_num_hits;      /* nullable: spans per fragment (0 => no row) */
} slk_shard_results;
uint32_t slk_shard_chunk(uint32_t n_shards);
uint64_t slk_shard_batch_rows(uint64_t total_bases, uint64_t total_mate_bases, uint64_t R, int32_t paired);
int32_t slk_shard_step_device(slk_index *ix, slk_stream *st, const slk_shard_lists *emit, const slk_shard_lookup *lookup,
                              const slk_shard_lists *apply_lists, const slk_shard_results *apply);
/* classifyHits (Classifier.scala:124-147, 439-454) over span slots whose taxa have been filled in (d_span_taxon: record
 * taxon / NONE for SEQUENCE spans; AMBIGUOUS and MATE_PAIR_BORDER spans are recognised from d_span_meta).  d_scratch:
 * as many 8-byte entries as span slots. */
int32_t slk_classify_hits_device(slk_index *ix, slk_stream *st, const uint64_t *d_offsets,
                                 const uint64_t *d_mate_offsets, uint64_t R, const int32_t *d_span_meta,
                                 const int32_t *d_span_taxon, const int32_t *d_span_count, uint64_t *d_scratch,
                                 int32_t min_hit_groups, const double *thresholds, int32_t C, int32_t *d_out_taxon,
                                 uint8_t *d_out_classified, int32_t *d_out_num_distinct, int32_t *d_out_total_kmers,
                                 int32_t *d_out_num_hits);

/* ---- table-sharded classification in ONE process (BASELINE.json configs[3]: a library whose table exceeds one GPU's HBM).
 * The host counterpart of the exchange the reference's join implies (S/slacken/Classifier.scala:84-95: the span rows are shuffled to
 * the records by minimizer, the hits shuffled back and regrouped by title).  n indices -- member g created on its device with
 * slk_index_set_shard(g, n), fed the whole record stream, finalized, all with the same splitter and taxonomy -- form a set; one
 * slk_shardset_classify call is one ROUND: member g classifies batches[g] (R may be 0: the member still answers the others' keys).
 * Every member scans its own fragments; 8-byte minimizers travel to their owners, 4-byte taxa travel back, nothing else moves.
 * The exchange is RCCL's (ncclSend / ncclRecv grouped over the members' streams; librccl is loaded at run time) when every member
 * has a device of its own, device-to-device copies otherwise (SLK_EXCHANGE_AUTO chooses) -- several members on ONE device is
 * how a one-GPU box tests this path.  A batch's arguments mean what slk_classify_batch's do (host pointers; hit lists optional),
 * and so do the results: bit-identical to the replicated mode.  One thread per set at a time; several sets may share members. */
typedef struct slk_shardset slk_shardset;
#define SLK_EXCHANGE_AUTO 0
#define SLK_EXCHANGE_RCCL 1
#define SLK_EXCHANGE_COPY 2
typedef struct {
  const uint8_t *bases;
  const uint64_t *offsets;
  const uint8_t *mate_bases;    /* nullable (single-end) */
  const uint64_t *mate_offsets; /* nullable */
  uint64_t R;
  int32_t *out_taxon;           /* [C*R] threshold-major */
  uint8_t *out_classified;      /* [C*R] */
  int32_t *out_num_distinct;    /* [R] nullable */
  int32_t *out_total_kmers;     /* [R] nullable */
  uint64_t *out_hit_offsets;    /* [R+1] nullable */
  slk_hit *out_hits;            /* nullable */
  uint64_t hits_capacity;
} slk_shard_batch;
int32_t slk_shardset_create(slk_index *const *members, int32_t n_members, int32_t exchange, slk_shardset **out);
int32_t slk_shardset_classify(slk_shardset *set, slk_shard_batch *batches /* [n_members] */, int32_t min_hit_groups,
                              const double *thresholds, int32_t C);
/* n_rounds rounds in one call, batches[round * n_members + member], PIPELINED: per step every member launches one kernel that scans
 * round t, answers the keys it received for round t - 2 and classifies round t - 4, while the keys of round t - 1 and the taxa of
 * round t - 3 travel on the members' exchange streams; the host's only wait per step is for the split sizes of the round emitted a
 * step earlier.  Results as n_rounds calls of slk_shardset_classify.  device_resident != 0: every pointer of the batches is a DEVICE
 * pointer on its member's GPU (reads and results stay in HBM; no hit lists: out_hit_offsets / out_hits must be NULL). */
int32_t slk_shardset_classify_rounds(slk_shardset *set, slk_shard_batch *batches /* [n_rounds][n_members] */, int32_t n_rounds,
                                     int32_t device_resident, int32_t min_hit_groups, const double *thresholds, int32_t C);
int32_t slk_shardset_exchange_mode(const slk_shardset *set); /* SLK_EXCHANGE_RCCL or SLK_EXCHANGE_COPY: what AUTO chose */
/* The ordered pairs (a, b), a != b, of members whose copies are staged through pinned host memory: b's device cannot reach the memory
 * of a's (hipDeviceCanAccessPeer), or SLK_SHARDSET_NO_PEER=1 was set when the set was created.  0 with SLK_EXCHANGE_RCCL. */
int32_t slk_shardset_staged_pairs(const slk_shardset *set);
void slk_shardset_destroy(slk_shardset *set);

/* Per-stage device timing of the last slk_classify_batch_device call on st, in milliseconds (HIP events on the
 * stream the kernels ran on): [0]=scan, [1]=probe, [2]=classify.  Synchronises st. */
int32_t slk_stream_last_stage_ms(slk_stream *st, float out_ms[3]);
/* How many fragments of the last classify call on st the lane-per-fragment kernel handed to the wave-per-fragment kernel
 * (longer than 1000 bases, or more than 12 distinct taxa); 0 if that call did not take the lane kernel.  Synchronises st. */
int32_t slk_stream_last_deferred(slk_stream *st, uint64_t *out_count);
/* Which kernels the last classify call on st launched, one SLK_ROUTE_* bit each, as the host issued them (a pass that found its list
 * empty counts: the bit says the launch, not the work).  The lane path is LANE or ROUTING first, then LONG, SEGMENT, PIECES as the
 * batch's plan has them, then WAVE for what they hand on; WAVE alone is the wave-per-fragment kernel as the batch's only pass (taxon
 * ids over 22 bits without the dense renumbering, a taxonomy set after finalize, SLK_FORCE_WAVE=1); STAGED alone the three staged
 * kernels (windows over 32 m-mers, several id columns, SLK_FORCE_V1=1).  RERUN is added when a taxon map was found overflowed and the
 * batch was classified again by the staged kernels: that happens in slk_stream_synchronize or at the end of a host entry, so after
 * slk_classify_batch_device the bit can appear only once the caller has synchronised.  Both switches are read once per classify call.
 * Of a host call cut into sub-batches: the last sub-batch's.  0 before the first call.  Host bookkeeping: nothing is synchronised. */
enum {
  SLK_ROUTE_LANE = 1,      /* lane per fragment, the first pass over the whole batch */
  SLK_ROUTE_ROUTING = 2,   /* the routing kernel that stands for it in batches of long fragments */
  SLK_ROUTE_LONG = 4,      /* the lane kernel's long variant (1001 .. 4999 bases) */
  SLK_ROUTE_SEGMENT = 8,   /* lane per segment */
  SLK_ROUTE_PIECES = 16,   /* the piece route */
  SLK_ROUTE_WAVE = 32,     /* wave per fragment */
  SLK_ROUTE_STAGED = 64,   /* scan, probe, classify as three kernels */
  SLK_ROUTE_RERUN = 128    /* the staged kernels again, unbounded taxon maps, after an overflow */
};
int32_t slk_stream_last_route(slk_stream *st, uint32_t *mask);

/* ---- Contig-length fragments: one fragment split over many waves.  A fragment otherwise runs on ONE wave, at
 * about 15 Mbp/s, with a taxon map of 128 entries; a batch of a few hundred assembled contigs leaves most of the part idle, and a contig
 * that names more than 128 taxa sends its whole batch through the staged kernels again.  On the piece route an unpaired fragment of at
 * least min_len bases is cut into pieces of 65 536 k-mer windows, every piece is scanned and probed by a wave of its own, and the
 * pieces' counts are merged in HBM, in a taxon map that cannot overflow, before the fragment is resolved -- with the results of the
 * other routes, bit for bit.  Scope: unpaired fragments, the default window of five m-mers, calls that want no hit lists (or
 * slk_stream_set_split_hits); everything else keeps its route.  A fragment of 2^31 bases or more on this route fails the call (SLK_E_INVALID, at the next synchronisation).
 *   slk_stream_set_split_long  min_len = -1: the engine's own choice -- fragments of at least 300 000 bases (where the route measured
 *                              faster), in batches whose fragments average over 1000 bases and whose map scratch
 *                              stays under 2 GiB and under 8 bytes per base of the batch (it grows with the cells' taxon bits:
 *                              with 18-bit ids 300 kbp contigs stay unsplit, 4 Mbp ones are split); batches of reads see nothing
 *                              of the route --, 0: off, > 0: fragments of at
 *                              least that many bases, whatever scratch that takes (with many taxon bits and fragments of a few
 *                              hundred kbp that measured SLOWER than not splitting: DESIGN.md 21); holds for every later classify call on st, through
 *                              whichever entry: slk_classify_batch[_packed], slk_classify_batch_device, slk_classify_text and the
 *                              batches of a slk_pipe all reach the same dispatch.  SLK_E_INVALID below -1.
 *   slk_stream_last_split      of the last classify call on st: the fragments that took the piece route, the pieces they made, and
 *                              how often a wave emptied a full 128-entry map into its fragment's map before its piece ended; zeros
 *                              if the route did not run.  Synchronises st.
 *   slk_stream_set_split_hits  on != 0: a call that wants hit lists takes the route as well -- under the conditions a call without
 *                              them takes it after slk_stream_set_split_long(st, min_len) with min_len > 0, and only then: with the
 *                              engine's own choice (-1) such calls keep the other routes whatever this switch says.  Off by
 *                              default.  The pieces' waves leave their entries where the segment kernel's lanes do, a plan per
 *                              piece is made with the borders, and one more kernel moves the entries to their places:
 *                              hit_offsets and hits are those of the other routes, entry for entry, merged
 *                              (slk_stream_set_merged_hits) or not.  272 bytes of scratch per piece on top of the route's.
 * Environment, read per call: SLK_PIECE_MIN_LEN overrides the setter, SLK_PIECE_HITS=0|1 overrides slk_stream_set_split_hits;
 * SLK_PIECE_WINDOWS sets the piece size in windows (rounded up to
 * a multiple of 64, at least 4 096).  The entries that take host arrays (slk_classify_batch[_packed], slk_classify_text) size the
 * scratch from the fragments' lengths and run nothing of the route for a batch without a fragment of min_len bases.  The device
 * entries and slk_pipe know total_bases alone: a batch of at least min_len bases in all gets one 64-byte memset, four launches and
 * map scratch for the worst batch of its size -- 32 bytes per base of the batch or, where that is less, 32 bytes per taxon id the
 * cells can name (2^taxon_bits) for each fragment of min_len bases the batch could hold; SLK_DEBUG_SPLIT=1 prints
 * slk_stream_last_split's numbers to stderr after every call that ran the route.
 * A slk_pipe's streams are the pipe's own: its batches follow the engine's choice, or SLK_PIECE_MIN_LEN and SLK_PIECE_HITS. */
int32_t slk_stream_set_split_long(slk_stream *st, int64_t min_len);
int32_t slk_stream_set_split_hits(slk_stream *st, int32_t on);
int32_t slk_stream_last_split(slk_stream *st, uint64_t *fragments, uint64_t *pieces, uint64_t *spills);
/* What the route holds on st: the waves of the piece kernel's fixed grid (more pieces than that are drawn from a counter), and the
 * bytes of device scratch the route has allocated on st so far (0 until a call ran it; it grows to the largest call's need). */
int32_t slk_stream_split_info(slk_stream *st, uint64_t *grid_waves, uint64_t *scratch_bytes);

/* ---- Bracken weights: replaces BrackenWeights.buildWeights (S/slacken/BrackenWeights.scala:294-352) -- every read of length
 * read_len at every position of every record (readClassifications :251-268) classified against the index (classify :276-285:
 * resolveTree with confidence 0 and minHitGroups 2) and counted by (dest, source) (groupBy, :350).
 *   slk_bracken_create   read_len >= k (else SLK_E_INVALID; the reference leaves it undefined); max_fragment: the pieces records
 *                        are cut into (splitToMaxLength, :152-164), 0 = FRAGMENT_MAX = 1 MiB (:303); one id column only
 *                        (SLK_E_UNSUPPORTED otherwise, as the staged device entries)
 *   slk_bracken_add      R whole records (any length, any host memory; bases WITHOUT whitespace, as after regexp_replace :311)
 *                        with the taxon each came from (TaxonFragment.taxon).  Synchronous on st.  The counts do not depend on how
 *                        the records are split into calls or on their order.  A call that fails after its arguments were
 *                        accepted (SLK_E_CAPACITY: more (source, dest) pairs than the map holds, SLK_BRACKEN_MAP_LOG2; SLK_E_HIP)
 *                        has counted an unknown part of its records: the handle is spent.  Every later slk_bracken_add and
 *                        slk_bracken_result on it returns SLK_E_STATE; slk_bracken_destroy is what remains.  A call refused
 *                        with SLK_E_INVALID counted nothing and leaves the handle usable.
 *   slk_bracken_result   the triples so far, dest ascending then source ascending; *n = their number; cap 0 queries only
 *                        that, 0 < cap < *n gives SLK_E_CAPACITY
 * The ordinal the reference gives a segment's trailing hit lacks the segment's position (:230); this engine reproduces what
 * that does to the reads near a piece start. */
typedef struct slk_bracken slk_bracken;
int32_t slk_bracken_create(slk_index *ix, int32_t read_len, uint64_t max_fragment, slk_bracken **out);
int32_t slk_bracken_add(slk_bracken *b, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *source_taxa,
                        uint64_t R);
int32_t slk_bracken_result(slk_bracken *b, uint64_t *n, int32_t *dest, int32_t *source, uint64_t *count, uint64_t cap);
void slk_bracken_destroy(slk_bracken *b);

/* ---- Minimizer migration: replaces MinimizerMigration.taxaDistances (S/slacken/analysis/MinimizerMigration.scala:38-66), the
 * arithmetic of `compareIndex` (Slacken.scala:332-341) -- the records of a SUBJECT library joined on the minimizer with those of a
 * REFERENCE library (joinWith, :47) and counted by (t1 = the subject's taxon, t2 = the reference's).  The reference's table is the
 * index; the subject's records are streamed through it, no second table is built.
 *   slk_migration_create      reference: finalized (SLK_E_STATE otherwise), taxonomy not needed; one id column and not a shard of
 *                             a table-sharded library (slk_index_set_shard), SLK_E_UNSUPPORTED otherwise.  depths[T] (copied):
 *                             Taxonomy.depth (Taxonomy.scala:222-228) of the REFERENCE's taxonomy (bcTax, :42) for every id -- the
 *                             rank depth of the nearest ranked ancestor-or-self, -1 for undefined ids; the caller computes it, the
 *                             engine knows parents, not ranks.  An id outside [0, T) has depth -1 (the reference would throw an
 *                             ArrayIndexOutOfBoundsException).  depths NULL with T 0: steps is written as 0, only the pairs mean
 *                             something.
 *   slk_migration_add         n records of the subject in host memory (left-aligned minimizer, taxon), any chunking, any order;
 *                             n = 0 is allowed.  Records with taxon NONE are skipped (as slk_index_append skips them); a record
 *                             whose minimizer the reference lacks leaves the join (:47) and is counted in `unmatched`, the others
 *                             add 1 to their (t1, t2).  Both taxa are the caller's ids, also when slk_index_finalize renumbered
 *                             the reference's; t1 is never looked at (any int32 but 0 is counted).  Synchronous on st, also on
 *                             failure.
 *   slk_migration_add_device  the same with pointers on the reference's GPU, asynchronous on st; a failure of the queued work
 *                             shows at the next call on the handle.
 *   slk_migration_result      synchronises the device; the triples so far sorted by t1 then t2, steps per distinct pair (:51-64):
 *                             -100 when depth(t1) == -1, else -200 when depth(t2) == -1, else depth(t1) - depth(t2).
 *                             *n_triples = their number; cap 0 queries only that, 0 < cap < *n_triples gives SLK_E_CAPACITY.
 *                             matched / unmatched (nullable): records counted / records that left the join (an addition: the
 *                             reference does not report them).  May be called repeatedly and between adds.
 * The pair map starts at 2^SLK_MIGRATION_MAP_LOG2 slots (default 20, at least 10) and doubles between calls (and between the 4 M
 * record pieces of a host call) while it is more than half full, so only a call (piece) that by itself brings more new pairs than
 * the map has free slots can fill it: that call returns SLK_E_CAPACITY.  After SLK_E_CAPACITY or SLK_E_HIP the handle has counted an
 * unknown part of its records and is spent: slk_migration_add* and slk_migration_result return SLK_E_STATE, slk_migration_destroy
 * is what remains.  A call refused with SLK_E_INVALID counted nothing and leaves the handle usable. */
typedef struct slk_migration slk_migration;
int32_t slk_migration_create(slk_index *reference, const int32_t *depths, int32_t T, slk_migration **out);
int32_t slk_migration_add(slk_migration *m, slk_stream *st, const int64_t *keys, const int32_t *taxa, uint64_t n);
int32_t slk_migration_add_device(slk_migration *m, slk_stream *st, const int64_t *d_keys, const int32_t *d_taxa, uint64_t n);
int32_t slk_migration_result(slk_migration *m, uint64_t *n_triples, int32_t *t1, int32_t *t2, int32_t *steps, uint64_t *count,
                             uint64_t cap, uint64_t *matched, uint64_t *unmatched);
void slk_migration_destroy(slk_migration *m);

/* ---- Genome coverage: replaces the arithmetic of IndexStatistics.showTaxonFullCoverageStats (S/slacken/IndexStatistics.scala:86-111;
 * its consumer is Dynamic.reportDynamicIndexSupport, S/slacken/Dynamic.scala:230-241) and the k-mers per source taxon that
 * IndexStatistics.totalKmerCountReport needs (:38-52).  Every labelled sequence is scanned, every super-mer's minimizer
 * (SplitterMinimizers.find, S/slacken/Minimizers.scala:43-76: one (minimizer, source taxon) row per super-mer, with repetitions)
 * is looked up in the index's table; the rows are grouped by (minimizer, source) into countAll and countDistinct = 1 (:91),
 * inner-joined with the records (:99-100: a minimizer the index lacks leaves the join) and grouped by (source, depth of the record's
 * LCA taxon) into sumAll and sumDistinct (:101-102).
 *   slk_coverage_create   the index: finalized (SLK_E_STATE otherwise), one id column and not a shard of a table-sharded library
 *                         (slk_index_set_shard), a window of at most 28 m-mers as for slk_index_add_sequences (SLK_E_UNSUPPORTED
 *                         otherwise).  depths[T] (copied): Taxonomy.depth (:94) for every id, with the meaning it has in
 *                         slk_migration_create; an id outside [0, T) has depth -1.  max_pairs: the most (minimizer, source) pairs
 *                         one group may hold (16 bytes per slot of a map kept at most half full); 0 = what fits half of the device
 *                         memory free at the call -- a choice, not a measured number.
 *   slk_coverage_add      R sequences exactly as slk_index_add_sequences takes them (no whitespace, split around anything that is
 *                         not ACGTU) with the taxon each came from (the `taxon` column of GenomeLibrary.joinSequencesAndLabels, :87).
 *                         source_taxa[i] is any int32 but NONE, need not be a node of the taxonomy, and is only carried; sequences
 *                         with source NONE are skipped.  Synchronous on st.
 *   slk_coverage_fold     closes a GROUP: the (minimizer, source) pairs counted so far go into the (source, depth) rows (:101-102)
 *                         and are forgotten, which frees the map.  The caller promises that no source taxon has sequences on
 *                         both sides of a fold: otherwise that taxon's `distinct` counts a minimizer once per group it occurs in.
 *                         `all` and the totals are sums and do not care.
 *   slk_coverage_result   folds what is pending, then the rows so far sorted by source then depth: all = sumAll, distinct =
 *                         sumDistinct (:102).  *n_rows = their number; cap 0 queries only that, 0 < cap < *n_rows gives
 *                         SLK_E_CAPACITY.  May be called repeatedly and between adds (it closes the group, as a fold does).
 *   slk_coverage_totals   one row per source taxon seen, ascending, also those without a k-mer: kmers = the sum over its super-mers
 *                         of length - (k - 1) (:45-46), supermers = their number, matched or not.  Same cap protocol.
 *   slk_coverage_budget   the handle's max_pairs (what 0 was resolved to)
 * Within one group the result does not depend on the order of the sequences or on how they are split over calls.
 * The pair map starts at 2^SLK_COVERAGE_MAP_LOG2 slots (default 20, at least 10) and doubles between kernel launches, never beyond
 * the budget; a launch covers no more k-mer windows than the map has free slots, so no launch can fill it.  More pairs in one group
 * than max_pairs, or more than 2^28 source taxa, is SLK_E_CAPACITY.  After SLK_E_CAPACITY or SLK_E_HIP the handle has counted an
 * unknown part and is spent: every call but slk_coverage_destroy returns SLK_E_STATE.  A call refused with SLK_E_INVALID counted
 * nothing and leaves the handle usable.  The index must outlive the adds and must not change (its table is the minimizers' names). */
typedef struct slk_coverage slk_coverage;
int32_t slk_coverage_create(slk_index *ix, const int32_t *depths, int32_t T, uint64_t max_pairs, slk_coverage **out);
int32_t slk_coverage_add(slk_coverage *c, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *source_taxa,
                         uint64_t R);
int32_t slk_coverage_fold(slk_coverage *c, slk_stream *st);
int32_t slk_coverage_result(slk_coverage *c, uint64_t *n_rows, int32_t *source, int32_t *depth, uint64_t *all, uint64_t *distinct,
                            uint64_t cap);
int32_t slk_coverage_totals(slk_coverage *c, uint64_t *n_sources, int32_t *source, uint64_t *kmers, uint64_t *supermers,
                            uint64_t cap);
uint64_t slk_coverage_budget(const slk_coverage *c);
void slk_coverage_destroy(slk_coverage *c);

/* ---- Sample support: replaces the arithmetic of Dynamic.minimizersInSubjects (S/slacken/Dynamic.scala:95-117: the counts behind
 * `classify2 -C` and `-D`) and of Dynamic.multiStatsPerTaxon (:152-180: totalKmerCount, distinctMinimizerCount and
 * totalMinimizerCount of the support reports, :210-228).  Every SEQUENCE super-mer of every read is looked up in the index's table;
 * a hit (a miss is NONE and never counts) whose taxon has depth >= min_depth (:103, :167-170) is grouped by taxon into
 *   kmers       the sum of its k-mer windows (sum(kmerCount), :174)
 *   minimizers  the number of such super-mers (count(*), :116, :176)
 *   distinct    the number of different minimizers among them (count_distinct, :112, :175).
 * A minimizer is one record, one cell of the table and one taxon, so `distinct` is the number of different cells hit: the handle
 * keeps one bit per table cell (cells / 8 bytes of device memory), set the first time the cell is hit, for its whole life.
 *   slk_support_create   the index: finalized (SLK_E_STATE otherwise), one id column, not a shard of a table-sharded library, a window
 *                        of at most 28 m-mers (SLK_E_UNSUPPORTED otherwise), as for slk_coverage_create.  depths[T] (copied) has the
 *                        meaning it has there; an id outside [0, T) has depth -1.  min_depth < 0 is SLK_E_INVALID.  want_distinct =
 *                        0: no bitmap is allocated and every row's `distinct` is 0.
 *   slk_support_add      R sequences exactly as slk_index_add_sequences takes them (no whitespace, split around anything that is not
 *                        ACGTU).  The mates of paired reads are sequences of their own: the mate-pair border and ambiguous spans
 *                        carry no true taxon and never count.  Synchronous on st.
 *   slk_support_result   the rows with kmers > 0 || minimizers > 0, ascending by taxon, in the caller's ids.  *n_taxa = their number;
 *                        cap 0 queries only that, 0 < cap < *n_taxa gives SLK_E_CAPACITY (the first cap rows are written).  May be
 *                        called repeatedly and between adds.
 *   slk_support_totals   sequences = those handed to slk_support_add; supermers = the SEQUENCE super-mers scanned; matched = those
 *                        the table holds; kept = those that passed min_depth (the sum of `minimizers`).  Any pointer may be null.
 * The result does not depend on the order of the sequences or on how they are split over calls; a super-mer that a long read's
 * 512-window chunks cut in two counts once as a minimizer, with all its k-mers.  After SLK_E_HIP the handle has counted an unknown
 * part and is spent: every call but slk_support_destroy returns SLK_E_STATE.  A call refused with SLK_E_INVALID counted nothing.
 * The index must outlive the handle and must not change: its cells name the minimizers, and the bitmap is sized at create. */
typedef struct slk_support slk_support;
int32_t slk_support_create(slk_index *ix, const int32_t *depths, int32_t T, int32_t min_depth, int32_t want_distinct, slk_support **out);
int32_t slk_support_add(slk_support *s, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, uint64_t R);
int32_t slk_support_result(slk_support *s, uint64_t *n_taxa, int32_t *taxa, uint64_t *kmers, uint64_t *minimizers, uint64_t *distinct,
                           uint64_t cap);
int32_t slk_support_totals(slk_support *s, uint64_t *sequences, uint64_t *supermers, uint64_t *matched, uint64_t *kept);
void slk_support_destroy(slk_support *s);

/* ---- low-complexity masking of genomes (mask.hip): replaces the `k2mask -r x` that the reference's library preparation runs over
 * every .fna before a library is built (scripts/k2/mask_low_complexity.sh, called from download_genomic_library.sh).  The function
 * is the symmetric DUST of Morgulis et al. 2006, pinned to the published definition in integers (equality with
 * k2mask's own output is unpinned):
 *   letters     A C G T U in either case are valid, U reads as T; every maximal run of valid letters inside one sequence is masked
 *               on its own -- a run never crosses an invalid letter or a sequence border.
 *   intervals   a run of n letters has the triplets t_0 .. t_{n-3} (6-bit values of three letters).  An interval [a, b] of
 *               l = b - a + 1 triplets, 2 <= l <= window - 2, has S = sum over the triplet values v of c_v (c_v - 1) / 2, c_v the
 *               occurrences of v in it.  It is good iff 10 * S > threshold * (l - 1), and perfect iff it is good and no sub-interval
 *               of l' >= 2 triplets scores strictly higher: S' * (l - 1) <= S * (l' - 1) for all of them.  No floating point.
 *   masked      letters a .. b + 2 of the run, for every perfect interval.  A masked letter becomes `replacement`, or its lower-case
 *               form when replacement == 0 (k2mask's default); every other byte stays as it was.
 *   cfg         NULL, or window 0 / threshold 0: window 64, threshold 20 (in tenths, as k2mask -T).  window outside 8..64 or
 *               threshold outside 1..255 is SLK_E_INVALID and nothing is touched.
 * The layout is the one slk_index_add_sequences takes: sequence i is bases[offsets[i] .. offsets[i+1]), no whitespace; offsets
 * non-decreasing from offsets[0] = 0.  The masked count is the number of letters CHANGED (a lower-case letter masked with replacement 0
 * stays as it is and is not counted).  The stream's index is only the stream's owner here: it need hold no record and no taxonomy.
 *   slk_mask_device     in place on the stream's device: d_bases, d_offsets (n_sequences + 1 entries) and d_masked (one uint64) are
 *                       device pointers.  The kernels run asynchronously on st; the call itself first waits for what st holds, because
 *                       it reads the number of letters from d_offsets[n_sequences] to size its scratch -- two bits per letter, the
 *                       stream's, no other allocation.
 *   slk_mask_sequences  from and to host memory, synchronous.  The letters are staged in batches of SLK_MASK_BATCH_BASES (environment;
 *                       default 2^28) with a halo of window - 1 letters on either side, so a sequence longer than a batch is cut and
 *                       the result does not depend on the batch size.
 *   slk_index_add_sequences_masked  slk_index_add_sequences of the letters masked first (`build --mask`): uploaded once to the
 *                       stream's staging, masked where they lie and scanned where they lie (slk_index_add_sequences_device).  The
 *                       caller's letters are not touched; st must be a stream of ix.  Synchronous.
 *   slk_mask_tile_bases the interval starts one workgroup takes at a time (tests place borders on its multiples). */
typedef struct {
  uint32_t window;      /* 0: 64 */
  uint32_t threshold;   /* 0: 20 */
  uint8_t replacement;  /* 0: lower-case */
} slk_mask_config;
uint32_t slk_mask_tile_bases(void);
int32_t slk_mask_device(slk_stream *st, uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_sequences, const slk_mask_config *cfg,
                        uint64_t *d_masked);
int32_t slk_mask_sequences(slk_stream *st, uint8_t *bases, const uint64_t *offsets, uint64_t n_sequences, const slk_mask_config *cfg,
                           uint64_t *out_masked);
int32_t slk_index_add_sequences_masked(slk_index *ix, slk_stream *st, const uint8_t *bases, const uint64_t *offsets, const int32_t *taxa,
                                       uint64_t n_sequences, const slk_mask_config *cfg /* nullable */, uint64_t *out_masked);

/* ---- classifications joined with a truth mapping (compare.hip): the join of `compare` (S/slacken/Slacken.scala:343-366,
 * S/slacken/analysis/MappingComparison.scala), on the bytes of the read ids.  The rows of a reference mapping stay resident on the
 * device; the per-read output of `classify` streams through and every row whose id equals a kept reference id is counted under
 * (reference taxon, test taxon).  The taxonomy stays with the caller: taxa go in and come out RAW, as the texts have them, and the
 * caller applies primary(), isDefined and the rank arithmetic to the distinct pairs.
 * Text: lines end with \n, \r\n or a lone \r; empty lines are skipped; fields are split at TAB only, quotes mean nothing.  A line
 * with fewer columns than asked for, an empty id or taxon field, or a taxon that Java's Integer.parseInt refuses ("+7" is 7) or that
 * is negative is a bad line.  Chunks follow the parser's contract: n < 2^32; with final = 0 a line counts only when its terminator
 * lies inside the chunk (a \r on the last byte is undecided); *consumed is the start of the first undecided line, where the next
 * chunk starts; *consumed == 0 with final = 0 and n > 0 means the chunk must grow.  Results do not depend on how a text was cut.
 *   slk_compare_create         an empty handle on the device of st; the stream's index is only its owner, as for slk_mask_*.
 *                              SLK_COMPARE_HASH_BITS=N (environment, read here) truncates the ids' hash to N bits (tests).
 *   slk_compare_add_reference  replaces readCustomFormat (:265-274) and the build side of the join: id_col and taxon_col count from 1;
 *                              a row whose id holds "/2" is dropped, every "/1" is removed from the others' ids, and the row is
 *                              kept.  Host text, synchronous; _device takes device text, aligned to 16 bytes (synchronous too: the
 *                              table, the arena of id bytes and the count maps are sized from the chunk's lines and grow by themselves).
 *   slk_compare_begin_test     a new test location: clears the pairs, the "matched" flags and the test totals; the reference stays.
 *   slk_compare_add_test       replaces readKrakenFormat (:259-263) and the join (:157-159, :216-217): columns 2 and 3, the id as it is.
 *   slk_compare_pairs          the distinct (reference taxon, test taxon) of the joined rows of the current test with their rows,
 *                              ascending (what hitCategory :313-331 and the per-taxon sets :170-209 are computed from).  *n = their
 *                              number; cap 0 queries only that, 0 < cap < *n gives SLK_E_CAPACITY (the first cap rows are written),
 *                              as slk_support_result.
 *   slk_compare_reference_taxa the kept reference rows per raw taxon, ascending (the isDefined filter :130-131 and refTaxa :177-183).
 *   slk_compare_totals         reference rows read, dropped as "/2", kept; test rows read and joined (the current test).  Any
 *                              pointer may be null.
 *   slk_compare_error          where the text was wrong: the byte offset of the line in its whole text (all chunks counted) and
 *                              SLK_COMPARE_BAD_LINE, SLK_COMPARE_DUPLICATE_REFERENCE (an id twice among the kept reference rows; the
 *                              reference's join would multiply such rows) or SLK_COMPARE_DUPLICATE_TEST (an id twice among the
 *                              JOINED test rows; an unjoined id may repeat).  Of several the lowest offset; a duplicate reports one
 *                              of its occurrences.  The add that met it returned SLK_E_INVALID.
 * After SLK_E_HIP, and after an add that returned SLK_E_INVALID for a bad line or a duplicate, the handle holds an unknown part and is
 * spent: every call but slk_compare_error, slk_compare_totals and slk_compare_destroy returns SLK_E_STATE. */
#define SLK_COMPARE_NO_ERROR 0
#define SLK_COMPARE_BAD_LINE 1
#define SLK_COMPARE_DUPLICATE_REFERENCE 2
#define SLK_COMPARE_DUPLICATE_TEST 3
typedef struct slk_compare slk_compare;
int32_t slk_compare_create(slk_stream *st, slk_compare **out);
int32_t slk_compare_add_reference(slk_compare *h, slk_stream *st, const uint8_t *text, uint64_t n, int32_t id_col, int32_t taxon_col,
                                  int32_t final, uint64_t *consumed);
int32_t slk_compare_add_reference_device(slk_compare *h, slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t id_col,
                                         int32_t taxon_col, int32_t final, uint64_t *consumed);
int32_t slk_compare_begin_test(slk_compare *h);
int32_t slk_compare_add_test(slk_compare *h, slk_stream *st, const uint8_t *text, uint64_t n, int32_t final, uint64_t *consumed);
int32_t slk_compare_add_test_device(slk_compare *h, slk_stream *st, const uint8_t *d_text, uint64_t n, int32_t final, uint64_t *consumed);
int32_t slk_compare_pairs(slk_compare *h, uint64_t *n, int32_t *ref_taxon, int32_t *test_taxon, uint64_t *count, uint64_t cap);
int32_t slk_compare_reference_taxa(slk_compare *h, uint64_t *n, int32_t *taxa, uint64_t *count, uint64_t cap);
int32_t slk_compare_totals(slk_compare *h, uint64_t *reference_rows, uint64_t *dropped_second, uint64_t *kept_ids, uint64_t *test_rows,
                           uint64_t *joined_rows);
int32_t slk_compare_error(slk_compare *h, uint64_t *byte_offset, int32_t *kind);
void slk_compare_destroy(slk_compare *h);

#ifdef __cplusplus
}
#endif
#endif
