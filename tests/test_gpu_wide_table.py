"""The record table of the minimizers wider than 32 nt (wide.hip: 2..4 id columns; slk_index_append[_device], slk_index_add_sequences,
slk_index_lookup, slk_index_export) where it is least friendly: a table filled to its last slot and one record beyond, keys that
come twice (across calls and inside one), rows chosen to trip a key comparison, dozens of waves merging into the same slots, taxa
up to 2^31 - 1, taxa the host never sees, and the device entries.  The reference for the table is a dict from key row to taxon,
folded with the oracle's LCA where library construction merges; everything is compared bit for bit."""
import numpy as np
import pytest

import synth
import taxgen
from test_gpu_wide import build_world

pytestmark = pytest.mark.gpu

SETS = [(45, 40), (80, 65), (110, 100)]      # (k, m): W = 2, 3, 4
MASK64 = (1 << 64) - 1


def W_of(m):
    return (m + 31) // 32


def as_rows(rows, W):
    """python ints (unsigned words) -> (n, W) int64"""
    return np.array(rows, dtype=np.uint64).reshape(-1, W).view(np.int64)


def row_tuples(keys):
    return [tuple(int(x) for x in r) for r in np.asarray(keys).view(np.uint64)]


def adversarial(W, rng):
    """-> (stored rows, partner rows), unsigned words.  The partners are NOT stored: each differs from a stored row in the way a
    sloppy key comparison overlooks -- only the last word, only the first word, the same words in another order -- and the all-zero
    and all-ones rows are stored (a zero row is also what an idle lane carries)."""
    def word():
        return int(rng.integers(1, 1 << 62)) * 2 + 1
    stored, partners = [(0,) * W, (MASK64,) * W], []
    for _ in range(4):
        a = [word() for _ in range(W)]
        stored.append(tuple(a))
        partners.append(tuple(a[:-1] + [a[-1] ^ (1 << int(rng.integers(0, 64)))]))        # only the last word differs
        b = [word() for _ in range(W)]
        stored.append(tuple(b))
        partners.append(tuple([b[0] ^ (1 << int(rng.integers(0, 64)))] + b[1:]))         # only the first word differs
        c = [word() for _ in range(W)]
        assert len(set(c)) == W
        stored.append(tuple(c))
        partners.append(tuple(c[1:] + c[:1]))                                            # the same words, rotated
        if W > 2:
            partners.append(tuple(c[:-2] + [c[-1], c[-2]]))                              # ... the last two swapped
    assert len(set(stored) | set(partners)) == len(stored) + len(partners)
    return stored, partners


def unique_rows(n, W, rng, avoid=()):
    """n distinct random key rows (unsigned words as tuples), none of them in `avoid`"""
    seen, out = set(avoid), []
    while len(out) < n:
        for r in rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, W), dtype=np.uint64):
            t = tuple(int(x) for x in r)
            if t not in seen and len(out) < n:
                seen.add(t)
                out.append(t)
    return out


def sorted_model(model, W):
    """dict row -> taxon  ->  (keys uint64 (n, W) sorted as export() sorts them, taxa)"""
    rows = sorted(model)
    return np.array(rows, dtype=np.uint64).reshape(-1, W), np.array([model[r] for r in rows], np.int32)


def assert_export_is(ix, model, W):
    gk, gt = ix.export()
    wk, wt = sorted_model(model, W)
    assert len(set(row_tuples(gk))) == len(gk), "the export repeats a row"
    assert np.array_equal(gk.view(np.uint64), wk) and np.array_equal(gt, wt)


def capacity_of(ix, E):
    cap = ix.info().buckets * ix.info().bucket_cells
    assert cap & (cap - 1) == 0 and 2 * E <= cap < 4 * E, cap        # the power of two at or above 2 E
    return int(cap)


def full_table(slacken_amd, k, m, rng, E=1000):
    W = W_of(m)
    ix = slacken_amd.Index(k=k, m=m, spaces=0, expected_records=E)
    cap = capacity_of(ix, E)
    stored, partners = adversarial(W, rng)
    rows = stored + unique_rows(cap - len(stored), W, rng, avoid=stored + partners)
    order = rng.permutation(cap)
    rows = [rows[i] for i in order]
    taxa = rng.integers(1, 5000, cap).astype(np.int32)
    keys = as_rows(rows, W)
    for a, b in ((0, 1), (1, cap // 3), (cap // 3, cap)):           # three calls, the first of one record
        ix.append(keys[a:b], taxa[a:b])
    assert ix.info().records == cap and ix.info().duplicate_keys == 0 and ix.info().grown == 0
    return ix, cap, rows, keys, taxa, partners


@pytest.mark.parametrize("k,m", SETS)
def test_a_table_filled_to_its_last_slot(k, m):
    """expected_records = 1000: 2048 slots, all of them used.  Every key is found; absent keys -- a miss in a full table walks every
    slot and must end -- return 0, among them stored keys with one bit flipped in every word and the adversarial partners."""
    import slacken_amd
    rng = np.random.default_rng(1000 + m)
    ix, cap, rows, keys, taxa, partners = full_table(slacken_amd, k, m, rng)
    W = W_of(m)
    ix.finalize()
    assert ix.info().records == cap
    assert np.array_equal(ix.lookup(keys), taxa)
    flipped = [tuple(w ^ (1 << int(rng.integers(0, 64))) for w in rows[i]) for i in rng.choice(cap, 128, replace=False)]
    absent = partners + flipped
    absent += unique_rows(256 - len(absent), W, rng, avoid=rows + absent)
    assert len(absent) == 256 and not set(absent) & set(rows)
    assert np.array_equal(ix.lookup(as_rows(absent, W)), np.zeros(256, np.int32))
    assert_export_is(ix, dict(zip(rows, taxa.tolist())), W)


@pytest.mark.parametrize("k,m", SETS)
def test_one_record_more_than_the_table_holds(k, m):
    """The table does not grow: the record after the last slot is SLK_E_CAPACITY, and so is slk_index_finalize; the records that
    found a slot are all there, each with its own taxon."""
    import slacken_amd
    rng = np.random.default_rng(2000 + m)
    ix, cap, rows, keys, taxa, partners = full_table(slacken_amd, k, m, rng)
    W = W_of(m)
    extra = unique_rows(1, W, rng, avoid=rows)
    with pytest.raises(slacken_amd.SlackenError) as e:
        ix.append(as_rows(extra, W), np.array([7], np.int32))
    assert e.value.code == slacken_amd.capi.E_CAPACITY
    with pytest.raises(slacken_amd.SlackenError) as e:
        ix.finalize()
    assert e.value.code == slacken_amd.capi.E_CAPACITY
    gk, gt = ix.export()                                              # (legal before finalize)
    assert len(gt) == cap
    model = dict(zip(rows, taxa.tolist()))
    assert all(model.get(r) == int(t) for r, t in zip(row_tuples(gk), gt))
    assert_export_is(ix, model, W)


@pytest.mark.parametrize("k,m", SETS)
def test_keys_that_come_again_in_a_later_call(k, m):
    """slk_index_info.duplicate_keys: "appended records whose key was already present (contract violation; first kept)" -- 700
    repeats with another taxon, shuffled among 500 new records."""
    import slacken_amd
    rng = np.random.default_rng(3000 + m)
    W, N = W_of(m), 3000
    stored, partners = adversarial(W, rng)
    rows = stored + unique_rows(N + 500 - len(stored), W, rng, avoid=stored + partners)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    taxa = rng.integers(1, 5000, N + 500).astype(np.int32)
    model = dict(zip(rows, taxa.tolist()))
    ix = slacken_amd.Index(k=k, m=m, spaces=0, expected_records=N + 500)
    ix.append(as_rows(rows[:N], W), taxa[:N])
    assert ix.info().records == N and ix.info().duplicate_keys == 0
    again = [rows[i] for i in rng.choice(N, 700, replace=False)]
    second_rows = rows[N:] + again
    second_taxa = np.concatenate([taxa[N:], np.array([model[r] + 5000 for r in again], np.int32)])
    order = rng.permutation(len(second_rows))
    ix.append(as_rows([second_rows[i] for i in order], W), second_taxa[order])
    assert ix.info().records == N + 500 and ix.info().duplicate_keys == 700
    ix.finalize()
    assert ix.info().records == N + 500 and ix.info().duplicate_keys == 700
    assert np.array_equal(ix.lookup(as_rows(again, W)), np.array([model[r] for r in again], np.int32))      # the first taxon
    assert np.array_equal(ix.lookup(as_rows(rows, W)), taxa)
    assert np.array_equal(ix.lookup(as_rows(partners, W)), np.zeros(len(partners), np.int32))
    assert_export_is(ix, model, W)


@pytest.mark.parametrize("k,m", SETS)
def test_keys_that_come_twice_in_one_call(k, m):
    """300 of 1700 keys twice in one call, with two taxa: one record each, one of the two taxa (which is not specified, as on the
    one-column table), 300 duplicates counted.  Some of the twins are neighbours in the call -- lanes of one wave --, some far apart."""
    import slacken_amd
    rng = np.random.default_rng(4000 + m)
    W = W_of(m)
    stored, partners = adversarial(W, rng)
    rows = stored + unique_rows(1700 - len(stored), W, rng, avoid=stored + partners)
    rows = [rows[i] for i in rng.permutation(1700)]
    taxa = rng.integers(1, 5000, 1700).astype(np.int32)
    twins = rng.choice(1700, 300, replace=False)
    call_rows, call_taxa = list(rows), taxa.tolist()
    for n, i in enumerate(twins):                                     # a third right behind their twin, the others anywhere
        at = call_rows.index(rows[i]) + 1 if n % 3 == 0 else int(rng.integers(0, len(call_rows) + 1))
        call_rows.insert(at, rows[i])
        call_taxa.insert(at, int(taxa[i]) + 5000)
    assert len(call_rows) == 2000
    ix = slacken_amd.Index(k=k, m=m, spaces=0, expected_records=1700)
    ix.append(as_rows(call_rows, W), np.array(call_taxa, np.int32))
    assert ix.info().records == 1700 and ix.info().duplicate_keys == 300
    ix.finalize()
    got = ix.lookup(as_rows(rows, W))
    twin = np.zeros(1700, bool)
    twin[twins] = True
    assert np.array_equal(got[~twin], taxa[~twin])
    assert np.all((got[twin] == taxa[twin]) | (got[twin] == taxa[twin] + 5000))
    gk, gt = ix.export()
    assert len(gt) == 1700 and len(set(row_tuples(gk))) == 1700
    assert_export_is(ix, dict(zip(rows, got.tolist())), W)            # the export says what the lookups say
    assert np.array_equal(ix.lookup(as_rows(partners, W)), np.zeros(len(partners), np.int32))


def contention_world(orc, k, m, rng):
    """64 sequences, every one with a leaf of its own: 48 times the same 2 000-base genome, 16 times that genome with the same 300
    bases replaced -- every minimizer is offered by 16, 48 or 64 taxa at once.  -> (p, parents, seqs, leaves, records dict)"""
    p = orc.params(k=k, m=m, spaces=5, canonical=True)
    W = W_of(m)
    parents = taxgen.taxonomy(8 * 64, rng)
    taxa = np.array(taxgen.defined_taxa(parents))
    all_leaves = np.setdiff1d(taxa, parents[taxa])
    all_leaves = all_leaves[all_leaves != 1]
    leaves = rng.choice(all_leaves, 64, replace=False).astype(np.int32)
    top = {taxgen.path_to_root(parents, t)[-2] for t in leaves}       # the children of the root above the leaves
    assert len(top) >= 3
    genome = synth.random_dna(2000, rng)
    variant = genome.copy()
    variant[900:1200] = synth.random_dna(300, rng)
    seqs = [genome] * 48 + [variant] * 16
    order = rng.permutation(64)
    seqs = [seqs[i] for i in order]
    spans_of = {}
    for s in (genome, variant):
        spans_of[s.tobytes()] = [tuple(sp["key"][:W]) for sp in orc.spans(p, s.tobytes()) if sp["flag"] == 1]
    recs = {}
    for s, t in zip(seqs, leaves):
        for key in spans_of[s.tobytes()]:
            recs[key] = orc.lca(parents, recs.get(key, 0), int(t))
    merged = np.mean([t not in set(leaves.tolist()) for t in recs.values()])
    assert merged >= 0.9, merged                                      # the records are merges, not somebody's own taxon
    return p, parents, seqs, leaves, recs


@pytest.mark.parametrize("k,m", SETS)
def test_sixty_four_sequences_merge_into_the_same_slots(orc, k, m):
    """wide_build_insert_kernel's claim / publish / LCA-CAS protocol under contention: one wave per sequence, all of them after the
    same slots at once.  One call, and the sequences in another order over three calls: the same records as the dict folded with
    the oracle's LCA."""
    import slacken_amd
    rng = np.random.default_rng(5000 + m)
    p, parents, seqs, leaves, recs = contention_world(orc, k, m, rng)
    W = W_of(m)
    second = rng.permutation(64)
    for order, cuts in ((np.arange(64), (0, 64)), (second, (0, 5, 40, 64))):
        ix = slacken_amd.Index(k=k, m=m, spaces=5, canonical=True, expected_records=len(recs), max_taxon=len(parents) - 1)
        ix.set_taxonomy(parents)
        for a, b in zip(cuts[:-1], cuts[1:]):
            bases, offsets = synth.pack([seqs[i] for i in order[a:b]])
            ix.add_sequences(bases, offsets, leaves[order[a:b]])
        assert ix.info().records == len(recs)
        assert_export_is(ix, recs, W)
        ix.finalize()
        wk, wt = sorted_model(recs, W)
        assert np.array_equal(ix.lookup(wk.view(np.int64)), wt)


@pytest.mark.parametrize("k,m", SETS)
def test_append_and_add_sequences_mixed(orc, k, m):
    """slk_index_add_sequences "may be called any number of times, also mixed with slk_index_append of records whose keys do not
    occur in the sequences": the table holds the union, whichever comes first."""
    import slacken_amd
    rng = np.random.default_rng(6000 + m)
    p, W, parents, genomes, keys, tx = build_world(orc, k, m, 5, True, rng, n_genomes=3, genome_len=1500)
    seq_recs = dict(zip(row_tuples(keys), tx.tolist()))
    stored, partners = adversarial(W, rng)
    rows = stored + unique_rows(400, W, rng, avoid=stored + partners)
    assert not set(rows) & set(seq_recs)
    own = rng.integers(1, len(parents), len(rows)).astype(np.int32)
    model = dict(seq_recs)
    model.update(zip(rows, own.tolist()))
    g_taxa = genome_taxa(orc, p, W, parents, genomes, seq_recs)
    bases, offsets = synth.pack(genomes)
    for append_first in (True, False):
        ix = slacken_amd.Index(k=k, m=m, spaces=5, canonical=True, expected_records=len(model), max_taxon=len(parents) - 1)
        ix.set_taxonomy(parents)
        if append_first:
            ix.append(as_rows(rows, W), own)
        ix.add_sequences(bases, offsets, g_taxa)
        if not append_first:
            ix.append(as_rows(rows, W), own)
        assert ix.info().records == len(model) and ix.info().duplicate_keys == 0
        assert_export_is(ix, model, W)
        ix.finalize()
        assert np.array_equal(ix.lookup(as_rows(partners, W)), np.zeros(len(partners), np.int32))


def genome_taxa(orc, p, W, parents, genomes, recs):
    """The taxa build_world gave its genomes, read back from its records: a genome's taxon is the taxon of a minimizer that only
    this genome has (one outside the stretches it shares with its neighbours)."""
    owners = {}
    for g, genome in enumerate(genomes):
        for sp in orc.spans(p, genome.tobytes()):
            if sp["flag"] == 1:
                owners.setdefault(tuple(sp["key"][:W]), set()).add(g)
    out = []
    for g in range(len(genomes)):
        mine = {recs[key] for key, who in owners.items() if who == {g}}
        assert len(mine) == 1
        out.append(mine.pop())
    return np.array(out, np.int32)


@pytest.mark.parametrize("k,m", SETS)
def test_taxa_up_to_31_bits_and_none_below_zero(k, m):
    """The wide table keeps the taxon as a whole word (taxon_bits = 31): 1, 2^22 - 1, 2^22 and 2^31 - 1 come back from lookup and
    export.  A negative taxon from the host is SLK_E_INVALID and nothing of that call is stored."""
    import slacken_amd
    rng = np.random.default_rng(7000 + m)
    W = W_of(m)
    ids = np.array([1, (1 << 22) - 1, 1 << 22, (1 << 31) - 1], np.int32)
    rows = unique_rows(400, W, rng)
    taxa = ids[rng.integers(0, 4, 400)]
    taxa[:4] = ids
    ix = slacken_amd.Index(k=k, m=m, spaces=0, expected_records=500)
    assert ix.info().taxon_bits == 31
    ix.append(as_rows(rows, W), taxa)
    bad_rows = unique_rows(50, W, rng, avoid=rows)
    for bad in (-1, -2, -(1 << 31)):
        bad_taxa = np.full(50, 9, np.int32)
        bad_taxa[37] = bad
        with pytest.raises(slacken_amd.SlackenError) as e:
            ix.append(as_rows(bad_rows, W), bad_taxa)
        assert e.value.code == slacken_amd.capi.E_INVALID
    assert ix.info().records == 400
    ix.finalize()
    assert np.array_equal(ix.lookup(as_rows(rows, W)), taxa)
    assert np.array_equal(ix.lookup(as_rows(bad_rows, W)), np.zeros(50, np.int32))
    assert_export_is(ix, dict(zip(rows, taxa.tolist())), W)


@pytest.mark.parametrize("k,m", SETS)
def test_a_negative_taxon_from_the_device_is_refused(k, m):
    """slk_index_append_device takes taxa the host cannot check.  -1 is also the table's own marker of a slot whose key is still
    being written: it must never stay in a slot.  The kernel skips records with a negative taxon, the call is SLK_E_INVALID, the
    other records of the call are stored.  (No slk_index_add_sequences on this index, by intent: it is the call that would have
    to wait for such a slot.)"""
    import slacken_amd
    import torch
    rng = np.random.default_rng(8000 + m)
    W = W_of(m)
    rows = unique_rows(300, W, rng)
    taxa = rng.integers(1, 5000, 300).astype(np.int32)
    taxa[[70, 200]] = [-1, -(1 << 31)]
    d_k = torch.from_numpy(as_rows(rows, W).copy()).cuda()
    d_t = torch.from_numpy(taxa.copy()).cuda()
    ix = slacken_amd.Index(k=k, m=m, spaces=0, expected_records=300)
    with pytest.raises(slacken_amd.SlackenError) as e:
        ix.append_device(d_k.data_ptr(), d_t.data_ptr(), 300)
    assert e.value.code == slacken_amd.capi.E_INVALID
    assert ix.info().records == 298
    ix.append_device(d_k.data_ptr(), d_t.data_ptr(), 60)             # the index goes on: 60 records it has already
    assert ix.info().records == 298 and ix.info().duplicate_keys == 60
    ix.finalize()
    want = np.where(taxa < 0, 0, taxa).astype(np.int32)
    assert np.array_equal(ix.lookup(as_rows(rows, W)), want)
    gk, gt = ix.export()
    assert len(gt) == 298 and gt.min() > 0
    assert_export_is(ix, {r: int(t) for r, t in zip(rows, taxa) if t > 0}, W)


@pytest.mark.parametrize("k,m", SETS)
def test_the_device_entries_with_several_id_columns(orc, k, m):
    """slk_index_append_device on an (n, W) int64 tensor, slk_index_add_sequences_device on bases that lie on the GPU, and
    slk_classify_batch_device, single and paired: the same records and the same calls as the host entries and the oracle give."""
    import slacken_amd
    import torch
    rng = np.random.default_rng(9000 + m)
    p, W, parents, genomes, keys, tx = build_world(orc, k, m, 5, True, rng, n_genomes=4, genome_len=2500)
    recs = dict(zip(row_tuples(keys), tx.tolist()))
    g_taxa = genome_taxa(orc, p, W, parents, genomes, recs)

    def new_index():
        ix = slacken_amd.Index(k=k, m=m, spaces=5, canonical=True, expected_records=len(tx), max_taxon=len(parents) - 1)
        ix.set_taxonomy(parents)
        return ix
    host = new_index()
    host.append(keys, tx)
    hk, ht = host.export()
    assert np.array_equal(hk, keys[np.lexsort(keys.view(np.uint64).T[::-1])]) and len(ht) == len(tx)

    order = rng.permutation(len(tx))
    d_k = torch.from_numpy(keys[order].copy()).cuda()
    d_t = torch.from_numpy(tx[order].copy()).cuda()
    assert tuple(d_k.shape) == (len(tx), W) and d_k.is_contiguous()
    dev = new_index()
    half = len(tx) // 2
    dev.append_device(d_k.data_ptr(), d_t.data_ptr(), half)
    dev.append_device(d_k.data_ptr() + 8 * W * half, d_t.data_ptr() + 4 * half, len(tx) - half)
    assert dev.info().records == len(tx) and dev.info().duplicate_keys == 0
    dk, dt = dev.export()
    assert np.array_equal(dk, hk) and np.array_equal(dt, ht)

    bases, offsets = synth.pack(genomes)
    host_seq = new_index()
    host_seq.add_sequences(bases, offsets, g_taxa)
    sk, st_ = host_seq.export()
    assert np.array_equal(sk, hk) and np.array_equal(st_, ht)          # (the sequences give the records of build_world)
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, np.uint8)])).cuda()      # 16 spare bytes past the end
    dev_seq = new_index()
    dev_seq.add_sequences_device(d_b.data_ptr(), offsets, g_taxa)
    assert dev_seq.info().records == len(tx)
    qk, qt = dev_seq.export()
    assert np.array_equal(qk, hk) and np.array_equal(qt, ht)

    class L:
        pass
    L.genomes = genomes
    reads = synth.make_reads(L, 300, rng, length=2 * k, vary_length=True, n_single=0.1, n_run=0.05)
    mates = synth.make_reads(L, 300, rng, length=k + 40, vary_length=True, short=0.1)
    oix = orc.Index(W, keys, tx)
    dev.finalize()
    stream = dev.stream()
    rb, ro = synth.pack(reads)
    mb, mo = synth.pack(mates)
    R = len(reads)
    d_rb = torch.from_numpy(np.concatenate([rb, np.zeros(16, np.uint8)])).cuda()
    d_ro = torch.from_numpy(ro.astype(np.int64)).cuda()
    d_mb = torch.from_numpy(np.concatenate([mb, np.zeros(16, np.uint8)])).cuda()
    d_mo = torch.from_numpy(mo.astype(np.int64)).cuda()
    thr = (0.0, 0.3)
    for paired in (False, True):
        want = orc.classify_batch(p, oix, parents, rb, ro, mb if paired else None, mo if paired else None, min_hit_groups=2, thresholds=thr)
        o_t = torch.zeros(2 * R, dtype=torch.int32, device="cuda")
        o_c = torch.zeros(2 * R, dtype=torch.uint8, device="cuda")
        o_nd, o_tk, o_nh = (torch.zeros(R, dtype=torch.int32, device="cuda") for _ in range(3))
        stream.classify_batch_device(d_rb.data_ptr(), d_ro.data_ptr(), R, int(ro[-1]), o_t.data_ptr(), o_c.data_ptr(), o_nd.data_ptr(),
                                     o_tk.data_ptr(), o_nh.data_ptr(), None, d_mb.data_ptr() if paired else None,
                                     d_mo.data_ptr() if paired else None, int(mo[-1]) if paired else 0, min_hit_groups=2, thresholds=thr)
        stream.synchronize()
        assert np.array_equal(o_t.cpu().numpy().reshape(2, R), want["taxon"]), paired
        assert np.array_equal(o_c.cpu().numpy().reshape(2, R), want["classified"]), paired
        assert np.array_equal(o_nd.cpu().numpy(), want["num_distinct"]), paired
        assert np.array_equal(o_tk.cpu().numpy(), want["total_kmers"]), paired
        assert np.array_equal(o_nh.cpu().numpy(), want["num_hits"]), paired
        assert want["classified"][0].mean() > 0.3
