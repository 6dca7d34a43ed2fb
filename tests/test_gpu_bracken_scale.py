"""Bracken weights on the device (slk_bracken_*, bracken.hip) where size and state matter: batches flushed in the middle of an add
and of a record, the window kernel's grid-stride loop, the (source, dest) map filled to its last slot and one pair beyond it, the
handle after that failure, extreme source ids, and windows of 566 k-mers over 41 taxa on the HBM map.

Every expected value comes from the model (tests/bracken_model.py) on a small input, and exact arithmetic on top of it: feeding a
set of records r times multiplies every count by r.  Each case asserts, on the model or on the input, that it reaches the branch it
is there for; the structural constants of bracken.hip are restated in tests/bracken_hard.py."""
import numpy as np
import pytest

import bracken_hard as bh
import bracken_model as bm
import synth
from bracken_cases import Case
from test_gpu_bracken import SPLITS, as_dict, device_index

pytestmark = pytest.mark.gpu

slacken_amd = pytest.importorskip("slacken_amd")

MIB = 1 << 20


def pack(records, sources, reps=1):
    """reps copies of the record list, one after the other, as the arrays of slk_bracken_add"""
    bases = np.frombuffer(b"".join(records), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
    if reps > 1:
        total = int(off[-1])
        off = np.concatenate([(np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(total) + off[None, :-1]).ravel(),
                              np.array([reps * total], np.uint64)])
        bases = np.tile(bases, reps)
    return bases, off, np.tile(np.array(sources, np.int32), reps)


def run(ix, read_len, calls, max_fragment=0, stream=None):
    bw = slacken_amd.BrackenWeights(ix, read_len, max_fragment, stream=stream)
    try:
        for call in calls:
            bw.add(*call)
        return bw.result()
    finally:
        bw.close()


def times(want, r):
    return {pair: r * n for pair, n in want.items()}


def diff(got, want):
    return sorted(set(got.items()) ^ set(want.items()))[:10]


# ---------------------------------------------------------------------------------------------------------------
# batch seams
# ---------------------------------------------------------------------------------------------------------------
def host_batches(lengths, read_len, max_fragment, batch_bytes):
    """slk_bracken_add's batching restated: the batch of every piece, as [(record, batch)]"""
    out, used, batch = [], 0, 0
    for r, n in enumerate(lengths):
        if n < read_len:
            continue
        for piece in bm.split_to_max_length(range(n), max_fragment, read_len):
            if used + len(piece) > batch_bytes and used:
                batch, used = batch + 1, 0
            used += len(piece)
            out.append((r, batch))
    return out


def test_batch_seams(orc, monkeypatch):
    sp = SPLITS[0]
    p = orc.params(**sp)
    L, F, reps = 100, 60_000, 4
    case = Case(orc, p, seed=99, n_genomes=8, genome_len=250_000, read_len=L)
    want = times(bm.fast(orc, p, case.index, case.parents, case.records, case.sources, L, F), reps)
    lengths = [len(r) for r in case.records] * reps
    assert sum(lengths) > 4 * MIB
    placed = host_batches(lengths, L, F, MIB)
    assert placed[-1][1] + 1 >= 8                                               # eight or so batches in the one add
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    whole = run(ix, L, [pack(case.records, case.sources, reps)], F)            # default batch: one batch
    monkeypatch.setenv("SLK_BRACKEN_BATCH_MB", "1")
    seamed = run(ix, L, [pack(case.records, case.sources, reps)], F)
    assert as_dict(seamed) == want, diff(as_dict(seamed), want)
    for a, b in zip(whole, seamed):
        assert np.array_equal(a, b)
    order = np.random.default_rng(5).permutation(len(lengths))
    recs, srcs = case.records * reps, case.sources * reps
    single = run(ix, L, [pack([recs[i]], [srcs[i]]) for i in order], F)        # one add per record, shuffled
    for a, b in zip(whole, single):
        assert np.array_equal(a, b)


def test_batch_seams_inside_records(orc, monkeypatch):
    """In test_batch_seams four records of 250 000 bases fill a 1 MiB batch to within 47 000 bases, less than the next record's
    first piece of 60 000: every seam there falls between two records.  Here the pieces are 7 000 bases of records of 20 000, and
    the seams cut records: pieces of one record in two batches, chunk and piece numbering restarted in the middle of a record."""
    sp = SPLITS[1]
    p = orc.params(**sp)
    L, F, reps = 100, 7000, 60
    case = Case(orc, p, seed=3, n_genomes=6, genome_len=20_000, read_len=L)
    want = times(bm.fast(orc, p, case.index, case.parents, case.records, case.sources, L, F), reps)
    lengths = [len(r) for r in case.records] * reps
    placed = host_batches(lengths, L, F, MIB)
    assert placed[-1][1] + 1 >= 5
    cut = sum(len({b for r, b in placed if r == rec}) > 1 for rec in set(r for r, _ in placed))
    assert cut >= 4                                                             # records with pieces on both sides of a seam
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    whole = run(ix, L, [pack(case.records, case.sources, reps)], F)
    monkeypatch.setenv("SLK_BRACKEN_BATCH_MB", "1")
    seamed = run(ix, L, [pack(case.records, case.sources, reps)], F)
    assert as_dict(seamed) == want, diff(as_dict(seamed), want)
    for a, b in zip(whole, seamed):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# linearity at scale: the window kernel's grid-stride loop
# ---------------------------------------------------------------------------------------------------------------
def short_records(case, rng, n, read_len):
    """n records of read_len .. read_len + 40 bases cut from the case's (mutated) genomes; every eighth with an N near its start"""
    recs, srcs = [], []
    while len(recs) < n:
        g = int(rng.integers(0, len(case.taxa)))
        ln = read_len + int(rng.integers(0, 41))
        a = int(rng.integers(0, len(case.records[g]) - ln))
        r = np.frombuffer(case.records[g][a:a + ln], np.uint8).copy()
        if len(recs) % 8 == 0:
            r[int(rng.integers(0, 40))] = ord("N")
        if r.tobytes() not in recs:   # distinct records
            recs.append(r.tobytes())
            srcs.append(case.sources[g])
    return recs, srcs


def test_linearity_beyond_the_grid(orc, monkeypatch):
    sp = SPLITS[0]
    p = orc.params(**sp)
    L, N, reps = 100, 1100, 600
    case = Case(orc, p, seed=61, n_genomes=6, genome_len=4000, read_len=L, extra_short=False)
    recs, srcs = short_records(case, np.random.default_rng(62), N, L)
    assert len(set(recs)) == N
    assert N * reps > bh.GRID_LANES + 64
    chunks = reps * sum(-(-(len(r) - L + 1) // bh.CHUNK) for r in recs)
    assert chunks > bh.GRID_LANES                                  # lanes of the window kernel take a second chunk
    base = bm.literal(orc, p, case.index, case.parents, recs, srcs, L)
    assert len({d for d, _ in base} - {0} - set(srcs)) > 0
    want = times(base, reps)
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    packed = pack(recs, srcs, reps)
    assert packed[0].size < 100_000_000
    one = run(ix, L, [packed])                                     # default batch (1 GiB): one batch of N * reps chunks
    assert as_dict(one) == want, diff(as_dict(one), want)
    monkeypatch.setenv("SLK_BRACKEN_BATCH_MB", "16")
    assert packed[0].size > 4 * 16 * MIB                           # several batches, none of them above the grid cap
    several = run(ix, L, [packed])
    for a, b in zip(one, several):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# the (source, dest) map: full to the last slot, and one pair too many
# ---------------------------------------------------------------------------------------------------------------
MAP_SLOTS = 1 << bh.MIN_MAP_LOG2


class FullMap:
    """Records of 260 bases, each with a source id of its own, that give exactly MAP_SLOTS (source, dest) pairs on the model; and
    one more record (random bases: destination NONE only) for the pair that does not fit."""

    def __init__(self, orc):
        self.sp = SPLITS[0]
        self.p = p = orc.params(**self.sp)
        self.L = 100
        self.case = case = Case(orc, p, seed=71, n_genomes=7, genome_len=6000, read_len=self.L, extra_short=False)
        rng = np.random.default_rng(72)
        self.records, self.sources, self.want = [], [], {}
        while len(self.want) < MAP_SLOTS:
            assert len(self.records) < 4000
            g = int(rng.integers(0, len(case.records)))
            a = int(rng.integers(0, len(case.records[g]) - 260))
            rec, src = case.records[g][a:a + 260], 1000 + len(self.records)
            pairs = bm.fast(orc, p, case.index, case.parents, [rec], [src], self.L)
            if len(self.want) + len(pairs) > MAP_SLOTS:
                continue
            self.records.append(rec)
            self.sources.append(src)
            self.want.update(pairs)
        self.extra = synth.random_dna(260, rng).tobytes()
        self.extra_source = 1000 + len(self.records)
        self.extra_want = bm.fast(orc, p, case.index, case.parents, [self.extra], [self.extra_source], self.L)

    def index(self):
        c = self.case
        return device_index(self.p, c.keys, c.rec_taxa, c.parents, self.sp["spaces"], self.sp["canonical"])


@pytest.fixture(scope="module")
def full_map(orc):
    return FullMap(orc)


def test_map_filled_to_the_last_slot(orc, full_map, monkeypatch):
    fm = full_map
    assert len(fm.want) == MAP_SLOTS and len({d for d, _ in fm.want}) > 4
    # the selection above used fast(): the expected triples once more from the line-by-line model
    assert bm.literal(orc, fm.p, fm.case.index, fm.case.parents, fm.records, fm.sources, fm.L) == fm.want
    monkeypatch.setenv("SLK_BRACKEN_MAP_LOG2", str(bh.MIN_MAP_LOG2))
    ix = fm.index()
    got = as_dict(run(ix, fm.L, [pack(fm.records, fm.sources)]))
    assert len(got) == MAP_SLOTS and got == fm.want, diff(got, fm.want)
    # every record 64 times in one call: many lanes insert the same new key at once
    recs = [r for r in fm.records for _ in range(64)]
    srcs = [s for s in fm.sources for _ in range(64)]
    got = as_dict(run(ix, fm.L, [pack(recs, srcs)]))
    assert len(got) == MAP_SLOTS and got == times(fm.want, 64), diff(got, times(fm.want, 64))


def test_one_pair_too_many(orc, full_map, monkeypatch):
    """A failed add spends the handle (include/slacken_amd.h, slk_bracken_add): result() and add() then give SLK_E_STATE.  Before the
    handle had that state, result() returned SLK_OK with the counts of whatever had reached the map."""
    fm = full_map
    assert len(fm.want) == MAP_SLOTS and len(fm.extra_want) == 1 and not set(fm.extra_want) & set(fm.want)
    want = {**fm.want, **fm.extra_want}
    assert len(want) == MAP_SLOTS + 1
    records, sources = fm.records + [fm.extra], fm.sources + [fm.extra_source]
    ix = fm.index()
    st = ix.stream()
    monkeypatch.setenv("SLK_BRACKEN_MAP_LOG2", str(bh.MIN_MAP_LOG2))
    bw = slacken_amd.BrackenWeights(ix, fm.L, stream=st)
    with pytest.raises(slacken_amd.SlackenError) as e:
        bw.add(*pack(records, sources))
    assert e.value.code == slacken_amd.capi.E_CAPACITY
    with pytest.raises(slacken_amd.SlackenError) as e:
        bw.result()
    assert e.value.code == slacken_amd.capi.E_STATE
    with pytest.raises(slacken_amd.SlackenError) as e:
        bw.add(*pack(fm.records[:1], fm.sources[:1]))
    assert e.value.code == slacken_amd.capi.E_STATE
    with pytest.raises(slacken_amd.SlackenError) as e:
        bw.result()
    assert e.value.code == slacken_amd.capi.E_STATE
    bw.close()
    assert bw.h is None
    monkeypatch.delenv("SLK_BRACKEN_MAP_LOG2")
    got = as_dict(run(ix, fm.L, [pack(records, sources)], stream=st))   # same index, same stream, default map
    assert got == want, diff(got, want)


# ---------------------------------------------------------------------------------------------------------------
# source ids
# ---------------------------------------------------------------------------------------------------------------
def test_source_ids(orc):
    sp = SPLITS[1]
    p = orc.params(**sp)
    L = 100
    case = Case(orc, p, seed=81, n_genomes=4, genome_len=2500, read_len=L)
    outside = len(case.parents) + 777                               # not a taxon of the taxonomy
    special = [0, 2**31 - 1, outside]
    sources = [special[i % 4] if i % 4 < 3 else s for i, s in enumerate(case.sources)]
    assert set(special) <= set(sources) and set(sources) & set(case.sources)
    want = bm.literal(orc, p, case.index, case.parents, case.records, sources, L)
    for s in special:
        assert sum(n for (_, src), n in want.items() if src == s) > 0
    assert (0, 0) in want                                           # the key of all zero bits
    ix = device_index(p, case.keys, case.rec_taxa, case.parents, sp["spaces"], sp["canonical"])
    got = as_dict(run(ix, L, [pack(case.records, sources)]))
    assert got == want, diff(got, want)
    # -1 is refused before anything is counted, and the handle stays usable
    bw = slacken_amd.BrackenWeights(ix, L)
    bad = list(sources)
    bad[len(bad) // 2] = -1
    with pytest.raises(slacken_amd.SlackenError) as e:
        bw.add(*pack(case.records, bad))
    assert e.value.code == slacken_amd.E_INVALID
    bw.add(*pack(case.records, sources))
    got = as_dict(bw.result())
    bw.close()
    assert got == want, diff(got, want)


# ---------------------------------------------------------------------------------------------------------------
# long windows on the HBM map
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [False, True])
def test_long_windows_of_many_taxa(orc, quirk):
    L = 600
    p = orc.params()
    mt = bh.ManyTaxa(orc, p, 3, L)
    assert L - p.k + 1 == 566
    records = mt.records(orc, quirk=quirk)
    assert len(records) == (4 if quirk else 3)
    most, initial, mid = 0, False, False
    for rec in records[:3]:
        n = [len(c) for c in bm.window_counts_pure(orc, p, mt.index, rec, L)]
        most = max(most, max(n))
        for c0 in range(0, len(n), bh.CHUNK):
            chunk = n[c0:c0 + bh.CHUNK]
            initial |= chunk[0] > bh.MAPCAP
            mid |= chunk[0] <= bh.MAPCAP and max(chunk) > bh.MAPCAP
    assert most == 41               # a window with every taxon the class has: its 40 leaves and B's
    assert initial and mid          # both hand-over points of the window lane are taken
    if quirk:
        _, _, _, _, qt, _ = bm.piece_arrays(orc, p, mt.index, records[3], L)
        assert qt != 0 and bh.deficits(orc, p, mt.index, records[3], L, qt).max() > 0
    ix = device_index(p, mt.keys, mt.rec_taxa, mt.parents, 7, True)
    src = [mt.tb] * len(records)
    for mf in (0, 1000):
        want = bm.literal(orc, p, mt.index, mt.parents, records, src, L, mf or 1024 * 1024)
        got = as_dict(run(ix, L, [pack(records, src)], mf))
        assert got == want, (mf, diff(got, want))
