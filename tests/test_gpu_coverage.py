"""Genome coverage on the GPU (slk_coverage_*, slacken_amd/csrc/coverage.hip) through capi.Coverage against coverage_model.py, by
exact equality: chunk seams with and without an invalid base in the priming window, degenerate sequences, repeated and shared
sequences, an index that lacks some minimizers, more than one wave and more than one block of chunks, three splitters (one with
m = 32), renumbered index ids, source taxa outside the taxonomy, any batching and order, folds between groups, the pair map's growth
and its budget, refusals."""
import numpy as np
import pytest

import coverage_model as cm
import migration_model as mm
import synth
import taxgen
from test_host_classify2_gpu import write_ranked_taxonomy

pytestmark = pytest.mark.gpu
SEAM = 512                      # BUILD_CHUNK_WINDOWS: a sequence's chunk c starts with window 512 c
FAR = 5_000_000                 # source taxa from here on are beyond 2^22 and outside every taxonomy of these tests


def dna(n, rng):
    return synth.random_dna(n, rng).tobytes()


def build_world(orc, tmp, k, m, s, seed, dense=False):
    """sequences, the taxon each is indexed under (a node of the taxonomy), the source each is counted under (anything), and an
    index built from a subset of them"""
    import slacken_amd
    rng = np.random.default_rng(seed)
    p = orc.params(k=k, m=m, spaces=s)
    parents = taxgen.taxonomy(8 * 6, rng)
    tax = write_ranked_taxonomy(str(tmp / f"tax_{k}_{m}_{s}_{int(dense)}"), parents)
    ls = (len(parents) - 2) // taxgen.N_RANKS
    species = list(range(7 * ls + 2, 8 * ls + 2))
    # long sequences of 1300..2000 bases (3 or 4 chunks); one of them must have a super-mer across the first seam
    for attempt in range(50):
        long_seqs = [dna(int(rng.integers(1300, 2001)), rng) for _ in range(12)]
        straddling = [i for i, q in enumerate(long_seqs) if (lambda wm: wm[SEAM - 1] == wm[SEAM])(cm.window_minimizers(orc, p, q))]
        if straddling:
            break
    assert straddling, "no super-mer straddles a chunk seam"
    seqs, node, source = [], [], []

    def add(q, t, src=None):
        seqs.append(q)
        node.append(t)
        source.append(t if src is None else src)

    for i, q in enumerate(long_seqs):
        add(q, species[i % 4], None if i % 3 else FAR + i % 4)          # four genomes of three sequences; some sources far away
    # an N at seam - 1 (the priming window holds it, the chunk's first own window does not), at the seam (both do), and at
    # seam + k - 1 (only the chunk's first own window does)
    for j, at in enumerate((SEAM - 1, SEAM, SEAM + k - 1)):
        q = bytearray(long_seqs[straddling[0]])
        q[at] = ord("N")
        add(bytes(q), species[4], FAR + 10)
    add(long_seqs[0], species[0], FAR)                                   # the same sequence twice under one source
    add(long_seqs[1], species[5], species[5])                            # ... and under two sources, two species: the LCA is inner
    assert source[0] == FAR and source[1] == species[1] and node[1] != species[5]
    for j, q in enumerate((b"", dna(k - 1, rng), b"N" * 300)):           # no window at all: a totals row, no coverage row
        add(q, species[4], FAR + 20 + j)
    add(dna(k, rng), species[4], FAR + 30)                               # one window
    add(dna(700, rng).lower(), species[4], FAR + 31)                     # lower case, and a source of their own
    add(dna(900, rng), species[4], 0)                                    # NONE: skipped
    for j in range(300):                                                 # more than 256 chunks: two blocks, five waves
        add(dna(int(rng.integers(k, k + 25)), rng), species[j % 6], FAR + 100 + j % 7)
    unindexed = {2, 5, len(long_seqs) + 1} | set(range(len(seqs) - 300, len(seqs), 3))
    sel = [i for i in range(len(seqs)) if i not in unindexed and len(seqs[i]) >= k and source[i] != 0]
    remap = None
    if dense:                                                            # ids that need the dense renumbering
        parents, remap = taxgen.sparse_relabel(parents, (1 << 22) + 5000, rng)
        node = [remap[t] for t in node]
        source = [remap.get(t, t) for t in source]
    bases, offsets = cm.pack([seqs[i] for i in sel])
    keys, taxa = orc.build_records(p, parents, bases, offsets, [node[i] for i in sel])
    ix = slacken_amd.Index(k=k, m=m, spaces=s, expected_records=len(keys), max_taxon=len(parents) - 1, device=0)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    if dense:
        inverse = {new: old for old, new in remap.items()}
        depth_of = lambda t: mm.depth(tax, inverse[t]) if t in inverse else -1     # noqa: E731
        depths = np.full(len(parents), -1, np.int32)
        for new, old in inverse.items():
            depths[new] = mm.depth(tax, old)
    else:
        depth_of = lambda t: mm.depth(tax, t)                                         # noqa: E731
        depths = np.array([mm.depth(tax, t) for t in range(len(parents))], np.int32)
    oidx = orc.Index(1, keys, taxa)
    want = cm.coverage(orc, p, oidx, depth_of, seqs, source)
    return dict(p=p, k=k, ix=ix, st=ix.stream(), depths=depths, seqs=seqs, source=np.array(source, np.int32), oidx=oidx, depth_of=depth_of,
                want=want, parents=parents, keys=keys, taxa=taxa, n_long=len(long_seqs), orc=orc)


@pytest.fixture(scope="module", params=[(35, 31, 7, False), (21, 11, 0, False), (35, 32, 7, False), (35, 31, 7, True)],
                ids=["k35m31s7", "k21m11s0", "k35m32s7", "dense-ids"])
def world(request, orc, tmp_path_factory):
    k, m, s, dense = request.param
    return build_world(orc, tmp_path_factory.mktemp("cov"), k, m, s, seed=100 + m + int(dense), dense=dense)


@pytest.fixture(scope="module")
def base(orc, tmp_path_factory):
    return build_world(orc, tmp_path_factory.mktemp("covb"), 35, 31, 7, seed=7)


def got_of(cov):
    s, d, a, n = cov.result()
    ts, tk, tn = cov.totals()
    assert a.dtype == np.uint64 and s.dtype == np.int32 and tk.dtype == np.uint64
    return list(zip(s.tolist(), d.tolist(), a.tolist(), n.tolist())), list(zip(ts.tolist(), tk.tolist(), tn.tolist()))


def run(W, order=None, per_call=None, max_pairs=0, fold_after=()):
    """the sequences in `order`, per_call at a time (None: all at once), a fold after the calls listed"""
    import slacken_amd
    order = list(range(len(W["seqs"]))) if order is None else list(order)
    per_call = len(order) if per_call is None else per_call
    cov = slacken_amd.Coverage(W["ix"], W["depths"], max_pairs=max_pairs, stream=W["st"])
    for c, a in enumerate(range(0, len(order), per_call)):
        part = order[a:a + per_call]
        bases, offsets = cm.pack([W["seqs"][i] for i in part])
        cov.add(bases, offsets, W["source"][part])
        if c in fold_after:
            cov.fold()
    got = got_of(cov)
    cov.close()
    return got


def test_matches_the_model_and_is_not_vacuous(world):
    W = world
    rows, totals, misses = W["want"]
    assert run(W) == (rows, totals)
    k = W["k"]
    by_source = {}
    for s, d, a, n in rows:
        by_source.setdefault(s, []).append((d, a, n))
    assert misses > 0                                                     # the index lacks some minimizers: they left the join
    assert any(len(v) >= 2 for v in by_source.values())                   # a source with more than one depth
    assert any(a > n for _, _, a, n in rows)                              # repetitions: all != distinct
    zero = {s for s, km, _ in totals if km == 0}
    assert len(zero) == 3 and not zero & set(by_source)                   # length 0, k - 1, all N: totals rows only
    assert len(totals) == len({int(s) for s in W["source"]} - {0})
    assert sum(max(0, (len(q) - k) // SEAM + 1) if len(q) >= k else 0 for q in W["seqs"]) > 256 + 64
    assert max(int(s) for s in W["source"]) >= (1 << 22)


def test_the_same_sequence_twice(base):
    """under one source `all` doubles and `distinct` does not; under two species the rows lie at their LCA's depth"""
    import slacken_amd
    W, orc = base, base["orc"]
    q = W["seqs"][1]
    for sources, want_all in (([77], 1), ([77, 77], 2)):
        cov = slacken_amd.Coverage(W["ix"], W["depths"], stream=W["st"])
        bases, offsets = cm.pack([q] * len(sources))
        cov.add(bases, offsets, sources)
        rows, totals = got_of(cov)
        cov.close()
        want = cm.coverage(orc, W["p"], W["oidx"], W["depth_of"], [q] * len(sources), sources)
        assert (rows, totals) == want[:2] and rows
        if want_all == 1:
            once = rows
        else:
            assert [(s, d, 2 * a, n) for s, d, a, n in once] == rows
    # sequence 1 is indexed under two species: none of its minimizers is stored at species depth
    lca_depths = {d for _, d, _, _ in once}
    assert lca_depths and max(lca_depths) < 8


def test_batching_order_and_folds(base, monkeypatch):
    W = base
    want = W["want"][:2]
    rng = np.random.default_rng(3)
    shuffled = rng.permutation(len(W["seqs"])).tolist()
    assert run(W, order=shuffled, per_call=1) == want                    # one sequence per call, any order
    assert run(W, order=shuffled[::-1], per_call=37) == want
    # a fold between source-disjoint groups: the sequences sorted by source, a fold wherever the source changes
    by_source = sorted(range(len(W["seqs"])), key=lambda i: int(W["source"][i]))
    src = [int(W["source"][i]) for i in by_source]
    folds = {c for c in range(len(src) - 1) if src[c] != src[c + 1]}
    assert len(folds) >= 10
    assert run(W, order=by_source, per_call=1, fold_after=folds) == want
    # a small map that has to grow, and be rehashed, on the way
    monkeypatch.setenv("SLK_COVERAGE_MAP_LOG2", "10")
    assert sum(n for _, _, _, n in want[0]) > 2048
    assert run(W, order=shuffled, per_call=5) == want
    assert run(W) == want


def test_budget(base):
    import slacken_amd
    W, orc = base, base["orc"]
    pairs = sum(n for _, _, _, n in W["want"][0])
    assert run(W, max_pairs=pairs) == W["want"][:2]                       # exactly enough
    cov = slacken_amd.Coverage(W["ix"], W["depths"], max_pairs=100, stream=W["st"])
    assert cov.budget() == 100
    bases, offsets = cm.pack(W["seqs"])
    with pytest.raises(slacken_amd.SlackenError) as e:
        cov.add(bases, offsets, W["source"])
    assert e.value.code == slacken_amd.capi.E_CAPACITY
    for call in (cov.result, cov.totals, cov.fold, lambda: cov.add(bases[:0], offsets[:1], W["source"][:0])):
        with pytest.raises(slacken_amd.SlackenError) as e:
            call()
        assert e.value.code == slacken_amd.capi.E_STATE
    cov.close()
    # the index is none the worse for it
    reads = [np.frombuffer(W["seqs"][i][a:a + 150], np.uint8) for i in range(W["n_long"]) for a in (0, 400, 1100)]
    rb, ro = synth.pack(reads)
    want = orc.classify_batch(W["p"], W["oidx"], W["parents"], rb, ro)
    got = W["st"].classify_batch(rb, ro, with_hits=False)
    assert np.array_equal(got["taxon"], want["taxon"]) and want["classified"].any()
    assert np.array_equal(W["ix"].lookup(W["keys"][:500]), W["taxa"][:500])


def test_refusals(base):
    import ctypes as C
    import slacken_amd
    from slacken_amd import capi
    W = base
    L = capi.lib()
    parents = W["parents"]

    def code_of(fn):
        with pytest.raises(slacken_amd.SlackenError) as e:
            fn()
        return e.value.code

    raw = slacken_amd.Index(expected_records=1000, max_taxon=len(parents) - 1, device=0)
    raw.append(W["keys"][:100], W["taxa"][:100])
    assert code_of(lambda: slacken_amd.Coverage(raw, W["depths"])) == capi.E_STATE            # not finalized
    raw.close()
    wide = slacken_amd.Index(k=45, m=40, spaces=0, expected_records=1000, max_taxon=len(parents) - 1, device=0)
    wide.finalize()
    assert code_of(lambda: slacken_amd.Coverage(wide, W["depths"])) == capi.E_UNSUPPORTED     # two id columns
    wide.close()
    shard = slacken_amd.Index(expected_records=1000, max_taxon=len(parents) - 1, device=0)
    shard.set_shard(1, 2)
    shard.append(W["keys"][:100], W["taxa"][:100])
    shard.finalize()
    assert code_of(lambda: slacken_amd.Coverage(shard, W["depths"])) == capi.E_UNSUPPORTED    # a shard of a sharded library
    shard.close()
    h = C.c_void_p()
    assert L.slk_coverage_create(None, None, 0, 0, C.byref(h)) == capi.E_INVALID
    assert L.slk_coverage_create(W["ix"].h, None, 0, 0, None) == capi.E_INVALID
    assert L.slk_coverage_create(W["ix"].h, None, 5, 0, C.byref(h)) == capi.E_INVALID
    assert L.slk_coverage_add(None, W["st"].h, None, None, None, 0) == capi.E_INVALID
    assert L.slk_coverage_result(None, None, None, None, None, None, 0) == capi.E_INVALID
    cov = slacken_amd.Coverage(W["ix"], W["depths"], stream=W["st"])
    bases, offsets = cm.pack(W["seqs"][:3])
    n = C.c_uint64(0)
    assert L.slk_coverage_add(cov.h, None, bases.ctypes.data, offsets.ctypes.data, W["source"].ctypes.data, 3) == capi.E_INVALID
    assert L.slk_coverage_add(cov.h, W["st"].h, bases.ctypes.data, None, W["source"].ctypes.data, 3) == capi.E_INVALID
    assert L.slk_coverage_add(cov.h, W["st"].h, None, offsets.ctypes.data, W["source"].ctypes.data, 3) == capi.E_INVALID
    assert L.slk_coverage_result(cov.h, None, None, None, None, None, 0) == capi.E_INVALID
    assert L.slk_coverage_result(cov.h, C.byref(n), None, None, None, None, 4) == capi.E_INVALID
    assert L.slk_coverage_totals(cov.h, C.byref(n), None, None, None, 4) == capi.E_INVALID
    bad = offsets.copy()
    bad[1], bad[2] = bad[2], bad[1]
    assert code_of(lambda: cov.add(bases, bad, W["source"][:3])) == capi.E_INVALID              # counted nothing ...
    assert got_of(cov) == ([], [])
    cov.add(bases, offsets, W["source"][:3])                                                    # ... and the handle still works
    want = cm.coverage(W["orc"], W["p"], W["oidx"], W["depth_of"], W["seqs"][:3], W["source"][:3])
    assert got_of(cov) == want[:2] and want[0]
    # too small a capacity: the number is still given
    s1, d1, a1, n1 = (np.zeros(1, dt) for dt in (np.int32, np.int32, np.uint64, np.uint64))
    assert L.slk_coverage_result(cov.h, C.byref(n), s1.ctypes.data, d1.ctypes.data, a1.ctypes.data, n1.ctypes.data, 1) == capi.E_CAPACITY
    assert n.value == len(want[0]) > 1 and (int(s1[0]), int(d1[0]), int(a1[0]), int(n1[0])) == want[0][0]
    assert got_of(cov) == want[:2]                                                              # (not spent by that)
    cov.close()
    # no depths at all: every record has depth -1
    cov = slacken_amd.Coverage(W["ix"], None, stream=W["st"])
    cov.add(bases, offsets, W["source"][:3])
    rows, _ = got_of(cov)
    assert rows and {d for _, d, _, _ in rows} == {-1} and sum(a for _, _, a, _ in rows) == sum(a for _, _, a, _ in want[0])
    cov.close()


@pytest.mark.parametrize("distinct", [1, 2, 3, 64])
def test_a_small_pair_map_of_few_sources(orc, monkeypatch, distinct):
    """448 one-window sequences under 1, 2, 3 or 64 sources against an index that holds them all under one taxon, in a pair map of
    1024 slots (SLK_COVERAGE_MAP_LOG2=10; 448 pairs do not make it grow): every wave of the fold reads 64 slots with some 28 pairs
    under that many (source, depth) keys -- with three, lanes are left over after the two leader rounds.  The first 64 sequences are
    one wave of the scan whose lanes all start their super-mer at step k - 1: one push brings its queue exactly 64 entries."""
    import slacken_amd
    k = 35
    monkeypatch.setenv("SLK_COVERAGE_MAP_LOG2", "10")
    rng = np.random.default_rng(90 + distinct)
    p = orc.params()
    parents = np.array([0, 0, 1, 2], np.int32)
    seqs = [dna(k, rng) for _ in range(448)]
    source = np.array([100 + i % distinct for i in range(len(seqs))], np.int32)
    keys, taxa = orc.build_records(p, parents, *cm.pack(seqs), [3] * len(seqs))
    assert len(keys) == len(seqs)
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=3, device=0)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    depths = np.array([-1, 0, 1, 2], np.int32)
    want = cm.coverage(orc, p, orc.Index(1, keys, taxa), lambda t: int(depths[t]), seqs, source.tolist())
    got = run(dict(ix=ix, depths=depths, st=ix.stream(), seqs=seqs, source=source))
    assert got == want[:2] and len(got[0]) == distinct and sum(a for _, _, a, _ in got[0]) == len(seqs)
