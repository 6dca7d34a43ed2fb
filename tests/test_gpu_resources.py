"""The host side of the C ABI gives back what it takes: one cycle through the handles and the host entry points (create, load,
classify in every form, spans, lookup, export, the library builder, a table growth by each route, destroy) is run twice, and the
second run must leave the device with exactly the free memory the first one left.  The first run is the warm-up: contexts, torch,
code objects.  Every result of a cycle is compared with the CPU oracle, so a cycle that did nothing cannot pass."""
import gc
import os

import numpy as np
import pytest

import synth
import taxgen
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

THR = (0.0, 0.15)
KEYS = ("taxon", "classified", "num_distinct", "total_kmers", "num_hits")


def _env(name, value):
    class _Set:
        def __enter__(self):
            self.old = os.environ.get(name)
            os.environ[name] = value

        def __exit__(self, *exc):
            if self.old is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = self.old
    return _Set()


def _same(got, want, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k)


def _cycle(orc, w):
    import slacken_amd
    from slacken_amd import capi
    p, keys, taxa, parents = w["p"], w["keys"], w["taxa"], w["parents"]
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1)
    ix.append(keys, taxa)
    ix.set_taxonomy(parents)
    ix.finalize()
    st = ix.stream()
    # host classify calls: text and packed, single and paired, with and without hit lists
    for name, (mb, mo) in (("single", (None, None)), ("paired", w["mates"])):
        want = w["want_" + name]
        lists = {}
        for packed in (False, True):
            got = st.classify_batch(w["bases"], w["offsets"], mb, mo, thresholds=THR, with_hits=True, packed=packed)
            _same(got, want, (name, packed, "hits"))
            lists[packed] = got
            fast = st.classify_batch(w["bases"], w["offsets"], mb, mo, thresholds=THR, with_hits=False, with_num_hits=True, packed=packed)
            _same(fast, want, (name, packed, "no hits"))
        _same(lists[True], lists[False], (name, "packed lists"), ("hit_offsets", "hits"))
        ho = lists[False]["hit_offsets"].astype(np.int64)
        for i in range(0, w["R"], 97):   # the un-merged lists themselves, as check_classify compares them
            _, hits = orc.classify_read(p, w["oix"], parents, w["reads"][i].tobytes(),
                                        None if mb is None else w["mate_reads"][i].tobytes(), 2, THR[0])
            g = lists[False]["hits"][ho[i]:ho[i + 1]]
            assert [(int(t), int(c)) for t, c in zip(g["taxon"], g["count"])] == hits, (name, i)
        # the three-stream route: sub-batches of 256 fragments
        with _env("SLK_HOST_SUBBATCH", "256"):
            sub = st.classify_batch(w["bases"], w["offsets"], mb, mo, thresholds=THR, with_hits=True)
            _same(sub, want, (name, "sub-batches"))
            _same(sub, lists[False], (name, "sub-batches, lists"), ("hit_offsets", "hits"))
            # ... from and to memory of slk_host_alloc (the result rows come down beside the kernels)
            pb = capi.pinned_array(w["bases"].shape, np.uint8); pb[:] = w["bases"]
            po = capi.pinned_array(w["offsets"].shape, np.uint64); po[:] = w["offsets"]
            out = dict(taxon=capi.pinned_array((len(THR), w["R"]), np.int32), classified=capi.pinned_array((len(THR), w["R"]), np.uint8),
                       num_distinct=capi.pinned_array((w["R"],), np.int32), total_kmers=capi.pinned_array((w["R"],), np.int32))
            st.classify_batch(pb, po, mb, mo, thresholds=THR, with_hits=False, out=out)
            _same(out, want, (name, "pinned"), KEYS[:4])
            del pb, po, out
    # spans, lookups, export
    got_off, got = st.spans_batch(w["bases"][:w["span_bases"]], w["offsets"][:w["span_reads"] + 1])
    assert got_off.tolist() == w["want_span_off"]
    assert [(int(s["key"]), int(s["kmers"]), int(s["flag"]), int(s["distinct"])) for s in got] == w["want_spans"]
    assert np.array_equal(ix.lookup(keys), taxa)
    gk, gt = ix.export()
    assert np.array_equal(gk, w["sorted_keys"]) and np.array_equal(gt, w["sorted_taxa"])
    # the library builder on a second, small index
    ix2 = slacken_amd.Index(expected_records=1 << 12, max_taxon=len(parents) - 1)
    ix2.set_taxonomy(parents)
    ix2.add_sequences(w["g_bases"], w["g_offsets"], w["g_taxa"])
    ix2.finalize()
    bk, bt = ix2.export()
    assert np.array_equal(bk, w["want_built"][0]) and np.array_equal(bt, w["want_built"][1])
    ix2.close()
    # one table growth by each route (every record found again, the export equal to the input: _grow_with_records)
    for via_host in ("0", "1"):
        with _env("SLK_GROW_VIA_HOST", via_host):
            parity._grow_with_records(w["grow_keys"], w["grow_taxa"], w["grow_dup_at"], np.random.default_rng(808))
    st.close()
    ix.close()


def _world(orc):
    rng = np.random.default_rng(4242)
    parents = taxgen.taxonomy(8 * 32, rng)
    p = orc.params()   # k = 35, m = 31
    lib = synth.Library(orc, p, parents, n_genomes=4, genome_len=3000, pad_records=1 << 14)
    keys, taxa = lib.keys[:1 << 14], lib.taxa[:1 << 14]   # 2^14 records
    order = np.argsort(keys, kind="stable")
    oix = orc.Index(1, keys, taxa)
    R = 2000
    reads = synth.make_reads(lib, R, rng, n_single=0.1, n_run=0.05, short=0)
    mate_reads = synth.make_reads(lib, R, rng, short=0)
    bases, offsets = synth.pack(reads)
    mates = synth.pack(mate_reads)
    w = dict(p=p, parents=parents, keys=keys, taxa=taxa, sorted_keys=keys[order], sorted_taxa=taxa[order], oix=oix, R=R, reads=reads,
             mate_reads=mate_reads, bases=bases, offsets=offsets, mates=mates)
    w["want_single"] = orc.classify_batch(p, oix, parents, bases, offsets, thresholds=THR)
    w["want_paired"] = orc.classify_batch(p, oix, parents, bases, offsets, mates[0], mates[1], thresholds=THR)
    w["span_reads"] = 200
    w["span_bases"] = int(offsets[200])
    off, sp = parity.oracle_spans(orc, p, reads[:200])
    w["want_span_off"], w["want_spans"] = off, [(int(a), b, c, d) for a, b, c, d in sp]
    # the builder's input and what it must make of it
    w["g_bases"], w["g_offsets"] = synth.pack(lib.genomes[:2])
    w["g_taxa"] = np.asarray(lib.genome_taxa[:2], np.int32)
    w["want_built"] = orc.build_records(p, parents, w["g_bases"], w["g_offsets"], w["g_taxa"])
    # the library of test_a_library_that_outgrows_its_table_makes_it_grow
    grng = np.random.default_rng(808)
    gk = np.unique(grng.integers(-2**62, 2**62, 400_000, dtype=np.int64) & ~np.int64(0x33333333))
    w["grow_keys"], w["grow_taxa"] = gk, grng.integers(1, 2000, len(gk)).astype(np.int32)
    w["grow_dup_at"] = grng.choice(len(gk) // 2, 700, replace=False)
    return w


def test_a_second_cycle_through_the_host_side_takes_no_device_memory(orc):
    import torch
    w = _world(orc)
    free = []
    for _ in range(2):
        _cycle(orc, w)
        gc.collect()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print(f"free device memory after cycle 1: {free[0]}, after cycle 2: {free[1]}, lost: {free[0] - free[1]}")
    assert free[0] - free[1] <= 0, f"the second cycle kept {free[0] - free[1]} bytes of device memory"
