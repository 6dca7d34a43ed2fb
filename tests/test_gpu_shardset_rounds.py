"""slk_shardset_classify_rounds with SEVERAL members and SEVERAL rounds at once: the pipeline of csrc/shardset.hip as the first
multi-GPU run will meet it -- a step's kernel carrying EMIT(t), LOOKUP(t - 2) and APPLY(t - 4) of three different rounds, the rings
of six round slots and three key buffers turning over, members waiting for each other's exchange events, empty batches in every role,
hit lists that differ inside a step, fragments handed back in mid-pipeline, a send region that overflows in mid-pipeline
(SLK_SHARDSET_REGION_CAP), device-resident rounds, an error in mid-pipeline, and all of it again over the host-staged leg of the
exchange (SLK_SHARDSET_NO_PEER: every copy between two members through the sender's pinned bounce buffer).

Every expected value is exact: the oracle's classify_batch for every output of every batch, the replicated stream's rows and WHOLE
hit arrays, the oracle's classify_read for the un-merged list of every 7th read, and the same batches through one round at a time.
A batch, its oracle results and its replicated results are computed once per module and shared (the `bank` of a world)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import shard_step_model as M
import synth
import taxgen
from test_gpu_shardset import NO_PEER, make_members, same, same_hits, set_no_peer, staged_as_asked

pytestmark = pytest.mark.gpu

THR = (0.0, 0.2)
ROWS = ("taxon", "classified", "num_distinct", "total_kmers")
PLACEMENT = pytest.mark.parametrize("placement", ["one-device", "device-each"])


class Batch:
    """a batch, what the oracle and the replicated stream say of it (once), and the oracle's un-merged list of every 7th read"""

    def __init__(self, W, reads, mates=None):
        self.W, self.reads, self.mates = W, reads, mates
        self.R = len(reads)
        self.packed = synth.pack(reads) + (synth.pack(mates) if mates is not None else ())
        self.want = W.orc.classify_batch(W.p, W.oix, W.parents, *self.packed, thresholds=THR)
        self.rep = W.whole().classify_batch(*self.packed, thresholds=THR, with_hits=True)
        self._lists = self._sends = None

    def lists(self):
        if self._lists is None:
            W = self.W
            self._lists = {i: W.orc.classify_read(W.p, W.oix, W.parents, self.reads[i].tobytes(),
                                                  None if self.mates is None else self.mates[i].tobytes(), 2, 0.0)[1]
                           for i in range(0, self.R, 7)}
        return self._lists

    def sends(self):
        """the SEQUENCE spans of the fragments the lane kernel takes: what the EMIT sends (shard_step_model.expected_sends)"""
        if self._sends is None:
            self._sends = M.expected_sends(self.W.orc, self.W.p, self.reads, self.mates, 1)[0]
        return self._sends

    def handed_back(self):
        """[R] bool, from the oracle's spans and the records: the fragments the lane kernel does not finish -- over 1 000 bases (both
        mates together), or more than 12 distinct taxa other than NONE among their hits (the 12 slots of the APPLY's map)"""
        lens = np.array([len(r) for r in self.reads]) + (np.array([len(r) for r in self.mates]) if self.mates is not None else 0)
        s, lib = self.sends(), self.W.lib
        order = np.argsort(lib.keys)
        at = np.searchsorted(lib.keys[order], s["key"]).clip(max=len(order) - 1)
        tx = np.where(lib.keys[order][at] == s["key"], lib.taxa[order][at], 0)
        pairs = np.unique(np.stack([s["frag"][tx > 0], tx[tx > 0].astype(np.int64)], 1), axis=0) if (tx > 0).any() else np.zeros((0, 2), np.int64)
        return (lens > 1000) | (np.bincount(pairs[:, 0], minlength=self.R) > 12)

    def per_owner(self, n):
        import slacken_amd
        L = slacken_amd.lib()
        return np.bincount(np.array([L.slk_shard_of(int(k), n) for k in self.sends()["key"]], np.int64), minlength=n)


class World:
    """a library in the oracle's index, in the replicated engine index, and sharded over n members (made once per n and placement)"""

    def __init__(self, orc, lib, parents):
        self.orc, self.lib, self.parents, self.p = orc, lib, parents, orc.params()
        self.oix = orc.Index(1, lib.keys, lib.taxa)
        self._members, self._bank, self._whole = {}, {}, None

    def members(self, n, placement="one-device"):
        if (n, placement) not in self._members:
            devices = list(range(n)) if placement == "device-each" else None
            self._members[(n, placement)] = make_members(self.lib, self.parents, n, devices=devices)
        return self._members[(n, placement)]

    def whole(self):
        import slacken_amd
        if self._whole is None:
            ix = slacken_amd.Index(expected_records=len(self.lib.keys), max_taxon=len(self.parents) - 1)
            ix.append(self.lib.keys, self.lib.taxa)
            ix.set_taxonomy(self.parents)
            ix.finalize()
            self._whole = (ix, ix.stream())
        return self._whole[1]

    def batch(self, *key):
        """the bank: one Batch per key, made by make_<kind>(rng, ...) with a generator seeded by the key"""
        if key not in self._bank:
            rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
            made = getattr(self, "make_" + key[0])(rng, *key[1:])
            self._bank[key] = Batch(self, *made) if isinstance(made, tuple) else Batch(self, made)
        return self._bank[key]

    def close(self):
        for ms in self._members.values():
            for ix in ms:
                ix.close()
        if self._whole:
            self._whole[1].close()
            self._whole[0].close()


class Plain(World):
    """the world of test_gpu_shardset.py: 10 genomes of 12 000 bases, 30 000 padding records, a taxonomy of 256 nodes"""

    def __init__(self, orc):
        rng = np.random.default_rng(77)
        parents = taxgen.taxonomy(8 * 32, rng)
        super().__init__(orc, synth.Library(orc, orc.params(), parents, n_genomes=10, genome_len=12000, pad_records=30000), parents)

    def short(self, rng, n):
        """n reads of 50-250 bases: from the genomes with substitutions, random ones, single Ns and runs of Ns, lower case"""
        return [synth.make_reads(self.lib, 1, rng, length=int(L), n_single=0.1, n_run=0.05, short=0)[0] for L in rng.integers(50, 251, n)]

    def long(self, rng, n):
        return [synth.make_reads(self.lib, 1, rng, length=int(L), short=0)[0] for L in rng.integers(1200, 1801, n)]

    def make_plain(self, rng, n):
        return self.short(rng, n)

    def make_pairs(self, rng, n):
        return self.short(rng, n), self.short(rng, n)          # (ragged: the two mates' lengths are drawn apart)

    def make_long(self, rng, n, n_long, paired=False):
        """n fragments, n_long of them of 1 200-1 800 bases (handed back by the lane kernel), anywhere"""
        reads = self.short(rng, n - n_long) + self.long(rng, n_long)
        reads = [reads[i] for i in rng.permutation(n)]
        return (reads, self.short(rng, n)) if paired else reads

    def make_ends(self, rng, n, paired=False):
        """the handed-back fragments are the batch's first and its last"""
        reads = self.long(rng, 1) + self.short(rng, n - 2) + self.long(rng, 1)
        return (reads, self.short(rng, n)) if paired else reads


class Many(World):
    """every minimizer of every read its own record with a random taxon.  `dense` reads (150-250 bases) hit more than 12 distinct taxa
    and are handed back by the lane kernel; `sparse` reads (50-56 bases, at most 6 minimizers: a PAIR of them stays within 12) are not"""

    def __init__(self, orc):
        rng = np.random.default_rng(78)
        parents = taxgen.taxonomy(8 * 32, rng)
        p = orc.params()
        self.dense = [synth.random_dna(int(L), rng) for L in rng.integers(150, 251, 700)]
        self.sparse = []
        while len(self.sparse) < 2400:
            r = synth.random_dna(int(rng.integers(50, 57)), rng)
            if len(np.unique(orc.minimizer_keys(p, r.tobytes()))) <= 6:
                self.sparse.append(r)
        keys = np.unique(np.concatenate([orc.minimizer_keys(p, r.tobytes()) for r in self.dense + self.sparse]))

        class Lib:
            pass
        lib = Lib()
        lib.keys, lib.taxa, lib.genomes = keys, rng.choice(np.array(taxgen.defined_taxa(parents)), size=len(keys)).astype(np.int32), []
        super().__init__(orc, lib, parents)

    @staticmethod
    def draw(rng, pool, n):
        return [pool[i] for i in rng.choice(len(pool), n, replace=False)]

    def make_plain(self, rng, n):
        return self.draw(rng, self.sparse, n)

    def make_pairs(self, rng, n):
        return self.draw(rng, self.sparse, n), self.draw(rng, self.sparse, n)

    def make_long(self, rng, n, n_long, paired=False):            # (here: every fragment over 12 taxa)
        return (self.draw(rng, self.dense, n), self.draw(rng, self.dense, n)) if paired else self.draw(rng, self.dense, n)

    def make_ends(self, rng, n, paired=False):
        reads = self.draw(rng, self.dense, 1) + self.draw(rng, self.sparse, n - 2) + self.draw(rng, self.dense, 1)
        return (reads, self.draw(rng, self.sparse, n)) if paired else reads


@pytest.fixture(scope="module")
def worlds(orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = (Plain if name == "plain" else Many)(orc)
        return made[name]
    yield get
    for w in made.values():
        w.close()


def devices_or_skip(n):
    import slacken_amd
    have = int(slacken_amd.lib().slk_device_count())
    if have < n:
        pytest.skip(f"a device per member needs {n} devices, this machine has {have}")


def matrix(rounds):
    return [[None if B is None else B.packed for B in row] for row in rounds]


def check(rounds, outs, hits):
    """every batch of every round: rows against the oracle and the replicated stream; hit lists (where asked for: `hits` is a bool or a
    [rounds][members] matrix) as WHOLE arrays against the replicated stream's and list by list, every 7th read, against the oracle's"""
    assert len(outs) == len(rounds)
    for r, (row, orow) in enumerate(zip(rounds, outs)):
        assert len(orow) == len(row)
        for g, (B, o) in enumerate(zip(row, orow)):
            if B is None:
                assert o is None, (r, g)
                continue
            h = hits[r][g] if isinstance(hits, list) else hits
            same(o, B.want, h)
            for key in ROWS:
                assert np.array_equal(o[key], B.rep[key]), (r, g, key)
            if not h:
                assert "hits" not in o
                continue
            assert np.array_equal(o["hit_offsets"], B.rep["hit_offsets"]), (r, g)
            assert np.array_equal(o["hits"], B.rep["hits"]), (r, g)
            ho = o["hit_offsets"].astype(np.int64)
            for i, want in B.lists().items():
                got = o["hits"][ho[i]:ho[i + 1]]
                assert [(int(t), int(c)) for t, c in zip(got["taxon"], got["count"])] == want, (r, g, i)


def equal_outputs(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), key


# sizes (reads per batch).  Round 0 takes the small ones, the later rounds the others -- dealt out so that the members of a round, a
# round and the round that takes its slot again (r + 6), and a round and the rounds sharing a step with it (r + 2, r + 4) all differ.
SMALL = [100, 112, 124, 136, 148]
BIG = [260, 600, 330, 540, 410, 480, 290, 570, 360, 450, 520]


def grown_rounds(W, n, R):
    """R rounds for n members, uneven per member and round; asserts on the oracle's spans that some member's keys GROW within the call
    by more than 1.25 x plus a page: a bounce buffer (sized 1.25 x + 4096 bytes of the 8-byte keys a member sends) is then
    reallocated while the call is running"""
    rounds = [[W.batch("plain", SMALL[g] if r == 0 else BIG[(r * 7 + g * 3) % len(BIG)]) for g in range(n)] for r in range(R)]
    sent = np.array([[8 * len(B.sends()) for B in row] for row in rounds])
    assert any(sent[r, g] > 1.25 * sent[:r, g].max() + 4096 for g in range(n) for r in range(1, R))
    return rounds


def run_both(sset, rounds, one_by_one=False):
    for with_hits in (True, False):
        outs = sset.classify_rounds(matrix(rounds), thresholds=THR, with_hits=with_hits)
        check(rounds, outs, with_hits)
        if one_by_one and with_hits:             # the same batches one round at a time: no two rounds share a step
            for row, orow in zip(rounds, outs):
                for a, b in zip(sset.classify(matrix([row])[0], thresholds=THR), orow):
                    equal_outputs(a, b)


# ---- a. rounds x members ---------------------------------------------------------------------------------------------------------
# members: 5 is the first count where slk_shard_chunk drops to 128.  rounds: 2 never overlap an APPLY, 5 is the first step carrying all
# three jobs, 7 the first reuse of slot 0, 13 two turns of the slot ring and four of the key ring.
@NO_PEER
@pytest.mark.parametrize("R", [2, 5, 7, 13])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_rounds_by_members(worlds, n, R, no_peer, monkeypatch):
    import slacken_amd
    from slacken_amd import capi
    set_no_peer(monkeypatch, no_peer)
    W = worlds("plain")
    assert slacken_amd.lib().slk_shard_chunk(5) == 128 and slacken_amd.lib().slk_shard_chunk(3) > 128
    rounds = grown_rounds(W, n, R)
    sset = capi.ShardSet(W.members(n))
    try:
        staged_as_asked(sset, no_peer)
        run_both(sset, rounds, one_by_one=True)
    finally:
        sset.close()


@NO_PEER
def test_one_set_takes_call_after_call(worlds, no_peer, monkeypatch):
    """5 rounds twice in a row, then 13, through ONE set: the slots, rings and events as an earlier call left them"""
    from slacken_amd import capi
    set_no_peer(monkeypatch, no_peer)
    W = worlds("plain")
    sset = capi.ShardSet(W.members(3))
    try:
        staged_as_asked(sset, no_peer)
        for R in (5, 5, 13):
            run_both(sset, grown_rounds(W, 3, R))
    finally:
        sset.close()


# ---- b. empty batches in every role -----------------------------------------------------------------------------------------------
def empties(shape, r, g):
    return {"middle": (r, g) == (3, 1),                  # one member without a batch in a middle round
            "always": g == 2,                            # a member that only answers keys
            "whole_round": r == 3,                       # nobody has a batch, between two full rounds
            "first_and_last": r in (0, 6)}[shape]


@NO_PEER
@pytest.mark.parametrize("shape", ["middle", "always", "whole_round", "first_and_last"])
def test_empty_batches(worlds, shape, no_peer, monkeypatch):
    from slacken_amd import capi
    set_no_peer(monkeypatch, no_peer)
    W = worlds("plain")
    rounds = [[None if empties(shape, r, g) else B for g, B in enumerate(row)] for r, row in enumerate(grown_rounds(W, 3, 7))]
    assert any(B is None for row in rounds for B in row)
    sset = capi.ShardSet(W.members(3))
    try:
        staged_as_asked(sset, no_peer)
        run_both(sset, rounds)                           # (check: None results where the batches were None, all else exact)
    finally:
        sset.close()


# ---- c. hit lists that differ -----------------------------------------------------------------------------------------------------
def test_hit_lists_that_differ_inside_a_step(worlds):
    """EMIT(t) and APPLY(t - 4) of one step must agree about hit lists, or the replay goes alone (launch_step): member 0 wants lists in
    round 1 and none in round 5 and the reverse in rounds 3 / 7, member 1 the reverse in rounds 2 / 6 and lists in round 4, none in
    round 8; in round 1 (and others) the two members of one round differ"""
    from slacken_amd import capi
    W = worlds("plain")
    T, F = True, False
    m0 = [T, T, F, F, T, F, F, T, T]
    m1 = [T, F, F, T, T, F, T, T, F]
    assert (m0[1], m0[5], m0[3], m0[7]) == (T, F, F, T) and (m1[2], m1[6], m1[4], m1[8]) == (F, T, T, F) and m0[1] != m1[1]
    hits = [[a, b] for a, b in zip(m0, m1)]
    rounds = grown_rounds(W, 2, 9)
    sset = capi.ShardSet(W.members(2))
    try:
        check(rounds, sset.classify_rounds(matrix(rounds), thresholds=THR, with_hits=hits), hits)
    finally:
        sset.close()


# ---- d. handed-back fragments in mid-pipeline -------------------------------------------------------------------------------------
@NO_PEER
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("world", ["plain", "many"])
def test_handed_back_fragments_in_mid_pipeline(worlds, world, paired, no_peer, monkeypatch):
    """rounds 1 and 3 of 6 hold what the lane kernel hands back -- plain world: 12 and 15 fragments of 1 200-1 800 bases; many-taxa
    world: every fragment over 12 distinct taxa -- and one batch whose handed-back fragments are its first and its last.  Their
    staged round runs after the pipeline has drained; with hit lists its lists are spliced into the pipeline's (finish_deferred)."""
    from slacken_amd import capi
    set_no_peer(monkeypatch, no_peer)
    W = worlds(world)
    rounds = [[W.batch("pairs" if paired else "plain", 110 + 30 * r + 17 * g) for g in range(2)] for r in range(6)]
    rounds[1] = [W.batch("long", 200, 12, paired), W.batch("ends", 130, paired)]
    rounds[3] = [rounds[3][0], W.batch("long", 150, 15, paired)]
    # the preconditions, on the oracle: what is handed back (over 1 000 bases, both mates together, or over 12 distinct taxa) and where
    for B, n_back in ((rounds[1][0], 12), (rounds[3][1], 15)):
        assert B.handed_back().sum() == (n_back if world == "plain" else B.R)
    assert np.array_equal(np.nonzero(rounds[1][1].handed_back())[0], [0, rounds[1][1].R - 1])
    if world == "many":                                   # (every hit group a taxon of its own here, up to the draw's repeats)
        assert (rounds[1][0].want["num_distinct"] > 12).all() and (rounds[3][1].want["num_distinct"] > 12).all()
        assert (rounds[1][1].want["num_distinct"][[0, -1]] > 12).all() and (rounds[1][1].want["num_distinct"][1:-1] <= 12).all()
    for r in (0, 2, 4, 5):
        assert not any(B.handed_back().any() for B in rounds[r])
    sset = capi.ShardSet(W.members(2))
    try:
        staged_as_asked(sset, no_peer)
        run_both(sset, rounds)
    finally:
        sset.close()


# ---- e. pairs -----------------------------------------------------------------------------------------------------------------------
def test_pairs_through_five_rounds(worlds, orc):
    from slacken_amd import capi
    W = worlds("plain")
    rounds = [[W.batch("pairs", 120 + 40 * r + 25 * g) for g in range(2)] for r in range(5)]
    sset = capi.ShardSet(W.members(2))
    try:
        outs = sset.classify_rounds(matrix(rounds), thresholds=THR)
        check(rounds, outs, True)
        for row, orow in zip(rounds, outs):
            for B, o in zip(row, orow):
                assert any(len(a) != len(b) for a, b in zip(B.reads, B.mates))
                # the mate border's pseudo-span: once in every list
                at = np.nonzero(o["hits"]["taxon"] == capi.TAXON_MATE_PAIR_BORDER)[0]
                assert np.array_equal(np.searchsorted(o["hit_offsets"].astype(np.int64), at, side="right") - 1, np.arange(B.R))
        same_hits(orc, dict(p=W.p, oix=W.oix, parents=W.parents), outs[4][1], rounds[4][1].reads, rounds[4][1].mates, step=5)
    finally:
        sset.close()


# ---- f. a region that overflows in mid-pipeline -----------------------------------------------------------------------------------
HEALTHY = [100, 115, 130, 145, 160, 175, 190]
LARGE = {"round_2_member_1": [(2, 1)], "first_round": [(0, 0)], "last_round": [(5, 1)], "both_members": [(3, 0), (3, 1)]}


@NO_PEER
@pytest.mark.parametrize("where", list(LARGE))
def test_region_overflows_in_mid_pipeline(worlds, where, no_peer, monkeypatch):
    """Under SLK_SHARDSET_REGION_CAP one batch's keys do not fit an owner's send region: nothing of it travels, its slot is marked
    failed, the steps after it go on, and all of it comes back through the staged round -- exact like every other batch."""
    import slacken_amd
    from slacken_amd import capi
    set_no_peer(monkeypatch, no_peer)
    W = worlds("plain")
    n = 2
    chunk = int(slacken_amd.lib().slk_shard_chunk(n))
    rounds = [[W.batch("plain", HEALTHY[(r * 3 + g * 5) % len(HEALTHY)]) for g in range(n)] for r in range(6)]
    for i, (r, g) in enumerate(LARGE[where]):
        rounds[r][g] = W.batch("plain", 600 - 10 * i)
    healthy = [B for r, row in enumerate(rounds) for g, B in enumerate(row) if (r, g) not in LARGE[where]]
    tiles = lambda B: (B.R + 63) // 64
    # never too small for a healthy batch (test_gpu_shard_step.py, Batch.safe_cap): a wave that emits holds at most one part-filled
    # chunk per owner, and there are at most `tiles` such waves
    cap = max((-(-int(B.per_owner(n).max()) // chunk) + tiles(B)) * chunk for B in healthy)
    assert cap % chunk == 0
    for B in healthy:
        assert int(B.per_owner(n).max()) + chunk * tiles(B) <= cap
    for r, g in LARGE[where]:
        assert int(rounds[r][g].per_owner(n).max()) > cap
    sset = capi.ShardSet(W.members(n))
    try:
        staged_as_asked(sset, no_peer)
        monkeypatch.setenv("SLK_SHARDSET_REGION_CAP", str(cap))
        run_both(sset, rounds)
        monkeypatch.delenv("SLK_SHARDSET_REGION_CAP")
        run_both(sset, rounds)                           # an ordinary call on the same set
    finally:
        sset.close()


# ---- g. device-resident rounds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_device_resident_rounds(worlds, n):
    import torch
    import slacken_amd
    from slacken_amd import capi
    W = worlds("plain")
    dev = torch.device("cuda", 0)
    rounds = grown_rounds(W, n, 7)
    rounds[2][1] = W.batch("long", 200, 12)
    sset = capi.ShardSet(W.members(n))
    try:
        host = sset.classify_rounds(matrix(rounds), thresholds=THR, with_hits=False)
        check(rounds, host, False)
        args, keep = [], []
        for row in rounds:
            arow = []
            for B in row:
                b, o = (torch.from_numpy(a.view(dt)).to(dev) for a, dt in zip(B.packed, (np.uint8, np.int64)))   # (exactly offsets[R] bytes)
                out = dict(taxon=torch.full((len(THR) * B.R,), -7, dtype=torch.int32, device=dev),
                           classified=torch.full((len(THR) * B.R,), 9, dtype=torch.uint8, device=dev),
                           num_distinct=torch.full((B.R,), -7, dtype=torch.int32, device=dev),
                           total_kmers=torch.full((B.R,), -7, dtype=torch.int32, device=dev))
                keep.append((b, o, out))
                arow.append(dict(bases=b.data_ptr(), offsets=o.data_ptr(), R=B.R, out_taxon=out["taxon"].data_ptr(),
                                 out_classified=out["classified"].data_ptr(), out_num_distinct=out["num_distinct"].data_ptr(),
                                 out_total_kmers=out["total_kmers"].data_ptr()))
            args.append(arow)
        torch.cuda.synchronize()
        sset.classify_rounds_device(args, thresholds=THR)
        torch.cuda.synchronize()
        it = iter(keep)
        for row, hrow in zip(rounds, host):
            for B, h in zip(row, hrow):
                out = next(it)[2]
                for key in ROWS:
                    got = out[key].cpu().numpy().reshape(h[key].shape)
                    assert np.array_equal(got, h[key]) and np.array_equal(got, B.want[key]), key
        # hit lists are not to be had from device-resident rounds: refused before anything is queued
        args[3][0]["out_hit_offsets"] = keep[0][1].data_ptr()
        with pytest.raises(slacken_amd.SlackenError) as e:
            sset.classify_rounds_device(args, thresholds=THR)
        assert e.value.code == capi.E_UNSUPPORTED
    finally:
        sset.close()


# ---- i. an error in mid-pipeline leaves a usable set ------------------------------------------------------------------------------
def test_error_in_mid_pipeline_leaves_a_usable_set(worlds):
    """hits_capacity too small for ONE batch, in round 2 of 6: SLK_E_CAPACITY (the host compares the count with the capacity before
    it copies anything), found while the steps of the rounds behind it are queued.  The same set then classifies the same six rounds"""
    import slacken_amd
    from slacken_amd import capi
    W = worlds("plain")
    rounds = grown_rounds(W, 2, 6)
    caps = [[None, None] for _ in rounds]
    caps[2][1] = int(rounds[2][1].want["num_hits"].sum()) - 1
    assert caps[2][1] > 0
    sset = capi.ShardSet(W.members(2))
    try:
        with pytest.raises(slacken_amd.SlackenError) as e:
            sset.classify_rounds(matrix(rounds), thresholds=THR, hits_capacity=caps)
        assert e.value.code == capi.E_CAPACITY
        caps[2][1] += 1                                  # exactly what the batch needs
        check(rounds, sset.classify_rounds(matrix(rounds), thresholds=THR, hits_capacity=caps), True)
        run_both(sset, rounds)
    finally:
        sset.close()


# ---- j. placement -----------------------------------------------------------------------------------------------------------------
@NO_PEER
@PLACEMENT
def test_seven_rounds_of_two_members_by_placement(worlds, placement, no_peer, monkeypatch):
    """one-device: both members on device 0.  device-each: member g on device g, copies -- between devices, directly where
    hipDeviceCanAccessPeer allows it, else (or with the switch) through the sender's bounce buffer"""
    import torch
    from slacken_amd import capi
    n = 2
    if placement == "device-each":
        devices_or_skip(n)
    set_no_peer(monkeypatch, no_peer)
    W = worlds("plain")
    rounds = grown_rounds(W, n, 7)
    sset = capi.ShardSet(W.members(n, placement), exchange=capi.EXCHANGE_COPY)
    try:
        if placement == "one-device":
            staged_as_asked(sset, no_peer)
        else:
            no_access = sum(not torch.cuda.can_device_access_peer(b, a) for a in range(n) for b in range(n) if a != b)
            print(f"device-each, copy mode: staged_pairs = {sset.staged_pairs}, pairs without peer access = {no_access}")
            assert sset.exchange_mode == capi.EXCHANGE_COPY
            assert sset.staged_pairs == (n * (n - 1) if no_peer else no_access)
        run_both(sset, rounds, one_by_one=True)
    finally:
        sset.close()


RCCL_ROUNDS_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import torch  # (as in the test session: PyTorch's HIP runtime first)
import slacken_amd, synth, taxgen
from slacken_amd import capi
rng = np.random.default_rng(6)
parents = taxgen.taxonomy(8 * 16, rng)
taxa = np.array(taxgen.defined_taxa(parents))
sizes = [[120, 150], [400, 330], [250, 0], [560, 210], [180, 470], [300, 260], [140, 520]]
rounds = [[[synth.random_dna(int(L), rng) for L in rng.integers(50, 251, s)] for s in row] for row in sizes]
rounds[3][1] += [synth.random_dna(1500, rng) for _ in range(5)]
# records: the minimizers of every third read (the oracle is not needed for them: the engine's own spans)
every = [r for row in rounds for reads in row for r in reads]
k0 = np.unique((rng.integers(0, 2**62, 2000, dtype=np.int64) * 4) & ~np.int64(0x33333330))
ix0 = slacken_amd.Index(expected_records=len(k0), max_taxon=len(parents) - 1)
ix0.append(k0, rng.choice(taxa, size=len(k0)).astype(np.int32)); ix0.set_taxonomy(parents); ix0.finalize()
so, spans = ix0.stream().spans_batch(*synth.pack(every[::3]))
keys = np.unique(spans["key"][spans["flag"] == 1])
tx = rng.choice(taxa, size=len(keys)).astype(np.int32)
whole = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1)
whole.append(keys, tx); whole.set_taxonomy(parents); whole.finalize()
wst = whole.stream()
members = []
for g in range(2):
    ix = slacken_amd.Index(expected_records=len(keys), max_taxon=len(parents) - 1, device=g)
    ix.set_shard(g, 2); ix.append(keys, tx); ix.set_taxonomy(parents); ix.finalize()
    members.append(ix)
sset = capi.ShardSet(members, exchange=capi.EXCHANGE_AUTO)
assert sset.exchange_mode == capi.EXCHANGE_RCCL and sset.staged_pairs == 0
packed = [[synth.pack(reads) if reads else None for reads in row] for row in rounds]
classified = 0
for _ in range(2):
    outs = sset.classify_rounds(packed, thresholds=(0.0, 0.2))
    for prow, orow in zip(packed, outs):
        for pk, got in zip(prow, orow):
            if pk is None:
                assert got is None
                continue
            want = wst.classify_batch(*pk, thresholds=(0.0, 0.2))
            classified += int(want["classified"][0].sum())
            for k in ("taxon", "classified", "num_distinct", "total_kmers", "hit_offsets", "hits"):
                assert np.array_equal(got[k], want[k]), k
assert classified > 1000
sset.close()
print("RCCL-ROUNDS-OK")
"""


def test_rccl_rounds_with_a_device_per_member(tmp_path):
    """Two members on two devices, SLK_EXCHANGE_AUTO: the exchange is RCCL's, seven pipelined rounds (one member without a batch in one
    of them, long fragments in another) against the replicated stream.  In a child process under a time limit, as
    test_rccl_leg_runs_with_one_member: a collective library that does not come up must not take the session with it."""
    devices_or_skip(2)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl_rounds.py"
    script.write_text(RCCL_ROUNDS_SCRIPT.format(root=root))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "RCCL-ROUNDS-OK" in p.stdout, p.stderr[-3000:]
