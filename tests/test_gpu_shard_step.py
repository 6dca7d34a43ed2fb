"""The table-sharded step kernel (lane_step_kernel through slk_shard_step_device) held to the contract of its lists
(include/slacken_amd.h: slk_shard_lists; engine.h: ShardIO, ApplyJob), not only to the final rows: every EMIT runs on buffers filled
with sentinels, everything it wrote is copied back, and tests/shard_step_model.py replays the probe log against the oracle's spans.

ONE index holds the whole table here: slk_lookup_device (or a LOOKUP job) on the keys of region g, answered into the same positions
of d_taxa, stands in for owner g -- no exchange, and one process covers any n_shards on one GPU.  All comparisons are exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import slacken_amd
from slacken_amd import capi

import shard_step_model as M
import synth
import taxgen

pytestmark = pytest.mark.gpu

KEY_SENT = 0x5A5A5A5A5A5A5A5B          # low bits set: no left-aligned minimizer of m <= 31 bases (2 m <= 62 bits) looks like this
META_SENT = -1                         # 0xFFFFFFFF: 8191 k-mers in one span of a fragment of at most 1000 bases
WORD_SENT = 0xEEEEEEEE - (1 << 32)     # log, tile rows, read info, span arrays, results (as int32)
TAXA_SENT = -77                        # an answer nobody gave
GUARD = 1024                           # entries behind every array (at least one chunk behind the last send region)
THR = (0.0, 0.15)
DEV = torch.device("cuda", 0)
OTHER = dict(k=21, m=12, spaces=5)     # w = 10: the van-Herk variant of the scan


class World:
    """a synthetic library in an engine index (the whole table) and in the oracle's, for one splitter"""

    def __init__(self, orc, ps=None, seed=77, n_genomes=6, genome_len=8000, pad=6000):
        ps = dict(ps or {})
        self.orc = orc
        self.p = orc.params(**ps)
        rng = np.random.default_rng(seed)
        self.parents = taxgen.taxonomy(8 * 32, rng)
        self.lib = synth.Library(orc, self.p, self.parents, n_genomes=n_genomes, genome_len=genome_len, pad_records=pad)
        self.ix = slacken_amd.Index(expected_records=len(self.lib.keys), max_taxon=len(self.parents) - 1, **ps)
        self.ix.append(self.lib.keys, self.lib.taxa)
        self.ix.set_taxonomy(self.parents)
        self.ix.finalize()
        self.oix = orc.Index(1, self.lib.keys, self.lib.taxa)
        self.st = self.ix.stream()
        self.w = self.p.k - self.p.m + 1
        self._known = {}
        self._models = {}

    def lookup(self, keys):
        """orc.Index.lookup of every key"""
        keys = np.asarray(keys, np.int64)
        uniq, inv = np.unique(keys, return_inverse=True)
        known = self._known
        for k in uniq.tolist():
            if k not in known:
                known[k] = self.oix.lookup([k & (2**64 - 1)])
        return np.array([known[k] for k in uniq.tolist()], np.int32)[inv].reshape(keys.shape)

    def model(self, reads, mates):
        """what the oracle says of a set of fragments, computed once: spans that travel, read info, rows, hit lists on demand"""
        key = (id(reads), id(mates))
        if key not in self._models:
            sends, _, info, taken = M.expected_sends(self.orc, self.p, reads, mates, 1)
            b, o = synth.pack(reads)
            mb, mo = synth.pack(mates) if mates is not None else (None, None)
            want = self.orc.classify_batch(self.p, self.oix, self.parents, b, o, mb, mo, thresholds=THR) if len(reads) else None
            # the APPLY's map of a fragment has 12 slots for taxa other than NONE: "more than 12 distinct taxa" goes back to the caller
            tx = self.lookup(sends["key"])
            pairs = np.unique(np.stack([sends["frag"][tx > 0], tx[tx > 0].astype(np.int64)], 1), axis=0) if (tx > 0).any() else np.zeros((0, 2), np.int64)
            many = np.bincount(pairs[:, 0], minlength=len(reads)) > 12
            self._models[key] = dict(sends=sends, info=info, taken=taken, want=want, keep=(reads, mates), packed=(b, o, mb, mo),
                                     back=~taken | many)
        return self._models[key]

    def hit_lists(self, reads, mates):
        m = self.model(reads, mates)
        if "hits" not in m:
            m["hits"] = [self.orc.classify_read(self.p, self.oix, self.parents, reads[r].tobytes(),
                                                mates[r].tobytes() if mates is not None else None, 2, 0.0)[1] for r in range(len(reads))]
            m["spans"] = [self.orc.spans(self.p, reads[r].tobytes(), mates[r].tobytes() if mates is not None else None)
                          if m["taken"][r] else [] for r in range(len(reads))]
        return m["hits"], m["spans"]


@pytest.fixture(scope="module")
def worlds(orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(orc, OTHER if name == "w10" else None)
        return made[name]
    yield get
    for w in made.values():
        w.st.close()
        w.ix.close()


def _full(n, value, dtype):
    return torch.full((max(int(n), 1),), value, dtype=dtype, device=DEV)


class Batch:
    """a batch, the oracle's view of it and its device state through the three jobs"""

    def __init__(self, W, reads, mates=None, n_shards=1, hits=False, cap=None):
        lib = slacken_amd.lib()
        self.W, self.reads, self.mates, self.n, self.hits = W, reads, mates, n_shards, hits
        self.R = R = len(reads)
        self.m = W.model(reads, mates)
        self.sends = self.m["sends"]
        self.owner = M.shard_of(self.sends["key"], n_shards)
        self.keys_g = np.bincount(self.owner, minlength=n_shards)
        self.chunk = int(lib.slk_shard_chunk(n_shards))
        assert self.chunk == M.chunk_of(n_shards)
        self.tiles = (R + 63) // 64
        # never too small: a wave that emits holds at most one part-filled chunk per owner, and there are at most `tiles` such waves
        self.safe_cap = (-(-int(self.keys_g.max()) // self.chunk) + max(self.tiles, 1)) * self.chunk
        self.cap = cap or self.safe_cap
        b, o, mb, mo = self.m["packed"]
        self.total, self.mtotal = int(o[-1]), int(mo[-1]) if mo is not None else 0
        self.rows = int(lib.slk_shard_batch_rows(self.total, self.mtotal, R, 1 if mates is not None else 0))
        self.slots = self.total + ((self.mtotal + R) if mates is not None else 0) + 1
        self.region = o[:R].astype(np.int64) + ((mo[:R].astype(np.int64) + np.arange(R)) if mates is not None else 0)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if len(a) else np.zeros(1, dt)).to(DEV)
        # (device buffers of exactly offsets[R] bytes: the kernels read nothing past them)
        self.d = dict(bases=dev(b, np.uint8), offsets=dev(o, np.int64))
        if mates is not None:
            self.d.update(mate_bases=dev(mb, np.uint8), mate_offsets=dev(mo, np.int64))
        big = n_shards * max(self.cap, self.safe_cap)
        self.t = dict(send_keys=_full(big + GUARD, KEY_SENT, torch.int64), send_meta=_full(big + GUARD, META_SENT, torch.int32),
                      cursors=_full(n_shards + 3 + 8, 0x77, torch.int64), log=_full((self.rows + 16) * n_shards * 4, WORD_SENT, torch.int32),
                      tile_rows=_full(2 * self.tiles + 16, WORD_SENT, torch.int32), read_info=_full(2 * R + 16, WORD_SENT, torch.int32),
                      defer=_full(R + 16, 5, torch.int32), taxa=_full(big + GUARD, TAXA_SENT, torch.int32))
        if hits:
            self.t.update(span_meta=_full(self.slots + 16, WORD_SENT, torch.int32), span_taxon=_full(self.slots + 16, WORD_SENT, torch.int32),
                          span_count=_full(R + 16, WORD_SENT, torch.int32))
        self.out = dict(taxon=_full(len(THR) * R + 16, WORD_SENT, torch.int32), classified=_full(len(THR) * R + 16, 0xEE, torch.uint8),
                        num_distinct=_full(R + 16, WORD_SENT, torch.int32), total_kmers=_full(R + 16, WORD_SENT, torch.int32),
                        num_hits=_full(R + 16, WORD_SENT, torch.int32))
        self.h = {}

    def sentinels(self, cap=None):
        """before an EMIT: everything it may write holds a sentinel"""
        if cap is not None:
            self.cap = cap
        for k, v in (("send_keys", KEY_SENT), ("send_meta", META_SENT), ("log", WORD_SENT), ("tile_rows", WORD_SENT),
                     ("read_info", WORD_SENT), ("defer", 5), ("cursors", 0x77), ("taxa", TAXA_SENT), ("span_meta", WORD_SENT),
                     ("span_taxon", WORD_SENT), ("span_count", WORD_SENT)):
            if k in self.t:
                self.t[k].fill_(v)

    def lists(self):
        t, d = self.t, self.d
        ptr = lambda x: x.data_ptr() if x is not None else None
        return capi.ShardLists(ptr(d["bases"]), ptr(d["offsets"]), ptr(d.get("mate_bases")), ptr(d.get("mate_offsets")), self.R, self.total,
                               self.mtotal, self.n, 0, self.cap, ptr(t["send_keys"]), ptr(t["send_meta"]), ptr(t["cursors"]), ptr(t["log"]),
                               ptr(t["tile_rows"]), ptr(t["read_info"]), ptr(t["defer"]), ptr(t.get("span_meta")), ptr(t.get("span_taxon")),
                               ptr(t.get("span_count")))

    def lookup_job(self):
        """every region in one array: [0, n_shards * cap), answered into the same positions"""
        return capi.ShardLookup(self.t["send_keys"].data_ptr(), self.n * self.cap, self.t["taxa"].data_ptr())

    def results(self):
        o = self.out
        self.thr = (C.c_double * len(THR))(*THR)
        return capi.ShardResults(self.t["taxa"].data_ptr(), 2, len(THR), self.thr, o["taxon"].data_ptr(), o["classified"].data_ptr(),
                                 o["num_distinct"].data_ptr(), o["total_kmers"].data_ptr(), o["num_hits"].data_ptr())

    def fetch(self):
        torch.cuda.synchronize()
        self.h = {k: v.cpu().numpy() for k, v in list(self.t.items()) + list(self.out.items())}
        return self.h


def step(W, emit=None, lookup=None, apply=None):
    """one slk_shard_step_device call, waited for (raises what slk_stream_synchronize reports)"""
    torch.cuda.synchronize()
    args = (emit.lists() if emit is not None else None, lookup, apply.lists() if apply is not None else None,
            apply.results() if apply is not None else None)
    W.st.shard_step(*args)
    W.st.synchronize()


def owners_answer(b):
    """the owners' side with slk_lookup_device: region g's keys [0, cursors[g]) answered into the same positions of d_taxa"""
    torch.cuda.synchronize()
    cur = b.t["cursors"].cpu().numpy()
    for g in range(b.n):
        if cur[g]:
            b.W.st.lookup_device(b.t["send_keys"].data_ptr() + 8 * g * b.cap, int(cur[g]), b.t["taxa"].data_ptr() + 4 * g * b.cap)
    b.W.st.synchronize()


def check_emit(b, overflowed=False):
    """the contract of the lists after an EMIT (slacken_amd.h: slk_shard_lists; engine.h: ShardIO) -> the replay"""
    h = b.fetch()
    n, cap, chunk, R, tiles = b.n, b.cap, b.chunk, b.R, b.tiles
    cur = h["cursors"][:n].astype(np.int64)
    keys, meta = h["send_keys"], h["send_meta"]
    assert (cur % chunk == 0).all(), cur
    if overflowed:
        assert cur[int(np.argmax(b.keys_g))] > cap, (cur, cap)
    else:
        assert (cur <= cap).all(), (cur, cap)
    assert h["cursors"][n + 2] == 0 and (h["cursors"][n + 3:] == 0x77).all()
    lim = np.minimum(cur, cap)
    # filled from the front without holes; nothing behind the cursor, nothing behind the last region
    for g in range(n):
        reg = keys[g * cap:(g + 1) * cap]
        assert (reg[:lim[g]] != KEY_SENT).all(), f"owner {g}: a hole below its cursor"
        assert (reg[lim[g]:] == KEY_SENT).all(), f"owner {g}: written at or behind its cursor"
        assert (meta[g * cap + lim[g]:(g + 1) * cap] == META_SENT).all(), f"owner {g}: metadata behind its cursor"
    assert (keys[n * cap:] == KEY_SENT).all() and (meta[n * cap:] == META_SENT).all(), "the guard behind the last region"
    assert (h["log"][b.rows * n * 4:] == WORD_SENT).all() and (h["tile_rows"][2 * tiles:] == WORD_SENT).all()
    assert (h["read_info"][2 * R:] == WORD_SENT).all() and (h["defer"][R:] == 5).all()
    # the tiles' rows
    tr = h["tile_rows"][:2 * tiles].view(np.uint32).reshape(tiles, 2).astype(np.int64)
    by = tr[np.argsort(tr[:, 0], kind="stable")]
    assert (by[:-1, 0] + by[:-1, 1] <= by[1:, 0]).all(), "rows of two tiles overlap"
    assert tiles == 0 or int((tr[:, 0] + tr[:, 1]).max()) <= b.rows
    # the log
    log = h["log"][:b.rows * n * 4].view(np.uint32).reshape(b.rows, n, 4)
    sends, addr, owner_of, dropped, beyond = M.replay(log, tr, keys, meta, cur, cap, n, R)
    assert len(np.unique(addr)) == len(addr), "two probes share a position"
    assert beyond == 0, "a probe lies at or behind its owner's cursor"
    assert np.array_equal(M.shard_of(keys[addr], n), owner_of), "a key in another owner's region"
    asked = np.zeros(n * cap, bool)
    asked[addr] = True
    for g in range(n):
        sl = slice(g * cap, g * cap + lim[g])
        assert (keys[sl][~asked[sl]] == 0).all(), f"owner {g}: a position nobody asks for holds a key"
    want = b.sends
    if not b.hits:       # (the ordinal travels only when hit lists are written)
        want = want.copy()
        want["ordinal"] = 0
        want = M.sort_sends(want)
    if overflowed:
        assert dropped > 0 and dropped + len(sends) == len(want)
        have = {}
        for row in want.tolist():
            have[row] = have.get(row, 0) + 1
        for row in sends.tolist():
            have[row] = have.get(row, 0) - 1
            assert have[row] >= 0, "a region holds what was not the batch's to send"
    else:
        assert dropped == 0
        assert np.array_equal(sends, want), "the replayed probes are not the oracle's spans"
        assert np.array_equal(np.bincount(owner_of, minlength=n), b.keys_g)
        taken = b.m["taken"]
        info = h["read_info"][:2 * R].reshape(R, 2)
        assert np.array_equal(info[taken], b.m["info"][taken])
    assert np.array_equal(h["defer"][:R], (~b.m["taken"]).astype(np.int32)), "defer == 1 exactly for the fragments over 1000 bases"
    return addr


def check_answers(b, addr):
    """the owners' answers at the positions of the keys"""
    h = b.fetch()
    assert np.array_equal(h["taxa"][addr], b.W.lookup(h["send_keys"][addr]))
    assert (h["taxa"][b.n * b.cap:] == TAXA_SENT).all()


def check_apply(b):
    h = b.fetch()
    R, n = b.R, b.n
    defer = h["defer"][:R] != 0
    assert np.array_equal(defer, b.m["back"]), "defer == 1 exactly for the fragments over 1000 bases or with more than 12 distinct taxa"
    assert h["cursors"][n + 2] == defer.sum()
    if R == 0:
        return
    want = b.m["want"]
    ok = ~defer
    Cn = len(THR)
    assert np.array_equal(h["taxon"][:Cn * R].reshape(Cn, R)[:, ok], want["taxon"][:, ok])
    assert np.array_equal(h["classified"][:Cn * R].reshape(Cn, R)[:, ok], want["classified"][:, ok])
    for k in ("num_distinct", "total_kmers", "num_hits"):
        assert np.array_equal(h[k][:R][ok], want[k][ok]), k
    assert (h["num_hits"][:R][defer] == 0).all()
    for k in ("taxon", "classified"):
        assert (h[k][Cn * R:] == (0xEE if k == "classified" else WORD_SENT)).all()
    if b.hits:
        hits, spans = b.W.hit_lists(b.reads, b.mates)
        cnt = h["span_count"][:R]
        assert np.array_equal(cnt[ok], want["num_hits"][ok]) and (cnt[defer] == 0).all()
        for r in np.nonzero(ok)[0]:
            sl = slice(int(b.region[r]), int(b.region[r]) + int(cnt[r]))
            sm, stx = h["span_meta"][sl], h["span_taxon"][sl]
            assert list(zip(stx.tolist(), (sm >> 4).tolist())) == hits[r], r
            assert [((x >> 1) & 7, x & 1) for x in sm.tolist()] == [(s["flag"], int(s["distinct"])) for s in spans[r]], r
        assert (h["span_meta"][b.slots:] == WORD_SENT).all() and (h["span_taxon"][b.slots:] == WORD_SENT).all()


def through(b):
    """one batch through its three jobs, a step each, everything checked"""
    b.sentinels()
    step(b.W, emit=b)
    addr = check_emit(b)
    owners_answer(b)
    check_answers(b, addr)
    step(b.W, apply=b)
    check_apply(b)


def edge_reads(W, rng, n, paired=False):
    """n fragments: mostly short ones of the library, and every special case of the fast route's borders"""
    lib = W.lib
    acgt = lambda L: synth.make_reads(lib, 1, rng, length=L, short=0, n_single=0, n_run=0, lowercase=0)[0]
    special = [np.zeros(0, np.uint8), acgt(W.p.k - 1), acgt(W.p.k), np.full(90, ord("N"), np.uint8), acgt(1000), acgt(1001),
               acgt(1), np.full(W.p.k - 1, ord("N"), np.uint8)]
    reads = synth.make_reads(lib, n - len(special), rng, n_single=0.1, n_run=0.05, vary_length=True)
    reads += special
    order = rng.permutation(n)
    reads = [reads[i] for i in order]
    if not paired:
        return reads, None
    mates = synth.make_reads(lib, n, rng, length=100, n_single=0.1, vary_length=True, short=0.05)
    at = {int(np.nonzero(order == n - len(special) + j)[0][0]): j for j in range(len(special))}
    for i, j in at.items():
        mates[i] = np.zeros(0, np.uint8) if j in (0, 4) else mates[i]       # an empty pair; 1000 + 0 bases: still taken
    # a pair whose mates are each short enough and together too long, and one of exactly 1000
    free = [i for i in range(n) if i not in at]
    reads[free[0]], mates[free[0]] = acgt(600), acgt(401)
    reads[free[1]], mates[free[1]] = acgt(600), acgt(400)
    return reads, mates


_sets = {}


def read_sets(W, name, paired):
    """(the main set: R = 64 T + 1; R = 65; R = 1), made once per world so that the oracle's view of them is computed once"""
    key = (name, paired)
    if key not in _sets:
        rng = np.random.default_rng(1000 + 7 * paired + (name == "w10"))
        big = edge_reads(W, rng, 64 * 14 + 1, paired)
        r65 = edge_reads(W, rng, 65, paired)
        one = synth.make_reads(W.lib, 1, rng, length=140, short=0)
        _sets[key] = (big, r65, (one, synth.make_reads(W.lib, 1, rng, length=90, short=0) if paired else None))
    return _sets[key]


@pytest.mark.parametrize("hits", [False, True], ids=["rows", "hitlists"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("n_shards", [1, 2, 3, 5, 8, 16, 64])
@pytest.mark.parametrize("name", ["w5", "w10"])
def test_owner_counts(worlds, name, n_shards, paired, hits):
    """All four chunk sizes (1024, 512, 256 twice, 128, 64), a count that is no power of two, an owner for every lane; both scans
    (w = 5 and van Herk); empty, short, all-N, 1000- and 1001-base fragments, pairs that are too long only together; a last tile of
    one lane (R = 64 T + 1, R = 65) and a batch of one fragment."""
    W = worlds(name)
    for reads, mates in read_sets(W, name, paired):
        b = Batch(W, reads, mates, n_shards, hits)
        assert (~b.m["taken"]).sum() >= (0 if b.R == 1 else 1)
        through(b)


def mixed_keys(W, n, rng):
    """present records, absent keys and zeros"""
    lib = W.lib
    keys = lib.keys[rng.integers(0, len(lib.keys), n)].copy()
    kind = rng.integers(0, 3, n)
    absent = (rng.integers(0, 2**62, n, dtype=np.int64) << 1) & np.int64(np.uint64(W.p.space[0]).astype(np.int64))
    keys[kind == 1] = absent[kind == 1]
    keys[kind == 2] = 0
    return keys


def test_lookup_dealing(worlds):
    """The LOOKUP job inside a scan of T tiles: fewer keys than one batch, exactly one, a last batch of 1, 63 and 7 keys, a share per
    tile that rounds up (the last tiles own batches beyond the end), a share at the very limit of what rides, and one beyond it,
    which runs beside the scan.  The answers are orc.Index.lookup's, nothing is written beyond n, and the EMIT the lookups ride in
    keeps its contract."""
    W = worlds("w5")
    rng = np.random.default_rng(31)
    T = 6
    reads = synth.make_reads(W.lib, 64 * T - 3, rng, n_single=0.1)
    b = Batch(W, reads, None, 3)
    # the limit of laneplan.h (shard_side_per_tile): per_tile <= 3 * own + 8 with own = 2 / (w + 1) * bases / 64 / tiles
    own = 2.0 / (W.w + 1) * b.total / 64.0 / T
    most = int(3.0 * own + 8.0)
    rides = 5
    assert rides + 1 <= most
    sizes = [1, 63, 64, 65, 64 * T - 1, 64 * T + 1, 64 * (T * rides) + 7, 64 * T * most, 64 * T * most + 1, 64 * T * (most + 1)]
    per_tile = [(-(-n // 64) + T - 1) // T for n in sizes]
    assert per_tile[6] == rides + 1 and per_tile[6] * T > -(-sizes[6] // 64)       # rounds up: batches beyond the end are owned
    assert per_tile[7] == most and per_tile[8] == most + 1 and per_tile[9] == most + 1   # the last to ride, the first two beside
    for n in sizes:
        keys = mixed_keys(W, n, rng)
        d_keys = torch.from_numpy(keys).to(DEV)
        d_out = _full(n + 256, TAXA_SENT, torch.int32)
        b.sentinels()
        step(W, emit=b, lookup=capi.ShardLookup(d_keys.data_ptr(), n, d_out.data_ptr()))
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:n], W.lookup(keys)), n
        assert (got[n:] == TAXA_SENT).all(), n
        check_emit(b)
    owners_answer(b)
    step(W, apply=b)
    check_apply(b)


def test_three_batches_in_one_launch(worlds):
    """Step t carries EMIT(t), LOOKUP(t - 1) and APPLY(t - 2), as the pipeline's steps do (there with the exchanges in between):
    an applied batch larger than the scanned one and the reverse, a batch of R = 0 in every role, LOOKUP + APPLY without a scan, a
    LOOKUP alone, an APPLY alone."""
    W = worlds("w5")
    rng = np.random.default_rng(32)
    sizes = [2500, 700, 1300, 0, 3000]
    bs = [Batch(W, synth.make_reads(W.lib, n, rng, n_single=0.1, n_run=0.05, vary_length=True) +
                (synth.make_reads(W.lib, 3, rng, length=1200, short=0) if i == 2 else []), None, 3) for i, n in enumerate(sizes)]
    addr = {}
    for t in range(len(bs) + 2):
        e = bs[t] if t < len(bs) else None
        lk = bs[t - 1] if 0 <= t - 1 < len(bs) else None
        ap = bs[t - 2] if 0 <= t - 2 < len(bs) else None
        if e is not None:
            e.sentinels()
        step(W, emit=e, lookup=lk.lookup_job() if lk is not None else None, apply=ap)
        if e is not None:
            addr[t] = check_emit(e)
        if lk is not None:
            check_answers(lk, addr[t - 1])
        if ap is not None:
            check_apply(ap)
    # LOOKUP + APPLY of two batches with no EMIT in the call at all (the pipeline's drain)
    X, Y = bs[1], bs[2]
    for b in (X, Y):
        b.sentinels()
        step(W, emit=b)
        addr[id(b)] = check_emit(b)
    owners_answer(X)
    step(W, lookup=Y.lookup_job(), apply=X)
    check_answers(Y, addr[id(Y)])
    check_apply(X)
    step(W, apply=Y)
    check_apply(Y)


def test_three_batches_with_hit_lists(worlds):
    """the same three jobs in one launch, pairs, hit lists written by all of them"""
    W = worlds("w5")
    rng = np.random.default_rng(33)
    bs = []
    for n in (500, 900, 300):
        reads, mates = edge_reads(W, rng, n, True)
        bs.append(Batch(W, reads, mates, 5, True))
    addr = {}
    for t in range(len(bs) + 2):
        e = bs[t] if t < len(bs) else None
        lk = bs[t - 1] if 0 <= t - 1 < len(bs) else None
        ap = bs[t - 2] if 0 <= t - 2 < len(bs) else None
        if e is not None:
            e.sentinels()
        step(W, emit=e, lookup=lk.lookup_job() if lk is not None else None, apply=ap)
        if e is not None:
            addr[t] = check_emit(e)
        if lk is not None:
            check_answers(lk, addr[t - 1])
        if ap is not None:
            check_apply(ap)


def expect_full_region(W, **jobs):
    with pytest.raises(slacken_amd.SlackenError) as e:
        step(W, **jobs)
    assert e.value.code == capi.E_CAPACITY and "send region" in str(e.value), str(e.value)   # (and no other error bit: its own message)


@pytest.mark.parametrize("n_shards,hits", [(1, False), (2, True), (8, False)])
def test_full_region_is_reported_and_recoverable(worlds, n_shards, hits):
    """Regions of ONE chunk for a batch that has more keys than that for some owner (counted from the oracle's spans before the
    launch): slk_stream_synchronize says SLK_E_CAPACITY, the owner's cursor is beyond the capacity, every region still holds only
    its own keys and zeros, from the front, the guard is untouched.  Then the same batch again on the same stream and buffers with
    regions that cannot overflow: the whole pipeline equals the oracle (which is also the check that nothing overflows falsely)."""
    W = worlds("w5")
    rng = np.random.default_rng(34 + n_shards)
    reads = synth.make_reads(W.lib, 700, rng, n_single=0.1, vary_length=True)
    b = Batch(W, reads, None, n_shards, hits)
    assert b.keys_g.max() > b.chunk
    b.sentinels(cap=b.chunk)
    expect_full_region(W, emit=b)
    check_emit(b, overflowed=True)
    W.st.synchronize()                       # the error was reported once; the stream is usable
    b.cap = b.safe_cap
    through(b)


def test_a_capacity_the_chunks_do_not_fill_exactly_is_refused(worlds):
    """Cursors advance by whole chunks, so "the next chunk fits" and "the region is not full yet" are one test only while
    capacity_per_owner is a multiple of slk_shard_chunk(n_shards): anything else is SLK_E_INVALID before a kernel is launched, as are
    owner counts outside 1..64 -- and the lists are untouched."""
    W = worlds("w5")
    rng = np.random.default_rng(37)
    for n in (1, 8, 64):
        b = Batch(W, synth.make_reads(W.lib, 100, rng), None, n)
        for cap in (b.chunk - 1, b.chunk + 1, b.safe_cap + b.chunk // 2, 0, 1 << 32):
            b.sentinels(cap=cap)
            with pytest.raises(slacken_amd.SlackenError) as e:
                step(W, emit=b)
            assert e.value.code == capi.E_INVALID, (n, cap)
            h = b.fetch()
            assert (h["send_keys"] == KEY_SENT).all() and (h["cursors"] == 0x77).all() and (h["log"] == WORD_SENT).all()
    b = Batch(W, synth.make_reads(W.lib, 10, rng), None, 64)
    for n in (0, 65):
        b.n = n
        with pytest.raises(slacken_amd.SlackenError) as e:
            step(W, emit=b)
        assert e.value.code == capi.E_INVALID, n
    W.st.synchronize()


def test_full_region_beside_two_healthy_batches(worlds):
    """the overflow inside a step that also answers batch B's keys and applies batch A: both are exact all the same"""
    W = worlds("w5")
    rng = np.random.default_rng(35)
    mk = lambda n: synth.make_reads(W.lib, n, rng, n_single=0.1, vary_length=True)
    A, B, Cb = Batch(W, mk(900), None, 2), Batch(W, mk(400), None, 2), Batch(W, mk(600), None, 2)
    A.sentinels()
    step(W, emit=A)
    a_addr = check_emit(A)
    B.sentinels()
    step(W, emit=B, lookup=A.lookup_job())
    b_addr = check_emit(B)
    check_answers(A, a_addr)
    assert Cb.keys_g.max() > Cb.chunk
    Cb.sentinels(cap=Cb.chunk)
    expect_full_region(W, emit=Cb, lookup=B.lookup_job(), apply=A)
    check_emit(Cb, overflowed=True)
    check_answers(B, b_addr)
    check_apply(A)
    # emitted again with larger regions, the batch goes on through the pipeline
    Cb.sentinels(cap=Cb.safe_cap)
    step(W, emit=Cb, apply=B)
    c_addr = check_emit(Cb)
    check_apply(B)
    step(W, lookup=Cb.lookup_job())
    check_answers(Cb, c_addr)
    step(W, apply=Cb)
    check_apply(Cb)


def test_pipeline_sends_an_overflowed_batch_through_the_staged_route(worlds, monkeypatch):
    """ShardedClassifier.classify_many, world = 1: the regions of the third batch of five are one chunk -- that batch comes back
    through the staged route (deferred == R), and all five equal the oracle"""
    from slacken_amd import sharded
    W = worlds("w5")
    rng = np.random.default_rng(36)
    sets = [synth.make_reads(W.lib, n, rng, n_single=0.1, vary_length=True) for n in (600, 900, 700, 300, 800)]
    packed = [synth.pack(r) for r in sets]
    dbs = [(torch.from_numpy(b).to(DEV), torch.from_numpy(o.astype(np.int64)).to(DEV), len(o) - 1, int(o[-1]), None) for b, o in packed]
    calls = []
    real = sharded.ShardedClassifier._region_capacity

    def small_third(self, total_bases, R):
        calls.append(R)
        return int(slacken_amd.lib().slk_shard_chunk(1)) if len(calls) == 3 else real(self, total_bases, R)
    monkeypatch.setattr(sharded.ShardedClassifier, "_region_capacity", small_third)
    sc = sharded.ShardedClassifier(W.ix, 0, 1, None, DEV)
    try:
        outs = sc.classify_many(dbs, thresholds=THR)
        assert calls == [len(r) for r in sets]
        for i, (o, (b, off)) in enumerate(zip(outs, packed)):
            R = len(sets[i])
            assert o["deferred"] == (R if i == 2 else 0), i
            want = W.orc.classify_batch(W.p, W.oix, W.parents, b, off, thresholds=THR)
            assert np.array_equal(o["taxon"].cpu().numpy().reshape(len(THR), -1)[:, :R], want["taxon"]), i
            assert np.array_equal(o["classified"].cpu().numpy().reshape(len(THR), -1)[:, :R], want["classified"]), i
            for k in ("num_distinct", "total_kmers", "num_hits"):
                assert np.array_equal(o[k].cpu().numpy()[:R], want[k]), (i, k)
        del outs, o
    finally:
        sc.close()


# ---- persistent waves ---------------------------------------------------------------------------------------------------------------

def short_reads(lib, R, rng, lo=36, hi=70):
    """R fragments of lo..hi bases cut from the library's genomes (a fifth random, a few N), without a Python loop"""
    G = np.concatenate(lib.genomes)
    lens = rng.integers(lo, hi + 1, R)
    offsets = np.zeros(R + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    start = rng.integers(0, len(G) - hi, R)
    total = int(offsets[-1])
    bases = G[np.repeat(start - offsets[:-1], lens) + np.arange(total)].copy()
    rnd = np.repeat(rng.random(R) < 0.2, lens)
    bases[rnd] = synth.ACGT[rng.integers(0, 4, int(rnd.sum()))]
    bases[rng.random(total) < 0.002] = ord("N")
    return np.split(bases, offsets[1:-1])


def _persistent_child():
    """(in a process of its own, SLK_STEP_BLOCKS_PER_CU=1: CUs x 4 waves) a batch of at least three tiles per wave: the waves draw
    tiles from cursors[n_shards] and carry their chunks from tile to tile; a LOOKUP rides in the EMIT; then the rest of the pipeline"""
    from oracle import oracle as orc
    assert os.environ.get("SLK_STEP_BLOCKS_PER_CU") == "1"
    W = World(orc)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = cus * 4
    tiles = 3 * waves
    R = 64 * (tiles - 1) + 1
    rng = np.random.default_rng(51)
    reads = short_reads(W.lib, R, rng)
    report = dict(cus=cus, waves=waves, tiles=tiles, R=R, bases=int(sum(len(r) for r in reads)))
    for n in (2, 8):
        b = Batch(W, reads, None, n)
        assert b.tiles == tiles >= 3 * cus * 4
        nk = 64 * (tiles * 2) + 7                       # three batches a tile, the last tiles' beyond the end: rides (3 <= 3 * own + 8)
        keys = mixed_keys(W, nk, rng)
        d_keys = torch.from_numpy(keys).to(DEV)
        d_out = _full(nk + 256, TAXA_SENT, torch.int32)
        b.sentinels()
        step(W, emit=b, lookup=capi.ShardLookup(d_keys.data_ptr(), nk, d_out.data_ptr()))
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:nk], W.lookup(keys)) and (got[nk:] == TAXA_SENT).all()
        addr = check_emit(b)
        cur = b.h["cursors"]
        draws = int(cur[n])
        assert draws >= tiles - waves > 0, (draws, tiles, waves)                     # tiles were drawn from the counter
        # a wave reserves a chunk only when the one it carries is full: whatever is reserved beyond the keys is at most the one
        # part-filled chunk per wave and owner (reserved afresh per tile it would be up to one per TILE)
        assert (cur[:n] <= b.keys_g + b.chunk * waves).all(), (cur[:n].tolist(), b.keys_g.tolist(), b.chunk, waves)
        owners_answer(b)
        check_answers(b, addr)
        step(W, apply=b)
        check_apply(b)
        report[f"n{n}"] = dict(draws=draws, cursors=[int(c) for c in cur[:n]], keys=[int(k) for k in b.keys_g], chunk=b.chunk)
    W.st.close()
    W.ix.close()
    print("STEP-REPORT " + json.dumps(report), flush=True)


def test_persistent_waves_draw_tiles_and_carry_their_chunks():
    """One resident block per CU (SLK_STEP_BLOCKS_PER_CU is read once per process: hence the child) and three tiles per wave -- about
    200 000 fragments of 36..70 bases on 256 CUs: the tile draw, the chunk carried from tile to tile and the LOOKUP batches dealt
    to DRAWN tiles all run, for n_shards = 2 and 8, under every check of this file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys\nsys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})\n"
            "import torch\nimport test_gpu_shard_step as T\nT._persistent_child()\n")
    env = dict(os.environ, SLK_STEP_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)   # (the timeout: a hang guard)
    assert r.returncode == 0 and "STEP-REPORT" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(r.stdout.split("STEP-REPORT ", 1)[1].splitlines()[0])
    print("persistent waves:", rep)
    assert rep["tiles"] >= 3 * rep["waves"] and rep["n2"]["draws"] >= rep["tiles"] - rep["waves"]
