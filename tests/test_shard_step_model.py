"""The numpy model of the sharded step's lists (shard_step_model.py) on hand-made logs and on the oracle's spans: the model itself
is checked here, on the CPU, before tests/test_gpu_shard_step.py holds the kernel against it."""
import numpy as np
import pytest

import shard_step_model as M

SENT = 0x5A5A5A5A5A5A5A5B


def _meta(lane, kmers, distinct, ordinal):
    return lane | (distinct << 6) | (kmers << 7) | (ordinal << 20)


def _lists(n_shards, cap, rows, tiles):
    keys = np.full(n_shards * cap, SENT, np.int64)
    meta = np.full(n_shards * cap, 0xFFFFFFFF, np.uint32)
    log = np.full((rows, n_shards, 4), 0xEEEEEEEE, np.uint32)
    tr = np.full((tiles, 2), 0xEEEEEEEE, np.uint32)
    return keys, meta, log, tr


def _put(keys, meta, at, key, lane, kmers, distinct, ordinal):
    keys[at], meta[at] = key, _meta(lane, kmers, distinct, ordinal)


def _tuples(sends):
    return [tuple(int(x) for x in row) for row in sends[["frag", "ordinal", "key", "kmers", "distinct"]].tolist()]


def test_a_group_that_fits_its_chunk():
    keys, meta, log, tr = _lists(1, 128, 4, 1)
    tr[0] = (2, 1)                                   # the tile's one row is row 2 of the log
    log[2, 0] = (5, M.NO_CHUNK, 3, 123)              # three keys at 5, 6, 7: plenty of room, no fresh chunk
    _put(keys, meta, 5, 1000, lane=9, kmers=4, distinct=1, ordinal=0)
    _put(keys, meta, 6, 2000, lane=9, kmers=1, distinct=0, ordinal=2)
    _put(keys, meta, 7, 3000, lane=63, kmers=966, distinct=1, ordinal=999)
    sends, addressed, owner, dropped, beyond = M.replay(log, tr, keys, meta, [128], 128, 1, 64)
    assert _tuples(sends) == [(9, 0, 1000, 4, 1), (9, 2, 2000, 1, 0), (63, 999, 3000, 966, 1)]
    assert addressed.tolist() == [5, 6, 7] and owner.tolist() == [0, 0, 0] and dropped == 0 and beyond == 0


def test_a_group_that_straddles_into_a_fresh_chunk():
    cap = 256
    keys, meta, log, tr = _lists(2, cap, 3, 1)
    tr[0] = (0, 1)
    log[0, 0] = (0, M.NO_CHUNK, 0, 0)                # owner 0: nothing in this batch
    log[0, 1] = (126, 192, 5, 2)                     # owner 1: two keys end the old chunk (126, 127), three open the one at 192
    for i, at in enumerate([126, 127, 192, 193, 194]):
        _put(keys, meta, cap + at, 10 + i, lane=i, kmers=i + 1, distinct=i & 1, ordinal=i)
    sends, addressed, owner, dropped, beyond = M.replay(log, tr, keys, meta, [0, 256], cap, 2, 5)
    assert addressed.tolist() == [cap + 126, cap + 127, cap + 192, cap + 193, cap + 194]
    assert owner.tolist() == [1] * 5 and dropped == 0 and beyond == 0
    assert _tuples(sends) == [(i, i, 10 + i, i + 1, i & 1) for i in range(5)]
    # the same entry with room for all five: they lie in a row
    log[0, 1] = (126, M.NO_CHUNK, 5, 5)
    assert M.replay(log, tr, keys, meta, [0, 256], cap, 2, 5)[1].tolist() == [cap + 126 + i for i in range(5)]
    # ... and with none left (room == 0): all of them in the fresh chunk
    log[0, 1] = (128, 192, 5, 0)
    assert M.replay(log, tr, keys, meta, [0, 256], cap, 2, 5)[1].tolist() == [cap + 192 + i for i in range(5)]


def test_empty_groups_and_empty_tiles_address_nothing():
    keys, meta, log, tr = _lists(3, 128, 4, 2)
    tr[0] = (0, 2)
    tr[1] = (3, 0)                                   # a tile that sent nothing: no rows
    log[0] = [(0, M.NO_CHUNK, 0, 0), (0, 0, 1, 0), (7, M.NO_CHUNK, 0, 121)]
    log[1] = [(0, M.NO_CHUNK, 0, 0), (1, M.NO_CHUNK, 0, 127), (7, M.NO_CHUNK, 0, 121)]
    _put(keys, meta, 128, 77, lane=3, kmers=2, distinct=1, ordinal=1)
    sends, addressed, owner, dropped, beyond = M.replay(log, tr, keys, meta, [0, 128, 128], 128, 3, 128)
    assert addressed.tolist() == [128] and owner.tolist() == [1] and dropped == 0 and beyond == 0
    assert _tuples(sends) == [(3, 1, 77, 2, 1)]


def test_two_tiles_number_their_fragments_apart():
    keys, meta, log, tr = _lists(2, 128, 8, 2)
    tr[0] = (0, 1)
    tr[1] = (5, 2)                                   # (rows of different tiles need not be adjacent)
    log[0] = [(0, 0, 2, 0), (0, 0, 1, 0)]
    log[5] = [(2, M.NO_CHUNK, 1, 126), (1, M.NO_CHUNK, 2, 127)]
    log[6] = [(3, M.NO_CHUNK, 0, 125), (3, M.NO_CHUNK, 1, 125)]
    _put(keys, meta, 0, 100, lane=0, kmers=1, distinct=1, ordinal=0)
    _put(keys, meta, 1, 101, lane=1, kmers=1, distinct=1, ordinal=0)
    _put(keys, meta, 128 + 0, 200, lane=0, kmers=2, distinct=1, ordinal=1)
    _put(keys, meta, 2, 102, lane=0, kmers=3, distinct=1, ordinal=0)            # tile 1: fragment 64
    _put(keys, meta, 128 + 1, 201, lane=5, kmers=1, distinct=1, ordinal=0)      # tile 1: fragment 69
    _put(keys, meta, 128 + 2, 202, lane=5, kmers=1, distinct=0, ordinal=1)
    _put(keys, meta, 128 + 3, 203, lane=0, kmers=1, distinct=1, ordinal=1)
    sends, addressed, owner, dropped, beyond = M.replay(log, tr, keys, meta, [64, 64], 128, 2, 70)
    assert sorted(addressed.tolist()) == [0, 1, 2, 128, 129, 130, 131] and len(set(addressed.tolist())) == 7
    assert dropped == 0 and beyond == 0
    assert _tuples(sends) == [(0, 0, 100, 1, 1), (0, 1, 200, 2, 1), (1, 0, 101, 1, 1),
                              (64, 0, 102, 3, 1), (64, 1, 203, 1, 1), (69, 0, 201, 1, 1), (69, 1, 202, 1, 0)]
    # a cursor that stops short of what the log addresses is reported
    assert M.replay(log, tr, keys, meta, [2, 64], 128, 2, 70)[4] == 1


def test_a_full_region_drops_the_keys_beyond_the_room():
    keys, meta, log, tr = _lists(1, 64, 2, 1)
    tr[0] = (0, 2)
    log[0, 0] = (60, M.NO_CHUNK, 7, 4)               # four keys fit, three found no chunk
    log[1, 0] = (0, M.NO_CHUNK, 9, 0)                # the wave holds no chunk any more: all nine dropped
    for i in range(4):
        _put(keys, meta, 60 + i, 500 + i, lane=i, kmers=1, distinct=1, ordinal=0)
    sends, addressed, owner, dropped, beyond = M.replay(log, tr, keys, meta, [128], 64, 1, 64)
    assert addressed.tolist() == [60, 61, 62, 63] and dropped == 12 and beyond == 0
    assert [t[2] for t in _tuples(sends)] == [500, 501, 502, 503]


def test_a_log_that_points_outside_its_region_is_refused():
    keys, meta, log, tr = _lists(1, 64, 1, 1)
    tr[0] = (0, 1)
    log[0, 0] = (62, M.NO_CHUNK, 3, 3)
    with pytest.raises(AssertionError):
        M.replay(log, tr, keys, meta, [64], 64, 1, 64)


def test_chunk_and_owner_agree_with_the_library():
    import slacken_amd
    L = slacken_amd.lib()
    rng = np.random.default_rng(11)
    keys = rng.integers(-2**63, 2**63 - 1, 2000, dtype=np.int64)
    for n in (1, 2, 3, 4, 5, 8, 15, 16, 17, 63, 64):
        assert M.chunk_of(n) == L.slk_shard_chunk(n)
        assert np.array_equal(M.shard_of(keys, n), np.array([L.slk_shard_of(int(k), n) for k in keys]))
    assert {M.chunk_of(n) for n in (1, 2, 3, 5, 8, 16, 64)} == {1024, 512, 256, 128, 64}


def test_expected_sends_are_the_oracles_sequence_spans(orc):
    p = orc.params()
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    dna = lambda n: acgt[rng.integers(0, 4, n)]
    n_run = dna(200)
    n_run[60:110] = ord("N")                          # an AMBIGUOUS span of 50 - 34 k-mers between two sequence runs
    reads = [dna(150), np.zeros(0, np.uint8), dna(20), np.full(80, ord("N"), np.uint8), dna(1000), dna(1001), n_run, dna(600)]
    mates = [dna(100), dna(50), np.zeros(0, np.uint8), dna(40), np.zeros(0, np.uint8), np.zeros(0, np.uint8), dna(90), dna(401)]
    for mm in (None, mates):
        sends, owner, info, taken = M.expected_sends(orc, p, reads, mm, 5)
        assert taken.tolist() == [True] * 5 + [False, True, mm is None]
        assert np.array_equal(owner, M.shard_of(sends["key"], 5))
        for r in range(len(reads)):
            mine = sends[sends["frag"] == r]
            if not taken[r]:
                assert len(mine) == 0 and info[r].tolist() == [0, 0]
                continue
            sp = orc.spans(p, reads[r].tobytes(), mm[r].tobytes() if mm is not None else None)
            seq = [s for s in sp if s["flag"] == orc.SEQUENCE_FLAG]
            assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in mine[["ordinal", "key", "kmers", "distinct"]].tolist()] == \
                [(s["ordinal"], np.uint64(s["key"][0]).astype(np.int64), s["kmers"], int(s["distinct"])) for s in seq]
            assert info[r, 1] == len(sp)
            assert info[r, 0] == sum(s["kmers"] for s in sp if s["flag"] != orc.MATE_PAIR_BORDER_FLAG)
        # the figures the oracle's classification reports are the same ones
        b1, o1 = _pack(reads)
        args = (b1, o1) + (_pack(mm) if mm is not None else ())
        ix = orc.Index(1, np.zeros(0, np.int64), np.zeros(0, np.int32))
        want = orc.classify_batch(p, ix, np.array([0, 1], np.int32), *args)
        assert np.array_equal(info[taken, 0], want["total_kmers"][taken])
        assert np.array_equal(info[taken, 1], want["num_hits"][taken])
    amb = orc.spans(p, n_run.tobytes())
    assert [s["flag"] for s in amb].count(orc.AMBIGUOUS_FLAG) == 1


def _pack(reads):
    import synth
    return synth.pack(reads)
