"""A numpy model of the lists the table-sharded step kernel leaves behind (slk_shard_step_device), written from the contract in
include/slacken_amd.h (slk_shard_lists) and slacken_amd/csrc/engine.h (ShardIO, ApplyJob) -- not from the kernel.  Two halves:

  expected_sends   what an EMIT has to queue, from the ORACLE's spans of every fragment;
  replay           what the lists an EMIT wrote actually say, walked the way the APPLY is documented to walk them.

Test infrastructure (numpy + the oracle's ctypes binding); exact integers throughout."""
import ctypes as C

import numpy as np

MAX_FAST_BASES = 1000          # the fast route takes fragments of up to 1000 bases, both mates together (slacken_amd.h)
NO_CHUNK = 0xFFFFFFFF          # `fresh` of a log entry whose owner's region was full: the keys beyond `room` were dropped
SEND = np.dtype([("frag", "<i8"), ("ordinal", "<i4"), ("key", "<i8"), ("kmers", "<i4"), ("distinct", "<i4")])
_SPAN = np.dtype([("key", "<u8", (4,)), ("kmers", "<i4"), ("flag", "<i4"), ("ordinal", "<i4"), ("distinct", "<i4")])


def shard_of(keys, n_shards):
    """slk_shard_of on an int64 array: fmix64(key) mod n_shards, unsigned"""
    x = np.ascontiguousarray(keys, np.int64).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return (x % np.uint64(n_shards)).astype(np.int64)


def chunk_of(n_shards):
    """slk_shard_chunk: 1024 entries shared out over the owners, never below 64"""
    c = 1024
    while c > 64 and c * n_shards > 1024:
        c >>= 1
    return c


def sort_sends(a):
    """canonical order of a SEND array: by fragment, then ordinal, then the rest -- equal arrays <=> equal multisets per fragment"""
    return a[np.lexsort((a["distinct"], a["kmers"], a["key"], a["ordinal"], a["frag"]))]


def expected_sends(orc, p, reads, mates, n_shards):
    """-> (sends, owner, read_info, taken)

    sends      SEND array, sorted (sort_sends): one row per span that travels, of every fragment the fast route takes (at most 1000
               bases, both mates together): (fragment, ordinal, key, kmers, distinct) exactly as orc.spans gives them;
    owner      slk_shard_of(key, n_shards) of every row;
    read_info  [R, 2] = (total k-mers, spans) of every taken fragment, zeros for the others;
    taken      [R] bool: False for the fragments longer than 1000 bases (the EMIT flags them in d_defer and sends nothing).

    Which spans travel: the SEQUENCE_FLAG spans only -- the super-mers of Supermers.spans that carry a minimizer and are joined
    with the records (KeyValueIndex.getSpans / spanToHit).  The AMBIGUOUS_FLAG spans (runs of non-ACGT of at least k characters) and
    the MATE_PAIR_BORDER pseudo-span have no key: the EMIT keeps them on its rank (with hit lists, in d_span_meta / d_span_taxon),
    but they COUNT: `ordinal` numbers all spans of the fragment, `spans` of read_info is the number of all of them (the "no span, no
    row" test) and `total k-mers` sums the k-mers of all but the border (TaxonCounts.totalKmers)."""
    L = orc.lib()
    R = len(reads)
    cap = 2 * MAX_FAST_BASES + 8
    buf = (orc.Span * cap)()
    addr, pp = C.addressof(buf), C.byref(p)
    raw, count = [], np.zeros(R, np.int64)
    taken = np.ones(R, bool)
    for r in range(R):
        s1 = reads[r].tobytes()
        s2 = mates[r].tobytes() if mates is not None else None
        if len(s1) + (len(s2) if s2 is not None else 0) > MAX_FAST_BASES:
            taken[r] = False
            continue
        n = L.orc_spans(pp, s1, len(s1), s2, len(s2) if s2 is not None else 0, buf, cap)
        if n < 0:
            raise ValueError(f"orc_spans failed: {n}")
        count[r] = n
        raw.append(C.string_at(addr, n * _SPAN.itemsize))
    sp = np.frombuffer(b"".join(raw), dtype=_SPAN)
    frag = np.repeat(np.arange(R, dtype=np.int64), count)
    read_info = np.zeros((R, 2), np.int32)
    read_info[:, 0] = np.bincount(frag, weights=np.where(sp["flag"] != orc.MATE_PAIR_BORDER_FLAG, sp["kmers"], 0), minlength=R)
    read_info[:, 1] = count
    seq = sp["flag"] == orc.SEQUENCE_FLAG
    sends = np.zeros(int(seq.sum()), SEND)
    sends["frag"] = frag[seq]
    sends["ordinal"] = sp["ordinal"][seq]
    sends["key"] = sp["key"][seq, 0].view(np.int64) if seq.any() else 0
    sends["kmers"] = sp["kmers"][seq]
    sends["distinct"] = sp["distinct"][seq]
    sends = sort_sends(sends)
    return sends, shard_of(sends["key"], n_shards), read_info, taken


def replay(log, tile_rows, send_keys, send_meta, cursors, cap, n_shards, R):
    """Walk the probe log the way the APPLY is documented to (engine.h: ShardIO.batch_log, slacken_amd.h: slk_shard_lists).

    log [rows, n_shards, 4] uint32, tile_rows [tiles, 2] uint32 ({first row, rows} of every tile of 64 fragments), send_keys int64 and
    send_meta uint32 [n_shards * cap (or longer)], cursors [>= n_shards].  For row rho of tile t and owner g the entry
    {pos, fresh, cnt, room} says: key i of the group sits at g * cap + (pos + i if i < room else fresh + i - room).  A group whose
    `fresh` is NO_CHUNK found its region full: its keys from `room` on were dropped (counted in `dropped`).

    -> (sends, addressed, owner_of, dropped, beyond): SEND array sorted as expected_sends' (fragment = tile * 64 + (meta & 63), kmers
    = (meta >> 7) & 0x1FFF, distinct = (meta >> 6) & 1, ordinal = meta >> 20); the addressed positions (indices into send_keys, in
    walk order, NOT made unique); the owner whose region each lies in; the number of dropped keys; the number of addressed
    positions at or beyond min(cursors[g], cap) of their owner, i.e. outside what travels."""
    log = np.asarray(log, np.uint32).reshape(-1, n_shards, 4)
    tile_rows = np.asarray(tile_rows, np.uint32).reshape(-1, 2)
    tiles = (R + 63) // 64
    assert len(tile_rows) >= tiles
    first, used = tile_rows[:tiles, 0].astype(np.int64), tile_rows[:tiles, 1].astype(np.int64)
    tile_of_row = np.repeat(np.arange(tiles, dtype=np.int64), used)
    rows = np.repeat(first, used) + (np.arange(int(used.sum()), dtype=np.int64) - np.repeat(np.cumsum(used) - used, used))
    assert rows.size == 0 or int(rows.max()) < len(log), "a tile's rows lie beyond the log"
    E = log[rows].astype(np.int64).reshape(-1, 4)                     # [(row, owner)] entries in walk order
    owner = np.tile(np.arange(n_shards, dtype=np.int64), len(rows))
    tile = np.repeat(tile_of_row, n_shards)
    pos, fresh, cnt, room = E[:, 0], E[:, 1], E[:, 2], E[:, 3]
    assert cnt.size == 0 or int(cnt.max()) <= 64, "a probe batch holds at most 64 keys"
    i = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    g = np.repeat(owner, cnt)
    t = np.repeat(tile, cnt)
    in_old = i < np.repeat(room, cnt)
    at = np.where(in_old, np.repeat(pos, cnt) + i, np.repeat(fresh, cnt) + i - np.repeat(room, cnt))
    lost = ~in_old & (np.repeat(fresh, cnt) == NO_CHUNK)
    dropped = int(lost.sum())
    at, g, t = at[~lost], g[~lost], t[~lost]
    assert at.size == 0 or (int(at.min()) >= 0 and int(at.max()) < cap), "the log addresses a position outside its owner's region"
    addressed = g * cap + at
    beyond = int((at >= np.minimum(np.asarray(cursors).astype(np.int64)[:n_shards], cap)[g]).sum())
    meta = np.asarray(send_meta).view(np.uint32)[addressed].astype(np.int64)
    sends = np.zeros(len(addressed), SEND)
    sends["frag"] = t * 64 + (meta & 63)
    sends["key"] = np.asarray(send_keys).view(np.int64)[addressed]
    sends["kmers"] = (meta >> 7) & 0x1FFF
    sends["distinct"] = (meta >> 6) & 1
    sends["ordinal"] = meta >> 20
    order = np.lexsort((sends["distinct"], sends["kmers"], sends["key"], sends["ordinal"], sends["frag"]))
    return sends[order], addressed, g, dropped, beyond
