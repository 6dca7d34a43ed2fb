"""The model of library merging: records folded per key with the oracle's LCA, the translation of a source's taxa
into the destination's taxonomy, and the generator of the sequences the merge tests share -- genomes with common segments, so that
the parts of a split hold many of the same minimizers under different taxa."""
from collections import namedtuple

import numpy as np

import synth
import taxgen
from oracle import oracle as orc

# a taxonomy as the model reads it: parents[] (0 = undefined, ROOT = 1) and the (old, new) pairs of its merged.dmp
Tax = namedtuple("Tax", ["parents", "merged"], defaults=[()])


def is_defined(parents, t):
    return 1 <= t < len(parents) and (t == 1 or parents[t] != 0)


def taxon_remap(src_tax, dst_tax):
    """(map, identity): map[t] for every node t src defines = dst's primary of t if dst defines that node, else 0; identity: the map
    changes no node of src.  Restates slacken_amd/host/merge.hpp."""
    primary = dict(getattr(dst_tax, "merged", ()) or ())
    out = np.zeros(len(src_tax.parents), np.int32)
    identity = True
    for t in range(1, len(src_tax.parents)):
        if not is_defined(src_tax.parents, t):
            continue
        p = primary.get(t, t)
        out[t] = p if is_defined(dst_tax.parents, p) else 0   # (also: an id beyond dst's array)
        identity = identity and out[t] == t
    return out, identity


def merge(parents, sources, remaps=None):
    """sources: (keys, taxa) pairs -> dict key -> taxon: per key the LCA (orc.lca) of every taxon that arrives for it.  Taxon 0 is
    skipped; remaps[i] (or None) translates source i's taxa first; a taxon that is then no defined node of `parents` is dropped."""
    parents = np.ascontiguousarray(parents, np.int32)
    out = {}
    for i, (keys, taxa) in enumerate(sources):
        rm = remaps[i] if remaps is not None else None
        for k, t in zip(np.asarray(keys).tolist(), np.asarray(taxa).tolist()):
            if t == 0:
                continue
            if rm is not None:
                t = int(rm[t]) if 0 <= t < len(rm) else 0
            if not is_defined(parents, t):
                continue
            have = out.get(k)
            out[k] = t if have is None or have == t else orc.lca(parents, have, t)
    return out


def refused(parents, keys, taxa, remap=None):
    """the source taxa (before the remap) of the records merge() drops, taxon 0 aside"""
    bad = []
    for t in np.asarray(taxa).tolist():
        x = t if remap is None or t <= 0 else (int(remap[t]) if t < len(remap) else 0)
        if t != 0 and not is_defined(parents, x):
            bad.append(t)
    return bad


def as_arrays(records):
    """a dict key -> taxon, or (keys, taxa) in any order, as (keys int64 ascending, taxa int32)"""
    if isinstance(records, dict):
        keys = np.fromiter(records.keys(), np.int64, len(records))
        taxa = np.fromiter(records.values(), np.int32, len(records))
    else:
        keys, taxa = np.asarray(records[0], np.int64), np.asarray(records[1], np.int32)
    order = np.argsort(keys, kind="stable")
    return keys[order], taxa[order]


def same(a, b):
    a, b = as_arrays(a), as_arrays(b)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def sequences(rng, n, parents, lo=100, hi=12_000, n_fraction=0.3):
    """n sequences of lo..hi bases labelled with defined taxa.  About half of each is copied, segment by segment, from a common
    ancestor genome and from earlier sequences (so the same minimizers occur under several taxa, in whatever way the sequences are
    split into parts); some carry Ns."""
    taxa_pool = [t for t in taxgen.defined_taxa(parents) if t != 1]
    ancestor = synth.random_dna(hi, rng)
    seqs, taxa = [], []
    for i in range(n):
        s = synth.random_dna(int(rng.integers(lo, hi + 1)), rng).copy()
        for _ in range(1 + len(s) // 1500):
            other = ancestor if i == 0 or rng.random() < 0.5 else seqs[int(rng.integers(0, i))]
            length = int(min(len(s), len(other), rng.integers(200, 1500)))
            a, b = int(rng.integers(0, len(other) - length + 1)), int(rng.integers(0, len(s) - length + 1))
            s[b:b + length] = other[a:a + length]
        if rng.random() < n_fraction and len(s) > 400:
            at = int(rng.integers(0, len(s) - 40))
            s[at:at + int(rng.integers(1, 40))] = ord("N")
        seqs.append(s)
        taxa.append(int(rng.choice(taxa_pool)))
    return seqs, taxa


def pack(seqs):
    return synth.pack(seqs)


def build_records(p, parents, seqs, taxa):
    """orc.build_records of the labelled sequences, sorted by key"""
    if not seqs:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    bases, offsets = pack(seqs)
    return as_arrays(orc.build_records(p, parents, bases, offsets, taxa))
