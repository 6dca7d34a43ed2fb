"""What `respace` computes (KeyValueIndex.respace, S/slacken/KeyValueIndex.scala:353-384), stated in full: every record's minimizer
ANDed with the space mask of the new number of spaces, the records grouped by the masked minimizer, each group's taxon the LCA of
its members' taxa.  And a generator of libraries on which that merges: the golden library alone keeps every one of its keys
distinct at 8, 10, 12 and 15 spaces, so it tests no merge at all.  Test infrastructure; numpy and the oracle's LCA only."""
import numpy as np

import taxgen
from oracle import oracle

WORD = (1 << 64) - 1
ROOT = 1


def mask(m, s):
    """SpacedSeed.spaceMask, left aligned, as tests/test_gpu_stats_cli.py::splitter_lines computes it"""
    assert 0 < m < 32 and 0 <= s <= m // 2
    space = (WORD << ((32 - m) * 2)) & WORD
    for _ in range(s):
        space = ((space << 4) | (3 << (64 - m * 2))) & WORD
    return space


def as_i64(x):
    return np.asarray(x, np.uint64).view(np.int64)


def respace(keys, taxa, parents, m, s_new):
    """-> (keys int64 ascending, taxa int32): {key & mask(m, s_new): LCA of the group's taxa}"""
    keys = (np.asarray(keys, np.int64).view(np.uint64) & np.uint64(mask(m, s_new))).view(np.int64)
    taxa = np.asarray(taxa, np.int32)
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    pairs = np.unique(np.stack([keys, taxa.astype(np.int64)], axis=1), axis=0)   # (LCA is idempotent: a pair counts once)
    uniq, start = np.unique(pairs[:, 0], return_index=True)
    ends = np.append(start[1:], len(pairs))
    out = pairs[start, 1].astype(np.int32)
    parents = np.ascontiguousarray(parents, np.int32)
    for i in np.nonzero(ends - start > 1)[0]:
        t = 0
        for x in pairs[start[i]:ends[i], 1]:
            t = oracle.lca(parents, t, int(x))
        out[i] = t
    return uniq.astype(np.int64), out


def free_bits(m, s_old, s_new):
    """positions of the bits that mask(s_old) keeps and mask(s_new) clears"""
    diff = mask(m, s_old) & ~mask(m, s_new) & WORD
    return [b for b in range(64) if diff >> b & 1]


def deposit(fills, bits):
    """bit j of every fill to position bits[j]"""
    fills = np.asarray(fills, np.uint64)
    out = np.zeros(len(fills), np.uint64)
    for j, b in enumerate(bits):
        out |= ((fills >> np.uint64(j)) & np.uint64(1)) << np.uint64(b)
    return out


def generate(n_classes, rng, m=31, s_old=7, s_new=12, parents=None):
    """-> dict(keys, taxa, parents, class_of, full_class): records of a library at s_old spaces in n_classes classes of keys that
    share key & mask(s_new).  Class sizes are geometric (p = 1/4) capped at 64 (and at the number of fills there are); class 0 holds
    ALL 2^(2(s_new - s_old)) fills of the freed bits.  Members are the base plus distinct random fills.  Taxa come from a
    taxgen.taxonomy(400): for every other class from one random clade, otherwise from all taxa.  The records are shuffled."""
    if parents is None:
        parents = taxgen.taxonomy(400, rng)
    bits = free_bits(m, s_old, s_new)
    F = 1 << len(bits)
    assert len(bits) == 2 * (s_new - s_old)
    base = np.unique(rng.integers(0, 2**64, int(n_classes * 1.1) + 8, dtype=np.uint64) & np.uint64(mask(m, s_new)))
    base = rng.permutation(base)[:n_classes]
    assert len(base) == n_classes
    size = np.minimum(rng.geometric(0.25, n_classes), min(64, F))
    size[0] = F
    class_of = np.repeat(np.arange(n_classes), size)
    j = np.arange(len(class_of)) - np.repeat(np.cumsum(size) - size, size)        # member number inside its class
    a = rng.integers(0, F, n_classes)
    b = rng.integers(0, F // 2, n_classes) * 2 + 1                                # odd: j -> a + b j is a bijection mod F
    fills = (a[class_of] + b[class_of] * j) % F
    keys = base[class_of] | deposit(fills, bits)
    defined = np.array(taxgen.defined_taxa(parents), np.int32)
    # clades: the descendants-or-self of every node (parents have lower ids than children in taxgen's trees)
    members = {int(t): [int(t)] for t in defined}
    for t in sorted(members, reverse=True):
        if parents[t] != 0:
            members[int(parents[t])].extend(members[t])
    taxa = rng.choice(defined, len(keys)).astype(np.int32)
    big = [t for t in members if t != ROOT and len(members[t]) >= 3]
    first = np.cumsum(size) - size
    for c in range(0, n_classes, 2):
        clade = members[big[int(rng.integers(0, len(big)))]]
        taxa[first[c]:first[c] + size[c]] = rng.choice(clade, size[c])
    order = rng.permutation(len(keys))
    return dict(keys=as_i64(keys[order]), taxa=taxa[order], parents=parents, class_of=class_of[order], full_class=as_i64(keys[class_of == 0]),
                m=m, s_old=s_old, s_new=s_new)


def outcomes(g):
    """classes with several taxa by what their LCA is: ROOT, an interior node no member held, a member's own taxon (an ancestor of the rest)"""
    mk, mt = respace(g["keys"], g["taxa"], g["parents"], g["m"], g["s_new"])
    masked = (g["keys"].view(np.uint64) & np.uint64(mask(g["m"], g["s_new"]))).view(np.int64)
    at = np.searchsorted(mk, masked)
    held = {}
    for i, t in zip(at.tolist(), g["taxa"].tolist()):
        held.setdefault(i, set()).add(t)
    out = dict(single=0, root=0, interior=0, member=0)
    for i, s in held.items():
        t = int(mt[i])
        out["single" if len(s) == 1 else "member" if t in s else "root" if t == ROOT else "interior"] += 1
    return out
