"""The rule between the pieces of a split fragment (tests/pieces_model.py) against the oracle's run over the whole read:
hit groups, spans, k-mer total and the taxon map must come out the same wherever the borders fall -- through super-mers, through runs
of Ns shorter and longer than k, through repeats that are one super-mer for hundreds of windows, through pieces that hold no
super-mer at all.  No GPU: this pins the rule the kernels implement."""
import numpy as np
import pytest

import pieces_model as pm
import taxgen


@pytest.fixture(scope="module")
def world(orc):
    p = orc.params()
    rng = np.random.default_rng(77)
    parents = taxgen.taxonomy(8 * 32, rng)
    lib, keys, taxa = pm.library_with_repeats(orc, p, parents, rng, n_genomes=6, genome_len=12000, pad_records=2000)
    return dict(p=p, lib=lib, parents=parents, oix=orc.Index(1, keys, taxa))


def same(orc, world, read, piece_windows):
    got = pm.by_pieces(orc, world["p"], world["oix"], read, piece_windows)
    want = pm.whole(orc, world["p"], world["oix"], world["parents"], read)
    assert got == want, (len(read), piece_windows, {k: (got[k], want[k]) for k in got if got[k] != want[k] and k != "map"})


def test_cut_takes_every_window_once():
    for n, pw in ((35, 64), (98, 64), (99, 64), (3300, 64), (3300, 200), (8226, 4096), (8227, 4096)):
        pieces = pm.cut(n, 35, pw)
        assert pieces[0][0] == 0 and sum(b - 34 for _, b in pieces) == n - 34
        assert all(a2 == a1 + b1 - 34 for (a1, b1), (a2, _) in zip(pieces, pieces[1:]))
        assert all(b - 34 == pw for _, b in pieces[:-1]) and 1 <= pieces[-1][1] - 34 <= pw


def test_every_piece_size_on_one_read(orc, world):
    read = pm.long_read(world["lib"], np.random.default_rng(5), 3300)
    for pw in range(64, 201):
        same(orc, world, read, pw)


@pytest.mark.parametrize("seed", range(4))
def test_long_reads(orc, world, seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(6):
        read = pm.long_read(world["lib"], rng, int(rng.integers(1001, 9000)))
        for pw in (64, 100, 333, 1024):
            same(orc, world, read, pw)


def test_n_runs_and_repeats_slid_across_borders(orc, world):
    base = world["lib"].genomes[0][:3300].copy()
    pw = 128                                           # borders at windows 128, 256, ..: bases 128, 256, ..
    for ins_len in (1, 34, 35, 36, 70):
        for at in range(1024 - 75, 1024 + 40, 1):
            r = base.copy()
            r[at:at + ins_len] = ord("N")
            same(orc, world, r, pw)
    unit = np.frombuffer(b"AC", np.uint8)
    for at in range(1000, 1000 + 130, 3):              # 300 bases of one repeat: across three borders
        r = base.copy()
        r[at:at + 300] = np.tile(unit, 150)
        same(orc, world, r, pw)
        same(orc, world, r, 64)


def test_one_span_cut_many_times(orc, world):
    for pw in (64, 100, 4096):
        same(orc, world, np.full(5000, ord("N"), np.uint8), pw)                      # one ambiguous span
        same(orc, world, np.tile(np.frombuffer(b"ACGGT", np.uint8), 1000), pw)       # one minimizer value throughout
        same(orc, world, np.full(3000, ord("A"), np.uint8), pw)


def test_a_piece_without_a_super_mer_between_equal_keys(orc, world):
    """the last super-mer before a piece's first one may lie several pieces back"""
    flank = world["lib"].genomes[1][:200]
    read = np.concatenate([flank, np.full(900, ord("N"), np.uint8), flank])
    for pw in (64, 128, 300):
        same(orc, world, read, pw)
    rep = np.tile(np.frombuffer(b"AC", np.uint8), 100)   # the same key on either side of the gap
    read = np.concatenate([rep, np.full(700, ord("N"), np.uint8), rep])
    for pw in (64, 128, 300):
        same(orc, world, read, pw)
