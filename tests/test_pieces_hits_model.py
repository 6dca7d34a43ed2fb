"""The rule that joins the pieces' hit lists (tests/pieces_hits_model.py) against the oracle's list of the whole read:
the same entries, taxon and k-mers, wherever the borders fall -- through runs of Ns shorter than, equal to and longer than k, through
one ambiguous span or one super-mer that every border cuts, through a whole piece of Ns, with a last piece of one window.  No GPU: this
pins the rule the kernels implement, and passes without them."""
import numpy as np
import pytest

import pieces_hits_model as phm
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
    got, plan = phm.by_pieces(orc, world["p"], world["oix"], world["parents"], read, piece_windows)
    want = phm.whole(orc, world["p"], world["oix"], world["parents"], read)
    assert got == want, (len(read), piece_windows, len(got), len(want), next((i, a, b) for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b))
    # the plan: the pieces' entries follow each other without a gap, and a cut piece begins where the entry it continues ends
    at = 0
    for start, cut, stored in plan:
        assert start == at and (not cut or start > 0)
        at += stored
    assert at == len(want)
    return plan


def test_every_piece_size_on_one_read(orc, world):
    read = pm.long_read(world["lib"], np.random.default_rng(5), 3300)
    for pw in range(64, 201):
        same(orc, world, read, pw)


def test_n_runs_slid_across_a_border(orc, world):
    """shorter than k, k - 1, k, k + 1, two k: every position from well before the border to behind it"""
    base = world["lib"].genomes[0][:1500].copy()
    pw = 128
    for ins_len in (1, 34, 35, 36, 70):
        for at in range(512 - 75, 512 + 40):
            r = base.copy()
            r[at:at + ins_len] = ord("N")
            same(orc, world, r, pw)


def test_repeats_slid_across_borders(orc, world):
    base = world["lib"].genomes[0][:1800].copy()
    unit = np.frombuffer(b"AC", np.uint8)
    for at in range(1000, 1000 + 130, 3):              # 300 bases of one repeat: across three borders
        r = base.copy()
        r[at:at + 300] = np.tile(unit, 150)
        same(orc, world, r, 128)
        same(orc, world, r, 64)


def test_one_entry_cut_by_every_border(orc, world):
    for pw in range(64, 201):
        for read in (np.full(700, ord("N"), np.uint8),                      # one ambiguous span
                     np.tile(np.frombuffer(b"ACGGT", np.uint8), 140)):      # one minimizer value throughout
            plan = same(orc, world, read, pw)
            assert [stored for _, _, stored in plan] == [1] + [0] * (len(plan) - 1)      # the later pieces store nothing and pass their k-mers on
            assert all(cut for _, cut, _ in plan[1:])
    for pw in (64, 100, 4096):
        same(orc, world, np.full(5000, ord("N"), np.uint8), pw)
        same(orc, world, np.tile(np.frombuffer(b"ACGGT", np.uint8), 1000), pw)
        same(orc, world, np.full(3000, ord("A"), np.uint8), pw)


def test_a_whole_piece_of_ns_between_equal_flanks(orc, world):
    flank = world["lib"].genomes[1][:200]
    rep = np.tile(np.frombuffer(b"AC", np.uint8), 100)   # the same key on either side of the gap
    for f in (flank, rep):
        read = np.concatenate([f, np.full(900, ord("N"), np.uint8), f])
        for pw in range(64, 201):
            plan = same(orc, world, read, pw)
        assert any(cut and stored == 0 for _, cut, stored in plan)          # (200 windows: a piece that is nothing but Ns)


def test_a_last_piece_of_one_window(orc, world):
    g = world["lib"].genomes[2]
    k = world["p"].k
    for pw in range(64, 201):
        for extra in (0, 1, 2):                        # two whole pieces; one window more; two more
            read = g[500:500 + 2 * pw + k - 1 + extra].copy()
            plan = same(orc, world, read, pw)
            assert len(plan) == (2 if extra == 0 else 3)
        read = np.concatenate([g[:2 * pw - 5], np.full(k + 40, ord("N"), np.uint8)])[:2 * pw + k].copy()   # ... and that window in an ambiguous span
        same(orc, world, read, pw)


@pytest.mark.parametrize("seed", range(3))
def test_long_reads(orc, world, seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(4):
        read = pm.long_read(world["lib"], rng, int(rng.integers(1001, 9000)))
        for pw in (64, 100, 333, 1024):
            same(orc, world, read, pw)
