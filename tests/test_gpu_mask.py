"""Low-complexity masking on the device (slacken_amd/csrc/mask.hip: slk_mask_sequences, slk_mask_device) bit for bit against the
recurrence of tests/mask_model.py (mask_dp), at the smallest shapes at which the kernel can go wrong: the shortest sequences, the
longest interval, repeats at every offset around the tile borders, runs that end and begin on them, invalid letters and sequence
borders inside the halo, every window and threshold the model's tests use, the replacements, the counter and the batch seams."""
import ctypes as C

import numpy as np
import pytest

import mask_model as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    import slacken_amd
    ix = slacken_amd.Index(expected_records=1024)   # (a stream belongs to an index; the masker needs nothing of it)
    s = ix.stream()
    yield s
    s.close()
    ix.close()


@pytest.fixture(scope="module")
def T():
    from slacken_amd import capi
    t = capi.mask_tile_bases()
    assert t >= 128 and t % 64 == 0
    return t


def flat(seqs):
    b = np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return b, offsets


def check(st, seqs, expect_some=True, **kw):
    """the device against the model on these sequences: letters and counter; -> (masked text, letters changed)"""
    b, offsets = flat(seqs)
    want, n_want = mm.mask_dp(b, offsets, **kw)
    got, n_got = st.mask_sequences(b, offsets, **kw)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"{diff.size} letters differ, the first at {diff[:8]} of {b.size}"
    assert n_got == n_want
    if expect_some:
        assert 0 < n_want < b.size, "vacuous: nothing masked, or everything"
    return bytes(got).decode("latin-1"), n_got


def filler(rng, n):
    return mm.skewed(rng, n, "ACGT")


def test_shortest_sequences_and_known_answers(st):
    seqs = ["", "A", "AA", "AAA", "A" * 6, "A" * 7, "AC" * 5, "AC" * 6, "A" * 6 + "N" + "A" * 6, "A" * 7 + "N" + "A" * 7, "AAAA", "AAAA", "",
            "u" * 7, "aAaAaAa", "TUtuTUt", "acacacACACAC", "GATTACA"]
    text, n = check(st, seqs)
    want = ["", "A", "AA", "AAA", "A" * 6, "x" * 7, "AC" * 5, "x" * 12, "A" * 6 + "N" + "A" * 6, "x" * 7 + "N" + "x" * 7, "AAAA", "AAAA", "",
            "x" * 7, "x" * 7, "x" * 7, "x" * 12, "GATTACA"]
    assert text == "".join(want)
    for s in ("", "A", "AA", "AAA", "A" * 6):
        check(st, [s], expect_some=False)
    assert check(st, ["A" * 7], expect_some=False) == ("x" * 7, 7)
    assert check(st, [], expect_some=False) == ("", 0)


@pytest.mark.parametrize("window", [8, 16, 64])
def test_the_longest_interval(st, T, window):
    """a perfect interval of exactly window - 2 triplets (window letters of one kind between invalid letters), one letter less and
    one more, at the start of the buffer and across a tile border"""
    rng = np.random.default_rng(window)
    parts = []
    for n in (window - 1, window, window + 1, 3 * window):
        parts += ["A" * n, "N", filler(rng, 30), "N"]
    text = "".join(parts)
    text += filler(rng, T - window // 2 - len(text) % T) + "N" + "T" * window + "N" + filler(rng, 50)
    out, _ = check(st, [text], window=window)
    assert out.startswith("x" * (window - 1) + "N") and "N" + "x" * window + "N" in out


@pytest.mark.parametrize("borders", [1, 2], ids=["one-border", "two-borders"])
@pytest.mark.parametrize("unit", ["A", "AC"])
def test_repeat_at_every_offset_around_the_tile_borders(st, T, unit, borders):
    """a 200-letter repeat whose start lies at every offset in [-64, +64] around tile border `borders` of its slab of three tiles
    (the slabs begin on multiples of the tile, so every repeat meets the border at its own offset), inside uniform text"""
    rng = np.random.default_rng(len(unit) * 10 + borders)
    rep = (unit * 200)[:200]
    slabs = []
    for o in range(-64, 65):
        at = borders * T + o
        slabs.append(filler(rng, at) + rep + filler(rng, 3 * T - at - 200))
    out, n = check(st, ["".join(slabs)])
    assert n >= 129 * 200


def test_a_repeat_over_more_than_two_tiles_and_runs_on_the_borders(st, T):
    rng = np.random.default_rng(2)
    text = filler(rng, T - 100) + "G" * (2 * T + 200) + filler(rng, T - 100)               # from tile 0 into tile 3
    assert len(text) == 4 * T
    text += filler(rng, T - 40) + "AC" * 20 + "N" + filler(rng, T - 2) + "N" + "TG" * 20     # a run that ends on the last letter of a tile; one that begins on the first
    assert text[5 * T - 1] == "C" and text[5 * T] == "N" and text[6 * T - 1] == "N" and text[6 * T] == "T"
    check(st, [text + filler(rng, 70)])
    # the same borders made by sequence ends instead of invalid letters
    seqs = [filler(rng, T - 40) + "AC" * 20, filler(rng, T - 30) + "A" * 30, "A" * 30 + filler(rng, 100)]
    out, _ = check(st, seqs)
    assert out[T - 40:T] == "x" * 40 and out[2 * T - 30:2 * T + 30] == "x" * 60


@pytest.mark.parametrize("where", [-1, 0, 1])
def test_an_invalid_letter_beside_the_tile_border_inside_a_repeat(st, T, where):
    rng = np.random.default_rng(3)
    text = list(filler(rng, T - 90) + "A" * 180 + filler(rng, T - 90 - 70) + "CA" * 70 + filler(rng, T - 70))
    for border in (T, 2 * T):
        assert text[border - 2] == text[border + 2] and text[border + where] in "AC"
        text[border + where] = "N"
    out, _ = check(st, ["".join(text)])
    assert out[T + where] == "N" and out[T + where - 5:T + where] == "xxxxx" and out[T + where + 1:T + where + 6] == "xxxxx"


def test_many_short_sequences_across_a_tile_border(st, T):
    """sequences of 1..10 letters of one kind packed from 300 letters before a tile border to 300 behind it: the runs end at sequence
    borders inside the halo; those of 7 letters and more are masked whole, the shorter ones not at all"""
    rng = np.random.default_rng(4)
    seqs = [filler(rng, T - 300)]
    total = 0
    while total < 600:
        n = int(rng.integers(1, 11))
        seqs.append("ACGT"[int(rng.integers(0, 4))] * n)
        total += n
    seqs.append(filler(rng, 200))
    out, _ = check(st, seqs)
    at = len(seqs[0])
    for s in seqs[1:-1]:
        assert out[at:at + len(s)] == ("x" * len(s) if len(s) >= 7 else s)
        at += len(s)


@pytest.fixture(scope="module")
def families(T):
    """skewed alphabets and planted repeats over a few tiles, with invalid letters, lower case and U, as several sequences"""
    rng = np.random.default_rng(5)
    seqs = []
    for alphabet in ("AC", "AAAC", "ACG", "AACG", "ACGT", "AAAAACGT"):
        seqs.append(mm.skewed(rng, int(rng.integers(T // 2, T)), alphabet))
        seqs.append("".join(c if c in alphabet else alphabet[0] for c in mm.planted(rng, 700, 6, 3, 14, 120)))
    text = list(mm.planted(rng, 3 * T + 17, 12, 4, 20, 300))
    for at in rng.integers(0, len(text), 25):
        text[int(at)] = "NnRYx-*"[int(at) % 7]
    for at in rng.integers(0, len(text) - 50, 6):
        text[int(at):int(at) + 50] = "".join(text[int(at):int(at) + 50]).lower().replace("t", "u")
    seqs.append("".join(text))
    return seqs


@pytest.mark.parametrize("threshold", [10, 20, 40])
@pytest.mark.parametrize("window", [8, 16, 64])
def test_windows_and_thresholds(st, families, window, threshold):
    # (window 8 with threshold 40 masks nothing by arithmetic -- see test_mask_model.py -- and must come back untouched)
    _, n = check(st, families, expect_some=(window, threshold) != (8, 40), window=window, threshold=threshold)
    assert (n == 0) == ((window, threshold) == (8, 40))


@pytest.mark.parametrize("replacement", [ord("x"), ord("N"), 0])
def test_replacements_and_the_counter(st, families, replacement):
    b, offsets = flat(families)
    out, n = check(st, families, replacement=replacement)
    changed = [i for i, (x, y) in enumerate(zip(bytes(b).decode("latin-1"), out)) if x != y]
    assert n == len(changed)
    if replacement:
        assert all(out[i] == chr(replacement) for i in changed)
    else:
        assert all(out[i] == chr(b[i]).lower() and chr(b[i]).isupper() for i in changed)
        _, n_hard = mm.mask_dp(b, offsets)
        assert n < n_hard                                             # masked lower-case letters stay as they are and are not counted


@pytest.mark.parametrize("batch", [1000, 4096])
def test_batch_seams(st, monkeypatch, batch):
    """slk_mask_sequences with small staged batches on a 20 000-letter sequence with repeats on the seams, and on short sequences
    beside it: the same letters as in one batch, and as the model"""
    rng = np.random.default_rng(6)
    text = list(filler(rng, 20000))
    for seam in range(batch, 20000, batch):
        unit = ("A", "AC", "ACG", "T")[(seam // batch) % 4]
        for o in (-100, -31, -3, 40):
            if (seam // batch) % 3 == (o % 3):
                text[seam + o:seam + o + 60] = (unit * 60)[:60]
    seqs = ["A" * 9, "".join(text), "AC" * 30, "", filler(rng, 333)]
    b, offsets = flat(seqs)
    one, n_one = st.mask_sequences(b, offsets)
    monkeypatch.setenv("SLK_MASK_BATCH_BASES", str(batch))
    out, n = check(st, seqs)
    assert out == bytes(one).decode() and n == n_one


def test_invalid_configs_leave_the_buffer_untouched(st):
    from slacken_amd import capi
    b, offsets = flat(["A" * 40, "AC" * 30])
    for window, threshold in ((7, 20), (65, 20), (64, 256), (1, 1), (1 << 20, 20)):
        with pytest.raises(capi.SlackenError) as e:
            st.mask_sequences(b, offsets, window=window, threshold=threshold)
        assert e.value.code == capi.E_INVALID
        work, masked = b.copy(), C.c_uint64(7)
        cfg = capi.MaskConfig(window, threshold, ord("x"))
        rc = capi.lib().slk_mask_sequences(st.h, work.ctypes.data, offsets.ctypes.data, 2, C.byref(cfg), C.byref(masked))
        assert rc == capi.E_INVALID and np.array_equal(work, b) and masked.value == 0
    bad = np.array([0, 50, 40, 100], np.uint64)
    work, masked = b.copy(), C.c_uint64(0)
    assert capi.lib().slk_mask_sequences(st.h, work.ctypes.data, bad.ctypes.data, 3, None, C.byref(masked)) == capi.E_INVALID
    assert np.array_equal(work, b)
    # the defaults: a null config, and zeros
    for cfg in (None, C.byref(capi.MaskConfig(0, 0, 0))):
        work = b.copy()
        assert capi.lib().slk_mask_sequences(st.h, work.ctypes.data, offsets.ctypes.data, 2, cfg, C.byref(masked)) == 0
        assert bytes(work) == b"a" * 40 + b"ac" * 30 and masked.value == 100


def test_mask_device_in_place(st, T, families):
    """slk_mask_device with every array on the device (torch tensors) and guard bytes behind the letters"""
    import torch
    from slacken_amd import capi
    b, offsets = flat(families)
    want, n_want = mm.mask_dp(b, offsets, replacement=ord("N"))
    guard = 4 * T
    d_bases = torch.full((b.size + guard,), 65, dtype=torch.uint8, device="cuda")          # (a homopolymer behind the end: it must stay)
    d_bases[:b.size] = torch.from_numpy(b).cuda()
    d_offsets = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_masked = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cfg = capi.MaskConfig(64, 20, ord("N"))
    rc = capi.lib().slk_mask_device(st.h, d_bases.data_ptr(), d_offsets.data_ptr(), offsets.size - 1, C.byref(cfg), d_masked.data_ptr())
    assert rc == 0, capi.lib().slk_last_error()
    st.synchronize()
    got = d_bases.cpu().numpy()
    assert np.array_equal(got[:b.size], want) and (got[b.size:] == 65).all()
    assert d_masked.cpu().tolist() == [n_want, -1]
    # invalid: nothing is touched
    bad = capi.MaskConfig(4, 20, ord("N"))
    assert capi.lib().slk_mask_device(st.h, d_bases.data_ptr(), d_offsets.data_ptr(), offsets.size - 1, C.byref(bad), d_masked.data_ptr()) == capi.E_INVALID
    st.synchronize()
    assert np.array_equal(d_bases.cpu().numpy(), got) and d_masked.cpu().tolist() == [n_want, -1]
