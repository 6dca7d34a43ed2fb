"""The two CPU statements of low-complexity masking (tests/mask_model.py: the definition and the recurrence) against the known
answers of DESIGN.md 20 and against each other.  Every random family must hold masked and unmasked letters, or its test is vacuous."""
import numpy as np
import pytest

import mask_model as mm


def masked_positions(text, **kw):
    out = mm.mask_text(text, **kw)
    return [i for i, (a, b) in enumerate(zip(text, out)) if a != b]


def test_known_answers():
    assert mm.mask_text("A" * 6) == "A" * 6                  # l = 4, S = 6: 60 > 60 is false
    assert mm.mask_text("A" * 7) == "x" * 7
    assert mm.mask_text("AC" * 5) == "AC" * 5
    assert mm.mask_text("AC" * 6) == "x" * 12


def test_invalid_letters_and_borders_end_a_run():
    assert mm.mask_text("A" * 6 + "N" + "A" * 6) == "A" * 6 + "N" + "A" * 6
    assert mm.mask_text("A" * 7 + "N" + "A" * 7) == "x" * 7 + "N" + "x" * 7
    b = np.frombuffer(b"AAAAAAAA", np.uint8)
    for f in (mm.mask_brute, mm.mask_dp):
        out, n = f(b, [0, 4, 8])
        assert bytes(out) == b"AAAAAAAA" and n == 0
        out, n = f(b, [0, 8])
        assert bytes(out) == b"xxxxxxxx" and n == 8
        out, n = f(b, [0, 0, 8, 8])                            # empty sequences beside it
        assert bytes(out) == b"xxxxxxxx" and n == 8


def test_u_and_lower_case_are_valid():
    assert mm.mask_text("u" * 7) == "x" * 7
    assert mm.mask_text("aAaAaAa") == "x" * 7
    assert mm.mask_text("TUtuTUt") == "x" * 7                # U is read as T
    assert mm.mask_text("TUTUTA") == "TUTUTA"
    assert mm.mask_text("acacacACACAC") == "x" * 12


def test_soft_masking_and_other_replacements():
    assert mm.mask_text("GATTACA" + "A" * 7 + "N", replacement=0) == "GATTAC" + "a" * 8 + "N"    # (the run of A starts inside GATTACA)
    assert mm.mask_text("A" * 7, replacement=ord("N")) == "N" * 7
    b = np.frombuffer(b"aaaaAAAA", np.uint8)
    out, n = mm.mask_dp(b, [0, 8], replacement=0)
    assert bytes(out) == b"aaaaaaaa" and n == 4               # letters CHANGED: the lower-case ones were as they are now
    out, n = mm.mask_dp(b, [0, 8], replacement=ord("x"))
    assert bytes(out) == b"xxxxxxxx" and n == 8


def test_parameters_are_checked():
    b = np.frombuffer(b"AAAAAAAA", np.uint8)
    for w, t in ((7, 20), (65, 20), (64, 0), (64, 256)):
        with pytest.raises(ValueError):
            mm.mask_dp(b, [0, 8], window=w, threshold=t)


FAMILIES = [("AC", 2), ("AAAC", 2), ("ACG", 3), ("AACG", 3), ("ACGT", 4), ("AAAAACGT", 4)]


@pytest.mark.parametrize("threshold", [10, 20, 40])
@pytest.mark.parametrize("window", [8, 16, 64])
def test_brute_equals_dp(window, threshold):
    """(window 8 with threshold 40 masks nothing by arithmetic: at most 6 triplets, S <= 15, and 10 * 15 > 40 * 5 is false.  There
    the families must come out untouched; everywhere else each must hold masked and unmasked letters.)"""
    rng = np.random.default_rng(1000 * window + threshold)
    for alphabet, _ in FAMILIES:
        fam_masked = fam_clear = 0
        for i in range(8):
            # skewed draws of 3..40 letters, and uniform text of 25..40 with one repeat of a 1- or 2-letter unit planted in it, folded
            # onto the family's alphabet (12 letters of one kind are 10 triplets, S / (l - 1) = 5: above every threshold used here)
            n = int(rng.integers(3, 41)) if i % 2 else int(rng.integers(25, 41))
            text = mm.skewed(rng, n, alphabet) if i % 2 else "".join(c if c in alphabet else alphabet[0] for c in mm.planted(rng, n, 1, 2, 14, 22))
            b = np.frombuffer(text.encode(), np.uint8)
            want, nw = mm.mask_brute(b, [0, n], window, threshold)
            got, ng = mm.mask_dp(b, [0, n], window, threshold)
            assert bytes(got) == bytes(want) and ng == nw, (text, window, threshold)
            fam_masked += nw
            fam_clear += n - nw
        if (window, threshold) == (8, 40):
            assert fam_masked == 0
        else:
            assert fam_masked and fam_clear, f"vacuous: family {alphabet} holds {fam_masked} masked and {fam_clear} unmasked letters"


@pytest.mark.parametrize("alphabet", [a for a, _ in FAMILIES])
def test_each_family_has_masked_and_unmasked_letters(alphabet):
    """at the default parameters, on the strings the engine's tests draw from the same generators"""
    rng = np.random.default_rng(len(alphabet) * 31 + ord(alphabet[-1]))
    text = mm.planted(rng, 400, 3, 4, 20, 60)
    text = text if alphabet == "ACGT" else mm.skewed(rng, 200, alphabet) + text
    pos = masked_positions(text)
    assert 0 < len(pos) < len(text)


def test_brute_equals_dp_with_several_sequences_and_invalid_letters():
    rng = np.random.default_rng(5)
    text = list(mm.planted(rng, 300, 6, 3, 10, 40))
    for at in rng.integers(0, 300, 12):
        text[int(at)] = "N"
    b = np.frombuffer("".join(text).encode(), np.uint8)
    offsets = [0] + sorted(int(x) for x in rng.integers(0, 300, 7)) + [300]
    for w in (8, 64):
        want, nw = mm.mask_brute(b, offsets, w, 20)
        got, ng = mm.mask_dp(b, offsets, w, 20)
        assert bytes(got) == bytes(want) and ng == nw and 0 < nw < 300


@pytest.mark.parametrize("window,threshold", [(64, 20), (16, 10), (16, 40), (8, 20)])
def test_reverse_complement_symmetry(window, threshold):
    rng = np.random.default_rng(window)
    seen = 0
    for alphabet in ("AAAC", "ACGT", "AACG"):
        for _ in range(4):
            text = mm.skewed(rng, 60, alphabet) + mm.planted(rng, 120, 2, 3, 15, 40)
            fwd = set(masked_positions(text, window=window, threshold=threshold))
            rev = set(masked_positions(mm.revcomp(text), window=window, threshold=threshold))
            assert {len(text) - 1 - p for p in rev} == fwd
            seen += len(fwd)
            assert len(fwd) < len(text)
    assert seen > 0
