"""slk_pack_bases_sparse (host only, no GPU): the codes of slk_pack_bases, and the validity as the list of the words that hold an
invalid base -- the dense validity rebuilt from that list equals slk_pack_bases's."""
import ctypes as C

import numpy as np
import pytest

import slacken_amd
from slacken_amd import capi

E_CAPACITY = -5
SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097]


def dense(text):
    codes, valid = capi.pack_bases(text)
    words = (text.size + 15) // 16
    return codes[:words], valid[:words]


def rebuild(n, exc_word, exc_bits):
    """the dense validity words of n bases that are all valid except in the listed words"""
    words = (n + 15) // 16
    valid = np.full(words, 0xFFFF, np.uint16)
    if n % 16:
        valid[-1] = (1 << (n % 16)) - 1
    valid[exc_word] = exc_bits
    return valid


def texts(n, rng):
    nt = np.frombuffer(b"ACGTacgtUu", np.uint8)
    clean = nt[rng.integers(0, len(nt), n)]
    every = clean.copy()
    every[::16] = ord("N")                      # an invalid base in every word
    few = clean.copy()
    few[rng.random(n) < 0.01] = ord("N")
    return dict(any_byte=rng.integers(0, 256, n).astype(np.uint8), no_exception=clean, every_word=every, a_few=few)


@pytest.mark.parametrize("n", SIZES)
def test_sparse_form_equals_dense(n):
    rng = np.random.default_rng(1000 + n)
    for name, text in texts(n, rng).items():
        want_codes, want_valid = dense(text)
        codes, exc_word, exc_bits = capi.pack_bases_sparse(text)
        words = (n + 15) // 16
        assert np.array_equal(codes[:words], want_codes), name
        assert np.array_equal(rebuild(n, exc_word, exc_bits), want_valid), name
        assert (np.diff(exc_word.astype(np.int64)) > 0).all() and (exc_word < max(words, 1)).all(), name
        # listed iff a base of the word is invalid
        full = rebuild(n, np.zeros(0, np.int64), np.zeros(0, np.uint16))
        assert np.array_equal(exc_word, np.flatnonzero(want_valid != full)), name
        if name == "no_exception":
            assert exc_word.size == 0
        if name == "every_word":
            assert exc_word.size == words


def test_large_input_goes_through_the_slices():
    """more than one 2^22-base slice: the exceptions of the slices in order, the words numbered through"""
    rng = np.random.default_rng(5)
    n = (1 << 23) + 12345
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    text[rng.integers(0, n, 5000)] = ord("N")
    text[(1 << 22) - 1] = text[1 << 22] = ord("n")      # either side of a slice border
    want_codes, want_valid = dense(text)
    codes, exc_word, exc_bits = capi.pack_bases_sparse(text)
    assert np.array_equal(codes[:len(want_codes)], want_codes)
    assert np.array_equal(rebuild(n, exc_word, exc_bits), want_valid)
    assert (np.diff(exc_word.astype(np.int64)) > 0).all()


def test_capacity_rule():
    L = slacken_amd.lib()
    rng = np.random.default_rng(9)
    n = 4097
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    text[::64] = ord("N")
    want_codes, want_valid = dense(text)
    _, all_word, all_bits = capi.pack_bases_sparse(text)
    need = all_word.size
    assert need == (n + 63) // 64
    for cap in (0, 1, need - 1):
        codes = np.full((n + 15) // 16, 0xDEADBEEF, np.uint32)
        exc_word, exc_bits = np.full(cap + 4, 0xA5A5A5A5, np.uint32), np.full(cap + 4, 0xA5A5, np.uint16)
        got = C.c_uint64(0)
        rc = L.slk_pack_bases_sparse(text.ctypes.data, n, codes.ctypes.data, exc_word.ctypes.data if cap else None,
                                     exc_bits.ctypes.data if cap else None, cap, C.byref(got))
        assert rc == E_CAPACITY and got.value == need
        assert np.array_equal(codes, want_codes)                       # the codes are written in full all the same
        assert np.array_equal(exc_word[:cap], all_word[:cap]) and np.array_equal(exc_bits[:cap], all_bits[:cap])
        assert (exc_word[cap:] == 0xA5A5A5A5).all() and (exc_bits[cap:] == 0xA5A5).all()   # nothing past the capacity
    got = C.c_uint64(0)
    exc_word, exc_bits = np.zeros(need, np.uint32), np.zeros(need, np.uint16)
    codes = np.zeros((n + 15) // 16, np.uint32)
    assert L.slk_pack_bases_sparse(text.ctypes.data, n, codes.ctypes.data, exc_word.ctypes.data, exc_bits.ctypes.data, need, C.byref(got)) == 0
    assert got.value == need and np.array_equal(exc_word, all_word)
    assert L.slk_pack_bases_sparse(text.ctypes.data, n, codes.ctypes.data, None, None, 0, None) == -1      # null count
