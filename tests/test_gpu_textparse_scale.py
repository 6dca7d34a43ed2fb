"""The device text parser (slacken_amd/csrc/textparse.hip) at the sizes the command line really sends: chunks of 8 MiB and more, where
one scan thread folds several tiles (more than SB tiles), the blocks stride over their tiles (more than G tiles), the line-tile and
record loops stride (more than G * LB lines or records), and one record's carries cross many scan parts.  The reference is
tests/hostmodel.py (parse_fasta, parse_fastq; pairparse_model.lockstep for mates), compared exactly: titles, sequences, record count
and `consumed`.  Every case first asserts, from the length of its text or from the model's own line split, that it lies on the side of
the border it is named for.  tests/test_textparse_cpu.py pins the four constants below to textparse.hip."""
import functools
import gzip
import re

import numpy as np
import pytest

from slacken_amd import capi
from pairparse_model import lockstep, strip
from test_gpu_pairparse import render
from test_gpu_pipe import small_k  # noqa: F401  (the fixture: the k = 21, m = 12 world)
from test_gpu_textparse import MODEL, parse_chunked
from test_gpu_textparse_cli import cli

pytestmark = pytest.mark.gpu

T = capi.parse_tile_bytes()   # textparse.hip: TP_TILE, the bytes of one block's tile (host arithmetic: no device is opened)
SB = 1024                     # TP_SCAN_BLOCK: the threads of the one-block scan; above SB tiles a thread folds several
G = 2048                      # TP_MAX_GRID: the blocks of a pass; above G tiles (or G line tiles, or G * LB records) a block takes several
LB = 256                      # TP_BLOCK: the lines of one line tile, the records of one block of the compare pass
EOLS = ("\n", "\r\n", "\r")
BIG_BYTES = (2 * G + 2) * T   # what the generated texts hold at least


def tiles(n, fmt, final=True):
    """launch_parse's ntiles: a final FASTA chunk has n + 1 positions, the end of the text closes a record"""
    return -(-(n + 1 if fmt == "fasta" and final else n) // T)


def model_lines(text):
    """the lines of a FASTQ text as hostmodel.parse_fastq splits them"""
    lines = re.split("\r\n|\n|\r", text)
    if lines and lines[-1] == "":
        lines.pop()
    return lines


@pytest.fixture(scope="module")
def st():
    import slacken_amd
    ix = slacken_amd.Index(expected_records=1024)   # (a stream belongs to an index; the parser needs nothing of it)
    s = ix.stream()
    yield s
    s.close()
    ix.close()
    for cached in (big, head_of, tiny_records, many_lines, numbered, mate_text):   # (the texts of this file are large)
        cached.cache_clear()


@functools.lru_cache(maxsize=None)
def pool():
    """2^16 bases drawn once: every sequence of this file is a slice of them"""
    rng = np.random.default_rng(3)
    return np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=1 << 16, p=[0.245, 0.245, 0.245, 0.245, 0.02])].tobytes().decode()


@functools.lru_cache(maxsize=None)
def big(fmt):
    """At least BIG_BYTES of records, built once per format: 1-300 bases, \\n, \\r\\n or a lone \\r per record, titles with spaces, empty
    lines between some records; FASTQ: quality lines that begin with '@', '+' lines with and without a name; FASTA: '>' inside
    headers, sequences over several lines of 61 or 70 columns or on one."""
    rng = np.random.default_rng({"fastq": 101, "fasta": 102}[fmt])
    P = pool()
    K = BIG_BYTES // 100
    lens, starts, eols = (rng.integers(1, 301, K).tolist(), rng.integers(0, len(P) - 300, K).tolist(), rng.integers(0, 3, K).tolist())
    qual = "I" * 300
    out, size = [], 0
    for i in range(K):
        if size >= BIG_BYTES + 64:
            break
        e, L = EOLS[eols[i]], lens[i]
        s = P[starts[i]:starts[i] + L]
        blank = e if i % 11 == 3 else ""
        if fmt == "fastq":
            q = "@" + qual[:L - 1] if i % 5 == 0 else qual[:L]
            rec = f"{blank}@r{i} desc {i % 7}{e}{s}{e}{'+r%d' % i if i % 3 == 0 else '+'}{e}{q}{e}"
        else:
            width = (61, 70, 300)[i % 3]
            head = f"r{i} d>x{i} y" if i % 4 == 0 else f"r{i} some words"
            rec = f"{blank}>{head}{e}{e.join(s[j:j + width] for j in range(0, L, width))}{e}"
        out.append(rec)
        size += len(rec)
    text = "".join(out)
    assert len(text) >= BIG_BYTES
    return text


def prefix(fmt, n):
    """the first n bytes of big(fmt), the last one a line end (test_gpu_textparse.filler): the last record is cut anywhere"""
    text = big(fmt)[:n - 1] + "\n"
    assert len(text) == n
    return text


def titles_at(data, pos, length):
    """the bytes of all titles, one after the other"""
    length = length.astype(np.int64)
    pos = pos.astype(np.int64)
    assert ((pos >= 0) & (pos + length <= data.size)).all()
    within = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(np.cumsum(length) - length, length)
    return data[np.repeat(pos, length) + within].tobytes()


def same_records(data, bases, offsets, title_pos, title_len, want, seq=1):
    """the raw arrays of a parse against the model's records [(title, seq, ...)]: no Python string per record"""
    R = len(want)
    assert len(title_len) == R and len(offsets) == R + 1
    joined = "".join(w[seq] for w in want).encode("latin-1")
    lens = np.fromiter((len(w[seq]) for w in want), np.int64, R)
    assert np.array_equal(offsets.astype(np.int64), np.concatenate([[0], np.cumsum(lens)]))
    assert bases.tobytes() == joined
    same_titles(data, title_pos, title_len, [w[0] for w in want])


def same_titles(data, title_pos, title_len, titles):
    assert np.array_equal(title_len.astype(np.int64), np.fromiter((len(t) for t in titles), np.int64, len(titles)))
    assert titles_at(np.frombuffer(data, np.uint8), title_pos, title_len) == "".join(titles).encode("latin-1")


def check_raw(st, text, fmt, final=True, want=None, consumed=None):
    data = text.encode("latin-1")
    o = st.parse_text_raw(data, fmt, final)
    want = MODEL[fmt](text) if want is None else want
    assert (o["R"], o["n_bases"]) == (len(want), sum(len(s) for _, s in want))
    same_records(data, o["bases"], o["offsets"], o["title_pos"], o["title_len"], want)
    assert o["consumed"] == (len(text) if consumed is None else consumed)
    return want


# ---- 1. the size ladder -------------------------------------------------------------------------------------------------------------
# (n, the tiles of a FASTQ text of n bytes, the tiles of a final FASTA text: one more position, so n = SB * T is already SB + 1 tiles
#  and n = G * T already G + 1)
LADDER = [(SB * T - 1, SB, SB), (SB * T, SB, SB + 1), (SB * T + 1, SB + 1, SB + 1), (SB * T + T + 17, SB + 2, SB + 2),
          (G * T - 1, G, G), (G * T, G, G + 1), (G * T + 1, G + 1, G + 1), (G * T + T + 5, G + 2, G + 2),
          ((2 * G + 1) * T + 3, 2 * G + 2, 2 * G + 2)]   # the last: block 0 takes a third tile
# the texts of SB * T + 1, G * T + 1 and the largest size without their final line end: one byte fewer
LADDER_BARE = [(SB * T, SB, SB + 1), (G * T, G, G + 1), ((2 * G + 1) * T + 2, 2 * G + 2, 2 * G + 2)]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("n,fq_tiles,fa_tiles", LADDER, ids=[str(n) for n, _, _ in LADDER])
def test_size_ladder(st, fmt, n, fq_tiles, fa_tiles):
    text = prefix(fmt, n)
    assert tiles(len(text), fmt) == (fq_tiles if fmt == "fastq" else fa_tiles)
    want = check_raw(st, text, fmt)
    assert len(want) > n // 500


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("n,fq_tiles,fa_tiles", LADDER_BARE, ids=[str(n) for n, _, _ in LADDER_BARE])
def test_size_ladder_without_the_final_line_end(st, fmt, n, fq_tiles, fa_tiles):
    text = prefix(fmt, n + 1)[:-1]
    assert len(text) == n and text[-1] not in "\r\n" and tiles(n, fmt) == (fq_tiles if fmt == "fastq" else fa_tiles)
    check_raw(st, text, fmt)


# Where the cut of the generated text falls inside a title line, the last position of a size decides nothing: a pass that left out
# the one tile more would go unnoticed.  So every size again with a record that is decided by the text's last byte -- FASTA: its only
# base, which the end of the text closes; FASTQ: the '+' that makes it a record, a line start of its own.
LAST_RECORD = {"fastq": "\n@z\nA\n+", "fasta": "\n>z\nA"}


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("n,fq_tiles,fa_tiles", LADDER, ids=[str(n) for n, _, _ in LADDER])
def test_size_ladder_record_on_the_last_byte(st, fmt, n, fq_tiles, fa_tiles):
    end = LAST_RECORD[fmt]
    text = prefix(fmt, n - len(end) + 1)[:-1] + end
    assert len(text) == n and tiles(n, fmt) == (fq_tiles if fmt == "fastq" else fa_tiles)
    want = check_raw(st, text, fmt)
    assert want[-1] == ("z", "A")


# ---- 2. markers on the new borders --------------------------------------------------------------------------------------------------
SEQ = "ACGTTGCA"
# test_gpu_textparse.test_markers_on_tile_wave_and_lane_borders: (what ends at the border B, what starts there)
PIECES = {"fastq": [("@h\r", "\n" + SEQ + "\n+\nIIIIIIII\n"),                 # \r | \n
                    ("", "@h\n" + SEQ + "\n+\nIIIIIIII\n"),                   # | @ at a line start
                    ("@h\n" + SEQ + "\n", "+\nIIIIIIII\n"),                   # | + at a line start
                    ("@h\n" + SEQ + "\r", "\n+\r\nIIIIIIII\r\n"),
                    ("@h\n" + SEQ + "\n+\nIIIIIIII\n@", "g\n" + SEQ + "\n+\nII\n")],   # @ | title
          "fasta": [(">h\r", "\n" + SEQ + "\n"), ("", ">h\n" + SEQ + "\n"), (">h\n" + SEQ + "\n", ">g\nAC\n"), (">h x", ">y\n" + SEQ + "\n"),
                    (">h\n" + SEQ, "\n" + SEQ + "\n>"), (">h\n", SEQ + "\n")]}
BORDERS = [SB * T,          # the first byte of tile 1024
           (SB + 1) * T,    # inside a scan part of two tiles
           G * T,           # the first byte of a block's second round
           (G + 1) * T, 2 * G * T]
MARKER_CASES = [(fmt, B, k) for fmt in ("fastq", "fasta") for B in BORDERS for k in range(len(PIECES[fmt]))]


@functools.lru_cache(maxsize=2)
def head_of(fmt, B):
    return big(fmt)[:B]


@pytest.mark.parametrize("fmt,B,k", MARKER_CASES, ids=[f"{fmt}-{B // T}T-{k}" for fmt, B, k in MARKER_CASES])
def test_markers_on_scan_and_grid_borders(st, fmt, B, k):
    left, right = PIECES[fmt][k]
    head = head_of(fmt, B)[:B - len(left) - 1] + "\n"
    text = head + left + right
    # at least 2G + 1 tiles where the border is a block's later round, at least SB + 2 otherwise
    floor = 2 * G * T + 1 if B >= G * T else (SB + 1) * T + 1
    text += prefix(fmt, max(40, floor - len(text)))
    assert text[B - len(left):B] == left and text[B:B + len(right)] == right
    assert tiles(len(text), fmt) >= (2 * G + 1 if B >= G * T else SB + 2) and B % T == 0 and B // T in (SB, SB + 1, G, G + 1, 2 * G)
    check_raw(st, text, fmt)


# ---- 3. one record over many scan parts ---------------------------------------------------------------------------------------------
def long_seq(n):
    P = pool()
    return (P * (n // len(P) + 1))[:n]


def in_lines(seq, width=61, eol="\n"):
    return eol.join(seq[i:i + width] for i in range(0, len(seq), width))


@pytest.mark.parametrize("one_line", [False, True], ids=["61_columns", "one_line"])
def test_fasta_record_over_many_scan_parts(st, one_line):
    seq = long_seq((SB + 6) * T)
    body = seq if one_line else in_lines(seq)
    text = f">short d\nAC\n>genome of many tiles\n{body}\n>after\r\nGT\r\n"
    assert tiles(len(text), "fasta") > SB + 6   # the last '>', terminator and kept byte are carried over more than SB tiles
    want = check_raw(st, text, "fasta")
    assert want == [("short", "AC"), ("genome", seq), ("after", "GT")]


def test_fasta_bare_lines_before_the_first_record(st):
    bare = in_lines(long_seq((SB + 500) * T), 70) + "\n"
    text = bare + ">a b\nACGT\nTT\n>c>d\nGG\n" + prefix("fasta", 3000)
    assert len(bare) > (SB + 500) * T and tiles(len(text), "fasta") > SB + 500
    want = check_raw(st, text, "fasta")
    assert len(want[0][1]) == (SB + 500) * T - 70 and want[1] == ("a", "ACGTTT")   # (the first bare line is the piece's title line)


# (SB + 6) * T bases: with the quality line more than G tiles, every block's second round lies inside one line;
# (G + 6) * T bases: more than 2G tiles, a third round
@pytest.mark.parametrize("tiles_of_bases,floor", [(SB + 6, G), (G + 6, 2 * G)], ids=["over_G_tiles", "over_2G_tiles"])
def test_fastq_read_over_many_scan_parts(st, tiles_of_bases, floor):
    seq = long_seq(tiles_of_bases * T)
    text = f"@long read\n{seq}\n+\n{'I' * len(seq)}\n@b x\r\nACGT\r\n+\r\nIIII\r\n@c\nGG\n+c\n@I\n"
    assert tiles(len(text), "fastq") > floor
    want = check_raw(st, text, "fastq")
    assert want == [("long", seq), ("b", "ACGT"), ("c", "GG")]


def test_fasta_chunk_ends_inside_a_long_record(st):
    done = ">r1 d\nACGT\nTT\n>r2\r\nGG\r\n>r3>r3b\nAC\n"
    body = in_lines(long_seq((SB + 6) * T))[:(SB + 6) * T - len(">long one\n")]
    chunk = done + ">long one\n" + body
    at = len(done)
    assert len(chunk) - at == (SB + 6) * T and body[-1] not in "\r\n" and tiles(len(chunk), "fasta", final=False) > SB + 6
    first = MODEL["fasta"](done)
    assert len(first) == 3
    check_raw(st, chunk, "fasta", final=False, want=first, consumed=at)   # the '>' of the record that is not finished
    carry = chunk[at:]
    fourth = check_raw(st, carry, "fasta")
    assert len(fourth) == 1 and first + fourth == MODEL["fasta"](chunk)


@pytest.mark.parametrize("mark,skip", [("\r\n", 1), ("\n@r", 2), ("\n+r", 3)], ids=["inside_crlf", "after_the_at", "inside_the_plus_line"])
def test_fastq_chunk_of_two_grids_ends_inside_a_marker(st, mark, skip):
    src = big("fastq")
    cut = src.index(mark, 2 * G * T + 1) + skip
    text = src[:cut + 1500] + "\n"
    assert tiles(cut, "fastq", final=False) > 2 * G and text[cut - skip:cut - skip + len(mark)] == mark
    assert parse_chunked(st, text, "fastq", [cut]) == MODEL["fastq"](text)


# ---- 4. many lines ------------------------------------------------------------------------------------------------------------------
LINE_COUNTS = [(SB * LB, SB),               # nlt = 1024: the last count one scan thread per line tile serves
               (SB * LB + 1, SB + 1),       # a scan thread folds two line tiles, the count comes from the device
               (G * LB, G),
               (G * LB + 1, G + 1),         # the first stride round of the line tiles
               (2 * G * LB + 300, 2 * G + 2)]


@functools.lru_cache(maxsize=None)
def tiny_records():
    """records of four short lines, sequences of 0 .. 3 bases"""
    P = pool()
    out = []
    for i in range(2 * G * LB // 4 + 100):
        L = (i * 7 + i // 5) % 4
        e = "\r\n" if i % 13 == 0 else "\n"
        out.append(f"@{i % 1000}{e}{P[i:i + L]}{e}+{e}{'I' * L}{e}")
    return out


@functools.lru_cache(maxsize=2)
def many_lines(M):
    """exactly M lines: tiny records, and blank lines in the middle and at the end"""
    recs = tiny_records()
    k = (M - 50) // 4
    blanks = M - 4 * k
    return "".join(recs[:k // 2]) + "\n" * (blanks // 2) + "".join(recs[k // 2:k]) + "\n" * (blanks - blanks // 2)


@pytest.mark.parametrize("M,line_tiles", LINE_COUNTS, ids=[str(M) for M, _ in LINE_COUNTS])
def test_many_lines(st, M, line_tiles):
    text = many_lines(M)
    assert len(model_lines(text)) == M and -(-M // LB) == line_tiles
    want = check_raw(st, text, "fastq")
    assert len(want) == (M - 50) // 4 and any(not s for _, s in want)


@pytest.mark.parametrize("M,line_tiles", [(SB * LB + 3, SB + 1), (G * LB + 3, G + 1)], ids=["scan_part_of_two", "second_round"])
def test_record_in_the_line_tile_past_the_border(st, M, line_tiles):
    """One line past SB * LB or G * LB cannot start a record: it has no line j + 2.  Three can: the lines of the last line tile are the
    '@', sequence and '+' line of a record, the only one that the scan's second tile of a part, or the second round of block 0, holds."""
    text = many_lines(M - 3) + "@z x\nA\n+"
    lines = model_lines(text)
    assert len(lines) == M and -(-M // LB) == line_tiles and lines[(line_tiles - 1) * LB:] == ["@z x", "A", "+"]
    want = check_raw(st, text, "fastq")
    assert len(want) == (M - 53) // 4 + 1 and want[-1] == ("z", "A")


@pytest.mark.parametrize("unit,count,floor", [("\n", 600_000, G * LB), ("\r", 600_000, G * LB), ("\r\n", 300_000, SB * LB)],
                         ids=["lf", "cr", "crlf"])
def test_every_byte_a_line(st, unit, count, floor):
    """the largest line-start table the scratch sizing allows per byte of text"""
    text = unit * count
    assert len(model_lines(text)) == count > floor
    assert check_raw(st, text, "fastq") == []
    assert check_raw(st, text, "fasta") == []


def test_capacity_past_one_grid_of_line_tiles(st):
    """test_gpu_textparse.test_capacity on the text of G * LB + 1 lines"""
    M = G * LB + 1
    text = many_lines(M)
    assert len(model_lines(text)) == M and -(-M // LB) > G
    data = text.encode()
    want = MODEL["fastq"](text)
    R, nb = len(want), sum(len(s) for _, s in want)
    guard = 64
    exact = st.parse_text_raw(data, "fastq", True, bases_capacity=nb, records_capacity=R, guard=guard)
    assert (exact["R"], exact["n_bases"], exact["consumed"]) == (R, nb, len(text))
    same_records(data, exact["bases"], exact["offsets"], exact["title_pos"], exact["title_len"], want)
    for key in ("raw_bases", "raw_title_pos", "raw_title_len", "raw_offsets"):
        assert (exact[key][-guard:].view(np.uint8) == 0xA5).all(), key
    for bcap, rcap in ((nb - 1, R), (nb, R - 1)):
        with pytest.raises(capi.SlackenError) as e:
            st.parse_text_raw(data, "fastq", True, bases_capacity=bcap, records_capacity=rcap, guard=guard)
        assert e.value.code == capi.E_CAPACITY
        part = e.value.partial
        assert (part["R"], part["n_bases"]) == (R, nb)   # the true counts: what the capacities would have to be
        for key in ("raw_bases", "raw_title_pos", "raw_title_len"):
            assert (part[key].view(np.uint8) == 0xA5).all(), key   # nothing written, the guard elements included
        assert (part["raw_offsets"][1:].view(np.uint8) == 0xA5).all()
    check_raw(st, text, "fastq", want=want)   # the stream stays usable


# ---- 5. pairs past one grid ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def numbered(M, suffix, bad=()):
    """the titles of test_gpu_pairparse.numbered, the sequences (1 .. 19 bases) sliced from the pool"""
    P = pool()
    shift = 7 * int(suffix[-1])   # (mates of other lengths and other bases)
    return [(f"read.{i}{'#' if i in bad else ''} d{suffix}" if i % 2 else f"read.{i}{'#' if i in bad else ''}{suffix}",
             P[(i + 100 * shift) % 60000:(i + 100 * shift) % 60000 + 1 + (i * 5 + i // 3 + shift) % 19]) for i in range(M)]


@functools.lru_cache(maxsize=6)
def mate_text(fmt, M, suffix, bad=()):
    text = render(fmt, numbered(M, suffix, bad))
    return text, MODEL[fmt](text)


def whole_raw(st, side1, side2):
    """test_gpu_pairparse.whole on the raw arrays: both texts final, against the lockstep of the model's records"""
    (fmt1, (text1, rec1)), (fmt2, (text2, rec2)) = side1, side2
    d1, d2 = text1.encode(), text2.encode()
    o = st.parse_text_paired_raw(d1, fmt1, True, d2, fmt2, True)
    want, P, mismatch = lockstep(rec1, rec2)
    assert (o["R1"], o["R2"], o["P"], o["mismatch"]) == (len(rec1), len(rec2), P, mismatch)
    # where either text's next chunk starts: at the opener of record P, which every title line of these texts names once
    for i, (text, recs, fmt) in enumerate(((text1, rec1, fmt1), (text2, rec2, fmt2))):
        mark = "@" if fmt == "fastq" else ">"
        at = len(text) if len(recs) <= P else 0 if P == 0 else text.index(f"\n{mark}{recs[P][0]}") + 1
        assert o[f"consumed{i + 1}"] == at, i
    assert (o["n_bases"], o["n_mate_bases"]) == (sum(len(w[1]) for w in want), sum(len(w[2]) for w in want))
    same_records(d1, o["bases"], o["offsets"], o["title_pos"][:P], o["title_len"][:P], want, seq=1)
    mates = np.frombuffer("".join(w[2] for w in want).encode(), np.uint8)
    assert np.array_equal(o["mate_bases"], mates)
    assert np.array_equal(o["mate_offsets"].astype(np.int64), np.concatenate([[0], np.cumsum([len(w[2]) for w in want], dtype=np.int64)]))
    same_titles(d1, o["title_pos"], o["title_len"], [strip(t, "/1") for t, _ in rec1])   # all R1 records, stripped
    return o


PAIR_COUNTS = [G * LB,        # the last count one round of the compare pass serves
               G * LB + 1,    # block 0 takes a second round of one record
               600_000]


@pytest.mark.parametrize("M", PAIR_COUNTS)
def test_mates_past_one_grid(st, M):
    side1 = ("fastq", mate_text("fastq", M, "/1"))
    assert len(side1[1][1]) == M
    o = whole_raw(st, side1, ("fastq", mate_text("fastq", M, "/2")))
    assert (o["P"], o["mismatch"]) == (M, False)
    if M == G * LB + 1:
        o = whole_raw(st, side1, ("fasta", mate_text("fasta", M, "/2")))
        assert (o["P"], o["mismatch"]) == (M, False)


@pytest.mark.parametrize("M,bad", [(G * LB + 1, (G * LB - 1,)),       # the last record of the first round
                                   (G * LB + 1, (G * LB,)),           # the one record of the second round
                                   (600_000, (599_999,)),
                                   (600_000, (10, G * LB + 70)),      # two: one in the second round inside a full wave, one earlier
                                   (G * LB + 1, (10, G * LB))],       # ... and the later one alone in its wave
                         ids=["last_of_round_1", "first_of_round_2", "last_record", "two_full_wave", "two_alone_in_its_wave"])
def test_planted_mismatch_past_one_grid(st, M, bad):
    assert M > G * LB and max(bad) < M and (len(bad) == 1 or max(bad) >= G * LB)
    o = whole_raw(st, ("fastq", mate_text("fastq", M, "/1")), ("fastq", mate_text("fastq", M, "/2", bad)))
    assert (o["P"], o["mismatch"]) == (min(bad), True)


@pytest.mark.parametrize("longer", [1, 2])
def test_surplus_past_one_grid(st, longer):
    M, surplus = G * LB + 1, 300
    counts = (M + surplus, M) if longer == 1 else (M, M + surplus)
    o = whole_raw(st, ("fastq", mate_text("fastq", counts[0], "/1")), ("fastq", mate_text("fastq", counts[1], "/2")))
    assert (o["P"], o["mismatch"], o["R1"], o["R2"]) == (M, False, counts[0], counts[1])
    assert len(o["title_len"]) == counts[0] > G * LB   # the surplus titles come back too


# ---- 6. through classification ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", [False, True], ids=["hits", "merged_hits"])
def test_classify_text_of_more_than_one_grid(small_k, merged):  # noqa: F811
    rng = np.random.default_rng(41)
    genome = small_k["genome"].tobytes().decode()
    n_reads = (G + 2) * T // 90
    lens, starts = rng.integers(21, 61, n_reads).tolist(), rng.integers(0, len(genome) - 60, n_reads).tolist()
    text = "".join(f"@q{i} x\n{genome[a:a + L]}\n+\n{'I' * L}\n" for i, (a, L) in enumerate(zip(starts, lens)))
    assert len(text) > (G + 1) * T and tiles(len(text), "fastq") > G + 1
    model = MODEL["fastq"](text)
    assert len(model) == n_reads > 32768
    bases = np.frombuffer("".join(q for _, q in model).encode(), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(q) for _, q in model])]).astype(np.uint64)
    s = small_k["st"]
    s.set_merged_hits(merged)
    try:
        thr = (0.0, 0.15)
        want = s.classify_batch(bases, offsets, thresholds=thr, with_hits=True, with_num_hits=True)
        got = s.classify_text(text.encode(), "fastq", thresholds=thr, with_hits=True)
    finally:
        s.set_merged_hits(False)
    assert got["R"] == len(model) and got["consumed"] == len(text)
    assert got["titles"] == [t for t, _ in model]
    assert np.array_equal(got["offsets"], offsets)
    for key in ("taxon", "classified", "num_distinct", "total_kmers"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["hit_offsets"], want["hit_offsets"]) and np.array_equal(got["hits"], want["hits"])
    assert want["classified"].any() and (got["num_hits"] > 0).any()


# ---- 7. the command line at its default chunk ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "gz", "crlf"])
def test_parse_device_at_the_default_chunk(tmp_path, form):
    """20 MiB: two chunks of the default size with their carries (more than G tiles each) and a rest; then chunks 1.5 times as large"""
    n = (20 << 20) + 5
    text = prefix("fastq", BIG_BYTES) + prefix("fastq", n - BIG_BYTES)
    if form == "crlf":
        text = text.replace("\r\n", "\n").replace("\r", "\n").replace("\n", "\r\n")
    data = text.encode()
    assert len(data) >= 20 << 20 and (8 << 20) == G * T
    path = tmp_path / ("reads.fastq.gz" if form == "gz" else "reads.fastq")
    path.write_bytes(gzip.compress(data, 1) if form == "gz" else data)
    want = cli("parse", path)
    assert want.count("\n") > n // 400
    assert cli("parse", "--device", path) == want   # SLK_IO_CHUNK unset: chunks of 8 MiB
    assert cli("parse", "--device", path, env={"SLK_IO_CHUNK": "12582912"}) == want
