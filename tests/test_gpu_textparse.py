"""FASTA / FASTQ text parsed on the device (slacken_amd/csrc/textparse.hip: slk_parse_text, slk_parse_device, slk_classify_text)
against the host rules as tests/hostmodel.py restates them (parse_fasta, parse_fastq; FileInputs.scala:155-221): crafted texts, tile,
wave and lane borders, the chunk contract (every split position, with the carry the caller owes), fuzz, capacities, and
classify_text against classify_batch on the model's records."""
import json
import os

import numpy as np
import pytest

import hostmodel
from test_host_cli import FASTA, FASTQ

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL = {"fasta": hostmodel.parse_fasta, "fastq": hostmodel.parse_fastq}


@pytest.fixture(scope="module")
def st():
    import slacken_amd
    ix = slacken_amd.Index(expected_records=1024)   # (a stream belongs to an index; the parser needs nothing of it)
    s = ix.stream()
    yield s
    s.close()
    ix.close()


@pytest.fixture(scope="module")
def T():
    from slacken_amd import capi
    t = capi.parse_tile_bytes()
    assert t >= 1024 and t % 1024 == 0   # whole waves of 16-byte lanes
    return t


def parse(st, text, fmt, final=True):
    titles, seqs, consumed = st.parse_text(text.encode("latin-1"), fmt, final)
    return list(zip(titles, seqs)), consumed


def check(st, text, fmt):
    got, consumed = parse(st, text, fmt)
    want = MODEL[fmt](text)
    assert got == want, (fmt, text[:200])
    assert consumed == len(text)
    return want


def parse_chunked(st, text, fmt, cuts):
    """The records of the calls a caller makes who receives the text cut at `cuts`: text[consumed, n) of every chunk goes in front of
    the next one, the last call is final."""
    out, carry, pos = [], "", 0
    for c in cuts:
        chunk = carry + text[pos:c]
        pos = c
        recs, consumed = parse(st, chunk, fmt, final=False)
        assert 0 <= consumed <= len(chunk)
        out += recs
        carry = chunk[consumed:]
    recs, consumed = parse(st, carry + text[pos:], fmt, final=True)
    assert consumed == len(carry) + len(text) - pos
    return out + recs


SEPARATED = [FASTA, FASTQ, FASTA.replace("\r\n", "\n").replace("\n", "\r\n"), FASTQ.replace("\n", "\r\n"),
             FASTA.replace("\r\n", "\n").replace("\n", "\r"), FASTQ.replace("\n", "\r"), FASTA.rstrip("\n"), FASTQ.rstrip("\n")]


@pytest.mark.parametrize("i", range(len(SEPARATED)))
def test_host_cli_fixtures(st, i):
    text = SEPARATED[i]
    fmt = "fastq" if text.startswith("@") else "fasta"
    assert len(check(st, text, fmt)) >= 3


CRAFTED_FASTQ = [
    "@a\nACGT\n+\n@III\n@b\nGG\n+\nII\n",                  # a quality line that starts with '@' ...
    "@a\nACGT\n+\n@qual\nXX\n+\nII\n",                      # ... followed two lines later by a '+' line: a record on the host too
    "@a\n\n+\n\n@b\n\n+\n\n",                               # empty sequence lines
    "@a\nACGT\n", "@a\nACGT", "@a", "@a\n", "", "\n", "\r", "\r\n", "+\n+\n+\n", "@\n@\n+\n+\n",   # fewer than three lines, and degenerate ones
    "@a\nAC\n+\nII\n\n\n@b\nGT\n+\nII\n\n",               # empty lines between records
    "\n\n@a x y\nAC\n+\nII", "@a\r\rAC\r+\r", "@a\r\n\r\nAC\r\n+\r\n", "@ lead\nAC\n+\n", "@a\nA C\n+ x\n",
]
CRAFTED_FASTA = [
    ">a>b\nACGT\n>c d>e\nGG\n",                             # '>' inside a header
    "ACGT\nGG\n>a\nTT\n", "x y\nACGT\n>a\nTT",              # text before the first '>'
    ">only\n>b\nAC\n>last", ">only", ">only\n", ">\n", ">", "",   # header-only records
    "\n>a\nAC\n", "\nACGT\n>a\nAC\n", "\r\n\r\n>a\r\nAC",   # a leading empty line
    ">a\n\r\n\rAC\r\r\n\nGT\n\r>b \n\n\rTT\r", ">a\r\n\n\n", "> t\nA\n>\nC\n>  \nG\n",   # runs of mixed \n and \r
]


@pytest.mark.parametrize("fmt,texts", [("fastq", CRAFTED_FASTQ), ("fasta", CRAFTED_FASTA)])
def test_crafted(st, fmt, texts):
    for text in texts:
        check(st, text, fmt)
        check(st, text + text, fmt)


def test_fasta_record_of_three_tiles(st, T):
    rng = np.random.default_rng(5)
    seq = "".join(rng.choice(list("ACGT"), size=3 * T + 11))
    lines = "\n".join(seq[i:i + 61] for i in range(0, len(seq), 61))
    want = check(st, f">short\nAC\n>genome of three tiles\n{lines}\n>after\nGT\n", "fasta")
    assert want[1] == ("genome", seq)
    check(st, f">one line\n{seq}", "fasta")
    check(st, f"@longread\n{seq}\n+\n{'I' * len(seq)}\n", "fastq")


def filler(fmt, n, rng):
    """n bytes of ordinary records (n >= 0), ending with a line end"""
    out = []
    size = 0
    while size < n:
        s = "".join(rng.choice(list("ACGTN"), size=int(rng.integers(1, 90))))
        rec = f"@r{len(out)} d\n{s}\n+\n{'I' * len(s)}\n" if fmt == "fastq" else f">r{len(out)} d\n{s}\n"
        out.append(rec)
        size += len(rec)
    text = "".join(out)[:n]
    return text[:-1] + "\n" if text else text


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_text_sizes_around_the_tile(st, T, fmt):
    rng = np.random.default_rng(9)
    for n in (T - 1, T, T + 1, 2 * T + 17, 16, 15, 17, 1023, 1024, 1025):
        text = filler(fmt, n, rng)
        assert len(text) == n
        check(st, text, fmt)
        check(st, text[:-1], fmt)   # ... and without the final line end


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_markers_on_tile_wave_and_lane_borders(st, T, fmt):
    """A \\r\\n, an '@' line start, a '+' line start and a '>' placed so that the border B falls between their two bytes / right before
    them, for B = the tile's, a wave's (1024 bytes) and a lane's (16 bytes) border."""
    rng = np.random.default_rng(13)
    seq = "ACGTTGCA"
    pieces = {"fastq": [("@h\r", "\n" + seq + "\n+\nIIIIIIII\n"),                 # \r | \n
                        ("", "@h\n" + seq + "\n+\nIIIIIIII\n"),                   # | @ at a line start
                        ("@h\n" + seq + "\n", "+\nIIIIIIII\n"),                   # | + at a line start
                        ("@h\n" + seq + "\r", "\n+\r\nIIIIIIII\r\n"),
                        ("@h\n" + seq + "\n+\nIIIIIIII\n@", "g\n" + seq + "\n+\nII\n")],   # @ | title
              "fasta": [(">h\r", "\n" + seq + "\n"), ("", ">h\n" + seq + "\n"), (">h\n" + seq + "\n", ">g\nAC\n"), (">h x", ">y\n" + seq + "\n"),
                        (">h\n" + seq, "\n" + seq + "\n>"), (">h\n", seq + "\n")]}[fmt]
    for B in (T, 2 * T, 1024, T + 1024, 16, T + 16, 1024 + 16):
        for left, right in pieces:
            head = filler(fmt, B - len(left), rng) if B > len(left) else ""
            if len(head) + len(left) != B:
                continue
            text = head + left + right + filler(fmt, 40, rng)
            assert text[B - len(left):B] == left
            check(st, text, fmt)
            check(st, text.rstrip("\n"), fmt)


CONTRACT = {
    "fastq": ("@r1 d\nACGT\n+\nIIII\n@r2\r\nGG\r\n+\r\nII\r\n@r3\rTTTT\r+r3\r@III\r\n\n@r4\n\n+\n\n@q\n@AC\n+\n+II\n"
              "@r5 a b\nACGTACGTAC\n+\n@@@@@@@@@@\n\r\n\r@r6\nNNNN\n+\nIIII\r" + "@r7\nACGTTGCAAC\n+\nIIIIIIIIII\n" * 10 + "@r8\nAC\n+\nII"),
    "fasta": ("pre text\nACGT\n>r1 d\nACGT\nTTGG\n>r2\r\nGG\r\nCC\r\n>only\n>r3\rTTTT\rAA\r>a>b\nAC\n>\nGT\n\n\r\n>r4 x y\n\nAC\n\n"
              "> lead\nTT\n>r5\n\r\n\rAC\r\r\n\nGT\n\r" + ">r6 d\nACGTTGCAAC\nACGT\n" * 13 + ">r7\nAC"),
}


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_chunk_contract_every_split(st, fmt):
    text = CONTRACT[fmt]
    assert 350 <= len(text) <= 450 and all(t in text for t in ("\r\n", "\n\n", "\r@" if fmt == "fastq" else "\r>"))
    want = MODEL[fmt](text)
    assert len(want) >= 15
    for p in range(len(text) + 1):
        assert parse_chunked(st, text, fmt, [p]) == want, p
    rng = np.random.default_rng(21)
    for _ in range(50):
        a, b = sorted(int(v) for v in rng.integers(0, len(text) + 1, 2))
        assert parse_chunked(st, text, fmt, [a, b]) == want, (a, b)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_fuzz(st, T, fmt):
    alphabet = list("ACGTN@+> \n\r")
    # (record marks, spaces and line ends weighted down on every other seed, so that long lines and long records occur as well)
    rare = np.array([8, 8, 8, 8, 4, 1, 1, 1, 1, 2, 1], float)
    for seed in range(300):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(0, 3 * T + 1)) if seed % 3 else int(rng.integers(0, 200))
        text = "".join(rng.choice(alphabet, size=n, p=rare / rare.sum() if seed % 2 else None))
        want = check(st, text, fmt)
        cuts = sorted(int(v) for v in rng.integers(0, n + 1, int(rng.integers(1, 4))))
        assert parse_chunked(st, text, fmt, cuts) == want, (seed, cuts)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_capacity(st, fmt):
    from slacken_amd import capi
    text = {"fastq": FASTQ, "fasta": FASTA}[fmt] * 40
    want = MODEL[fmt](text)
    R, nb = len(want), sum(len(s) for _, s in want)
    G = 8
    exact = st.parse_text_raw(text.encode(), fmt, True, bases_capacity=nb, records_capacity=R, guard=G)
    assert (exact["R"], exact["n_bases"]) == (R, nb)
    assert exact["bases"].tobytes().decode() == "".join(s for _, s in want)
    for key in ("raw_bases", "raw_title_pos", "raw_title_len", "raw_offsets"):
        raw = exact[key]
        assert (raw[-G:].view(np.uint8) == 0xA5).all(), key
    for bcap, rcap in ((nb - 1, R), (nb, R - 1), (0, 0)):
        with pytest.raises(capi.SlackenError) as e:
            st.parse_text_raw(text.encode(), fmt, True, bases_capacity=bcap, records_capacity=rcap, guard=G)
        assert e.value.code == capi.E_CAPACITY
        part = e.value.partial
        assert (part["R"], part["n_bases"]) == (R, nb)   # what the capacities would have to be
        for key in ("raw_bases", "raw_title_pos", "raw_title_len"):
            assert (part[key].view(np.uint8) == 0xA5).all(), key   # nothing written, the guard elements included
        assert (part["raw_offsets"][1:].view(np.uint8) == 0xA5).all()
        assert parse(st, text, fmt)[0] == want   # the stream stays usable


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_parse_device_respects_capacities(st, fmt):
    """slk_parse_device with every array on the device (torch tensors) and guard elements behind the capacities"""
    import torch
    from slacken_amd import capi
    text = ({"fastq": FASTQ, "fasta": FASTA}[fmt] * 40).encode()
    want = MODEL[fmt](text.decode())
    R, nb = len(want), sum(len(s) for _, s in want)
    G = 16
    dev = torch.device("cuda:0")
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    for bcap, rcap, over in ((nb, R, 0), (nb - 1, R, 1), (nb, R - 1, 1)):
        bases = torch.full((bcap + G,), 0xA5, dtype=torch.uint8, device=dev)
        offsets = torch.full((rcap + 1 + G,), -1, dtype=torch.int64, device=dev)
        tpos = torch.full((rcap + G,), -1, dtype=torch.int64, device=dev)
        tlen = torch.full((rcap + G,), -1, dtype=torch.int32, device=dev)
        counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        rc = capi.lib().slk_parse_device(st.h, d_text.data_ptr(), len(text), capi._format(fmt), 1, bases.data_ptr(), bcap, offsets.data_ptr(),
                                         tpos.data_ptr(), tlen.data_ptr(), rcap, counts.data_ptr())
        assert rc == 0, capi.lib().slk_last_error()
        st.synchronize()
        assert counts.cpu().tolist() == [R, nb, 0 if over else len(text), over]
        assert (bases[bcap:].cpu() == 0xA5).all() and (offsets[rcap + 1:].cpu() == -1).all()
        assert (tpos[rcap:].cpu() == -1).all() and (tlen[rcap:].cpu() == -1).all()
        if over:
            assert (bases.cpu() == 0xA5).all() and (tpos.cpu() == -1).all() and (tlen.cpu() == -1).all() and (offsets.cpu() == -1).all()
        else:
            off = offsets[:R + 1].cpu().numpy()
            b = bases[:nb].cpu().numpy().tobytes().decode()
            assert [b[off[r]:off[r + 1]] for r in range(R)] == [s for _, s in want]


@pytest.mark.parametrize("merged", [False, True], ids=["hits", "merged_hits"])
def test_classify_text_equals_classify_batch(merged):
    import slacken_amd
    g = json.load(open(os.path.join(GOLD, "golden_classify.json")))
    lib = np.load(os.path.join(GOLD, "library.npz"))
    reads = [line.rstrip("\n").split("\t") for line in open(os.path.join(GOLD, "reads.tsv"))]
    ix = slacken_amd.Index(k=g["k"], m=g["m"], spaces=g["spaces"], expected_records=len(lib["keys"]), max_taxon=len(lib["parents"]) - 1)
    ix.append(lib["keys"], lib["taxa"])
    ix.set_taxonomy(lib["parents"])
    ix.finalize()
    s = ix.stream()
    s.set_merged_hits(merged)
    texts = {"fasta": "".join(f">{t} length={len(q)}\n{q[:60]}\n{q[60:]}\r\n" for t, q in reads),
             "fastq": "".join(f"@{t} x\n{q}\n+\n{'I' * len(q)}\n" for t, q in reads)}
    thr = (0.0, 0.15, 0.5)
    for fmt, text in texts.items():
        model = MODEL[fmt](text)
        assert [(t, q) for t, q in model] == [(t, q) for t, q in reads]
        bases = np.frombuffer("".join(q for _, q in model).encode(), np.uint8)
        offsets = np.cumsum([0] + [len(q) for _, q in model]).astype(np.uint64)
        for with_hits in (True, False):
            want = s.classify_batch(bases, offsets, thresholds=thr, with_hits=with_hits, with_num_hits=True)
            got = s.classify_text(text.encode(), fmt, thresholds=thr, with_hits=with_hits)
            assert got["R"] == len(model) and got["consumed"] == len(text)
            assert got["titles"] == [t for t, _ in model]
            assert np.array_equal(got["offsets"], offsets)
            for key in ("taxon", "classified", "num_distinct", "total_kmers"):
                assert np.array_equal(got[key], want[key]), (fmt, key)
            if with_hits:
                assert np.array_equal(got["hit_offsets"], want["hit_offsets"]) and np.array_equal(got["hits"], want["hits"])
                assert (got["num_hits"] > 0).any()
    # a chunk of a longer text: the records it takes, and where the next chunk starts
    text = texts["fastq"]
    cut = len(text) // 2
    got = s.classify_text(text[:cut].encode(), "fastq", final=False, thresholds=thr)
    whole = s.classify_text(text.encode(), "fastq", thresholds=thr)
    assert 0 < got["R"] < whole["R"] and 0 < got["consumed"] < cut and text[got["consumed"] - 1] == "\n"
    assert np.array_equal(got["taxon"], whole["taxon"][:, :got["R"]])
    rest = s.classify_text(text[got["consumed"]:].encode(), "fastq", thresholds=thr)
    assert got["R"] + rest["R"] == whole["R"] and np.array_equal(rest["taxon"], whole["taxon"][:, got["R"]:])
    s.close()
    ix.close()


@pytest.mark.parametrize("with_hits", [False, True], ids=["rows", "hits"])
def test_classify_text_reruns_a_batch_whose_taxon_map_overflows(orc, with_hits):
    """slk_classify_text on a text with one record of more than 128 distinct taxa: the batch is classified again by the unbounded
    kernels (status bit 1) before its rows come down -- every record against the oracle."""
    import manytaxa
    import synth
    w = manytaxa.world(orc, 4200)
    reads = w["reads"]
    bases, offsets = synth.pack(reads)
    want = orc.classify_batch(w["p"], w["oix"], w["parents"], bases, offsets, thresholds=manytaxa.THR)
    text = "".join(f"@r{i}\n{r.tobytes().decode()}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads))
    got = w["st"].classify_text(text.encode(), "fastq", thresholds=manytaxa.THR, with_hits=with_hits)
    assert got["R"] == len(reads) and got["consumed"] == len(text) and np.array_equal(got["offsets"], offsets)
    manytaxa.check(orc, w, got, want, with_hits, reads)
