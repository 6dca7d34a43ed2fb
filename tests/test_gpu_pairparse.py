"""Two mate texts parsed and paired on the device (slacken_amd/csrc/textparse.hip: slk_parse_text_paired, slk_pair_device;
hostcalls.hip: slk_classify_text_paired) against the lockstep model (tests/pairparse_model.py) and the single-text device parser, which
tests/test_gpu_textparse.py pins: R_i and consumed_i of every call are checked against st.parse_text_raw of each text alone and the
opener positions its raw_title_pos gives."""
import json
import os

import numpy as np
import pytest

from pairparse_model import MODEL, lockstep, strip
from test_gpu_textparse import CONTRACT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMBOS = [("fastq", "fastq"), ("fasta", "fasta"), ("fasta", "fastq")]


@pytest.fixture(scope="module")
def st():
    import slacken_amd
    ix = slacken_amd.Index(expected_records=1024)   # (a stream belongs to an index; the parser needs nothing of it)
    s = ix.stream()
    yield s
    s.close()
    ix.close()


def render(fmt, records, eol="\n"):
    """records [(title line, seq)] as text"""
    if fmt == "fastq":
        return "".join(f"@{t}{eol}{s}{eol}+{eol}{'I' * len(s)}{eol}" for t, s in records)
    return "".join(f">{t}{eol}{s}{eol}" for t, s in records)


def opener(title_pos):
    return int(title_pos) - 1 if title_pos else 0


def paired(st, text1, fmt1, final1, text2, fmt2, final2):
    """One paired call, checked against the single-text parser of either side and the lockstep of what those parsers find.
    -> (the call's dict, [(title, seq, mate)])"""
    d1, d2 = text1.encode("latin-1"), text2.encode("latin-1")
    o = st.parse_text_paired_raw(d1, fmt1, final1, d2, fmt2, final2)
    single = [st.parse_text_raw(d, f, fin) for d, f, fin in ((d1, fmt1, final1), (d2, fmt2, final2))]
    recs = []
    for d, s in zip((d1, d2), single):
        off = s["offsets"]
        recs.append([(d[int(p):int(p) + int(l)].decode("latin-1"), s["bases"][int(off[r]):int(off[r + 1])].tobytes().decode("latin-1"))
                     for r, (p, l) in enumerate(zip(s["title_pos"], s["title_len"]))])
    want, P, mismatch = lockstep(recs[0], recs[1])
    assert (o["R1"], o["R2"]) == (single[0]["R"], single[1]["R"])
    assert (o["P"], o["mismatch"]) == (P, mismatch), (text1[:200], text2[:200])
    for i, (s, d) in enumerate(zip(single, (d1, d2))):
        consumed = opener(s["title_pos"][P]) if s["R"] > P else s["consumed"]
        assert o[f"consumed{i + 1}"] == consumed, (i, P, text1[:200], text2[:200])
        assert 0 <= consumed <= len(d)
    off, moff = o["offsets"], o["mate_offsets"]
    assert off[0] == 0 and moff[0] == 0 and o["n_bases"] == off[P] and o["n_mate_bases"] == moff[P]
    titles = [d1[int(p):int(p) + int(l)].decode("latin-1") for p, l in zip(o["title_pos"], o["title_len"])]
    assert titles == [strip(t, "/1") for t, _ in recs[0]]   # all R1 records, stripped
    got = [(titles[r], o["bases"][int(off[r]):int(off[r + 1])].tobytes().decode("latin-1"),
            o["mate_bases"][int(moff[r]):int(moff[r + 1])].tobytes().decode("latin-1")) for r in range(P)]
    assert got == want
    return o, got


def whole(st, text1, fmt1, text2, fmt2):
    """both texts final, against the model's parsers"""
    o, got = paired(st, text1, fmt1, True, text2, fmt2, True)
    want, P, mismatch = lockstep(MODEL[fmt1](text1), MODEL[fmt2](text2))
    assert got == want and (o["P"], o["mismatch"]) == (P, mismatch)
    return o


def title_of_length(rng, n):
    return "".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz0123456789.:_-"), size=n))


def title_cases():
    """[(title 1, title 2, mates?)]"""
    rng = np.random.default_rng(7)
    cases = [("a/1", "a/2", True), ("a", "a/2", True), ("a/1", "a", True), ("a", "a", True),
             ("a/2", "a/2", False), ("a/1", "a/1", False), ("a/1/1", "a/1/2", True), ("a/1/1", "a/2", False),
             ("/1", "/2", True), ("", "", True), ("/1", "", True), ("", "/2", True), ("/", "/", True), ("1", "2", False), ("/1", "/1", False)]
    for n in list(range(1, 71)) + [300]:
        t = title_of_length(rng, n)
        cases.append((t + "/1", t + "/2", True))
        cases.append((t, t, True))
        first = ("X" if t[0] != "X" else "Y") + t[1:]
        last = t[:-1] + ("X" if t[-1] != "X" else "Y")
        cases.append((t + "/1", first + "/2", False))   # only the first byte differs
        cases.append((t, last, False))                  # only the last byte
        cases.append((t, t + "x", False))               # only the length
        cases.append((t + "x/1", t, False))
    return cases


@pytest.mark.parametrize("fmt1,fmt2", COMBOS)
def test_title_table(st, fmt1, fmt2):
    rng = np.random.default_rng(11)
    seq = lambda: "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 40))))
    cases = title_cases()
    aligns = [set(), set()]
    for k, (t1, t2, mates) in enumerate(cases):
        desc = (" a description/1", " other words/2") if k % 2 else ("", "")   # (a title ends at the first space)
        lead = [(f"lead{j}", seq()) for j in range(k % 3)]
        r1 = lead + [(t1 + desc[0], seq()), ("tail/1", seq())]
        r2 = lead + [(t2 + desc[1], seq()), ("tail/2", seq())]
        if fmt1 == "fasta" and not t1 and not lead:
            continue   # (covered with a lead: an empty first title line is still a title)
        o, _ = paired(st, render(fmt1, r1), fmt1, True, render(fmt2, r2), fmt2, True)
        assert o["P"] == (len(lead) + 2 if mates else len(lead)) and o["mismatch"] == (not mates), (t1, t2)
    # every case again in ONE pair of texts, mates only: the lengths move both title positions through every 16-byte alignment
    good = [(t1, t2) for t1, t2, mates in cases if mates and (t1 or fmt1 == "fastq") and (t2 or fmt2 == "fastq")]
    r1 = [(t1, seq()) for t1, _ in good]
    r2 = [(t2, seq()) for _, t2 in good]
    text1, text2 = render(fmt1, r1), render(fmt2, r2)
    o = whole(st, text1, fmt1, text2, fmt2)
    assert o["P"] == len(good)
    for i, (text, fmt) in enumerate(((text1, fmt1), (text2, fmt2))):
        s = st.parse_text_raw(text.encode(), fmt, True)
        aligns[i] = {int(p) % 16 for p in s["title_pos"]}
    assert aligns[0] == set(range(16)) and aligns[1] == set(range(16))


def numbered(M, suffix, bad=()):
    rng = np.random.default_rng(M)
    return [(f"read.{i}{'#' if i in bad else ''} d{suffix}" if i % 2 else f"read.{i}{'#' if i in bad else ''}{suffix}",
             "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 20))))) for i in range(M)]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257, 513])
def test_borders_of_waves_and_blocks(st, M):
    r1 = numbered(M, "/1")
    text1 = render("fastq", r1)
    assert whole(st, text1, "fastq", render("fastq", numbered(M, "/2")), "fastq")["P"] == M
    for at in sorted({0, 63, 64, 255, 256, M - 1}):
        if at >= M:
            continue
        o = whole(st, text1, "fastq", render("fasta", numbered(M, "/2", bad=(at,))), "fasta")
        assert (o["P"], o["mismatch"]) == (at, True)
        if at + 70 < M:   # two planted mismatches, in another wave and in the same one: the smaller index wins
            for second in (at + 70, at + 1):
                o = whole(st, text1, "fastq", render("fastq", numbered(M, "/2", bad=(at, second))), "fastq")
                assert (o["P"], o["mismatch"]) == (at, True)


@pytest.mark.parametrize("surplus", [1, 300])
def test_surplus_on_either_side(st, surplus):
    for M in (0, 1, 64, 130):
        a, b = numbered(M + surplus, "/1"), numbered(M, "/2")
        o = whole(st, render("fastq", a), "fastq", render("fastq", b), "fastq")
        assert (o["P"], o["mismatch"], o["R1"], o["R2"]) == (M, False, M + surplus, M)
        assert o["consumed2"] == len(render("fastq", b))
        assert len(o["title_len"]) == M + surplus   # the surplus titles come back too
        a, b = numbered(M, "/1"), numbered(M + surplus, "/2")
        o = whole(st, render("fasta", a), "fasta", render("fastq", b), "fastq")
        assert (o["P"], o["mismatch"], o["R1"], o["R2"]) == (M, False, M, M + surplus)
        assert o["consumed1"] == len(render("fasta", a))


def test_text_ends(st):
    long_title = "a.title.of.23.bytes.xyz"
    assert len(long_title) == 23
    r1 = [("r0/1", "ACGT"), (long_title + "/1", "ACGTAC")]
    r2 = [("r0/2", "GG"), (long_title + "/2", "T")]
    for fmt2 in ("fastq", "fasta"):
        text1 = render("fastq", r1)[:-1]
        text2 = render(fmt2, r2)
        text2 = text2[:text2.rindex("T") + 1] if fmt2 == "fasta" else text2[:text2.rindex("+") + 1]   # the last title lies within 16 bytes of n2
        pos = text2.rindex(long_title)
        assert len(text2) - (pos + len(long_title) + 2) <= 16 and len(text1) % 16 and len(text2) % 16
        assert whole(st, text1, "fastq", text2, fmt2)["P"] == 2
        bad = text2[:pos + 22] + "Z" + text2[pos + 23:]   # ... and differs in its last byte
        assert whole(st, text1, "fastq", bad, fmt2)["P"] == 1
    text = render("fastq", r1)
    for final1 in (True, False):
        for final2 in (True, False):
            for t1, t2 in (("", text), (text, ""), ("", "")):
                o, got = paired(st, t1, "fastq", final1, t2, "fastq", final2)
                assert (o["P"], o["mismatch"], got) == (0, False, [])
                assert o["consumed1"] == 0 and o["consumed2"] == 0   # nothing is paired: either text starts at its first record again


def drive(st, text1, fmt1, text2, fmt2, cuts1, cuts2):
    """The pairs of the calls a caller makes who receives the texts cut at cuts1 / cuts2: text_i[consumed_i:] of every call goes in
    front of what arrives next, and the calls after the last piece are final on that side.  -> (pairs, mismatch)"""
    sides = [dict(text=text1, cuts=list(cuts1) + [len(text1)], pos=0, carry=""), dict(text=text2, cuts=list(cuts2) + [len(text2)], pos=0, carry="")]
    pairs = []
    for _ in range(len(text1) + len(text2) + 8):
        for s in sides:
            if s["cuts"]:
                c = s["cuts"].pop(0)
                s["carry"] += s["text"][s["pos"]:c]
                s["pos"] = c
        final = [not s["cuts"] for s in sides]
        o, got = paired(st, sides[0]["carry"], fmt1, final[0], sides[1]["carry"], fmt2, final[1])
        pairs += got
        if o["mismatch"]:
            return pairs, True
        consumed, R = (o["consumed1"], o["consumed2"]), (o["R1"], o["R2"])
        for s, c in zip(sides, consumed):
            assert 0 <= c <= len(s["carry"])
            s["carry"] = s["carry"][c:]
        if o["P"] == 0 and any(f and r == 0 for f, r in zip(final, R)):
            return pairs, False   # a final side is exhausted: the file pair is finished
        # progress, or a side that is not final has no record yet and must grow
        assert o["P"] > 0 or any(consumed) or any(not f and r == 0 for f, r in zip(final, R))
    raise AssertionError("the calls do not come to an end")


def mates_of(records, fmt2, rng, suffix="/2", eol="\n"):
    """a mate text for the records of text 1: the same titles, sequences of other lengths"""
    return render(fmt2, [(strip(t, "/1") + suffix, "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 12))))) for t, _ in records], eol)


@pytest.mark.parametrize("fmt1,fmt2", COMBOS)
def test_chunk_contract_every_split(st, fmt1, fmt2):
    rng = np.random.default_rng(31)
    text1 = CONTRACT[fmt1]
    records1 = MODEL[fmt1](text1)
    text2 = mates_of(records1, fmt2, rng, eol="\r\n" if fmt2 == "fasta" else "\n")
    assert 250 <= len(text2) <= 600 and len(records1) >= 15
    want, P, mismatch = lockstep(records1, MODEL[fmt2](text2))
    assert P == len(records1) and not mismatch
    # re-parsing from a record's opener yields the same records (both record rules are local)
    for text, fmt in ((text1, fmt1), (text2, fmt2)):
        s = st.parse_text_raw(text.encode("latin-1"), fmt, True)
        recs = MODEL[fmt](text)
        for r in range(0, s["R"], 3):
            assert MODEL[fmt](text[opener(s["title_pos"][r]):]) == recs[r:], (fmt, r)
    for p in range(len(text1) + 1):
        q = round(p * len(text2) / len(text1))
        assert drive(st, text1, fmt1, text2, fmt2, [p], [q]) == (want, False), (p, q)
    for _ in range(200):
        p, q = int(rng.integers(0, len(text1) + 1)), int(rng.integers(0, len(text2) + 1))
        assert drive(st, text1, fmt1, text2, fmt2, [p], [q]) == (want, False), (p, q)


@pytest.mark.parametrize("fmt1", ["fastq", "fasta"])
def test_fuzz(st, fmt1):
    alphabet = list("ACGTN@+> \n\r")
    rare = np.array([8, 8, 8, 8, 4, 1, 1, 1, 1, 2, 1], float)
    for seed in range(200):
        rng = np.random.default_rng(5000 + seed)
        n = int(rng.integers(0, 3000)) if seed % 3 else int(rng.integers(0, 200))
        text1 = "".join(rng.choice(alphabet, size=n, p=rare / rare.sum() if seed % 2 else None))
        records1 = MODEL[fmt1](text1)
        # text 2: the records of text 1 under their titles again (FASTA only where no title holds a '>')
        fmt2 = "fasta" if seed % 4 == 1 and not any(">" in t or not t for t, _ in records1) else "fastq"
        retitled = [(strip(t, "/1"), s) for t, s in records1]
        if seed % 5 == 0 and retitled:   # a planted disagreement
            j = int(rng.integers(0, len(retitled)))
            retitled[j] = (retitled[j][0] + "~", retitled[j][1])
        if seed % 7 == 0:   # a surplus
            retitled = retitled[:len(retitled) // 2] if seed % 2 else retitled + [("more", "AC")]
        text2 = mates_of(retitled, fmt2, rng, suffix="/2" if seed % 2 else "")
        want = lockstep(records1, MODEL[fmt2](text2))
        cuts1 = sorted(int(v) for v in rng.integers(0, len(text1) + 1, int(rng.integers(0, 3))))
        cuts2 = sorted(int(v) for v in rng.integers(0, len(text2) + 1, int(rng.integers(0, 3))))
        pairs, mismatch = drive(st, text1, fmt1, text2, fmt2, cuts1, cuts2)
        assert (pairs, mismatch) == (want[0], want[2]), (seed, cuts1, cuts2)


def test_capacity(st):
    from slacken_amd import capi
    r1, r2 = numbered(300, "/1"), numbered(290, "/2")
    r2 = [(t, s + "ACGT") for t, s in r2]
    d1, d2 = render("fastq", r1).encode(), render("fasta", r2).encode()
    R, nb = (len(r1), len(r2)), (sum(len(s) for _, s in r1), sum(len(s) for _, s in r2))
    G = 8
    exact = st.parse_text_paired_raw(d1, "fastq", True, d2, "fasta", True, bases_capacity=nb, records_capacity=R, guard=G)
    assert (exact["P"], exact["R1"], exact["R2"], exact["mismatch"]) == (290, 300, 290, False)
    assert exact["bases"].tobytes().decode() == "".join(s for _, s in r1[:290]) and exact["mate_bases"].tobytes().decode() == "".join(s for _, s in r2)
    for key in ("raw_bases", "raw_mate_bases", "raw_offsets", "raw_mate_offsets", "raw_title_pos", "raw_title_len"):
        assert (exact[key][-G:].view(np.uint8) == 0xA5).all(), key
    short = [((nb[0] - 1, nb[1]), R), ((nb[0], nb[1] - 1), R), (nb, (R[0] - 1, R[1])), (nb, (R[0], R[1] - 1)), ((0, 0), (0, 0))]
    for bcap, rcap in short:
        with pytest.raises(capi.SlackenError) as e:
            st.parse_text_paired_raw(d1, "fastq", True, d2, "fasta", True, bases_capacity=bcap, records_capacity=rcap, guard=G)
        assert e.value.code == capi.E_CAPACITY
        part = e.value.partial
        assert (part["R1"], part["R2"], part["n_bases"], part["n_mate_bases"]) == (R[0], R[1], nb[0], nb[1])   # what both sides need
        assert (part["P"], part["consumed1"], part["consumed2"]) == (0, 0, 0)
        for key in ("raw_bases", "raw_mate_bases", "raw_offsets", "raw_mate_offsets", "raw_title_pos", "raw_title_len"):
            assert (part[key].view(np.uint8) == 0xA5).all(), key   # nothing written, the guard elements included
        again = st.parse_text_paired_raw(d1, "fastq", True, d2, "fasta", True)   # the stream stays usable
        assert again["P"] == 290 and np.array_equal(again["bases"], exact["bases"])


def test_pair_device_on_resident_arrays(st):
    """slk_pair_device over the outputs of two slk_parse_device calls, every array on the device"""
    import torch
    from slacken_amd import capi
    r1, r2 = numbered(200, "/1"), numbered(150, "/2", bad=(97,))
    texts = [render("fastq", r1).encode(), render("fastq", r2).encode()]
    dev = torch.device("cuda:0")
    side = []
    for text in texts:
        n = len(text)
        t = dict(text=torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev), bases=torch.zeros(n, dtype=torch.uint8, device=dev),
                 offsets=torch.zeros(n // 2 + 3, dtype=torch.int64, device=dev), tpos=torch.zeros(n // 2 + 2, dtype=torch.int64, device=dev),
                 tlen=torch.zeros(n // 2 + 2, dtype=torch.int32, device=dev), counts=torch.zeros(4, dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        rc = capi.lib().slk_parse_device(st.h, t["text"].data_ptr(), n, capi.FORMAT_FASTQ, 1, t["bases"].data_ptr(), n, t["offsets"].data_ptr(),
                                         t["tpos"].data_ptr(), t["tlen"].data_ptr(), n // 2 + 2, t["counts"].data_ptr())
        assert rc == 0, capi.lib().slk_last_error()
        st.synchronize()
        t["R"] = int(t["counts"][0])
        side.append(t)
    assert (side[0]["R"], side[1]["R"]) == (200, 150)
    pair = torch.full((8 + 4,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    a, b = side
    rc = capi.lib().slk_pair_device(st.h, a["text"].data_ptr(), len(texts[0]), a["tpos"].data_ptr(), a["tlen"].data_ptr(), a["offsets"].data_ptr(),
                                    a["counts"].data_ptr(), a["R"], b["text"].data_ptr(), len(texts[1]), b["tpos"].data_ptr(), b["tlen"].data_ptr(),
                                    b["offsets"].data_ptr(), b["counts"].data_ptr(), b["R"], pair.data_ptr())
    assert rc == 0, capi.lib().slk_last_error()
    st.synchronize()
    got = pair.cpu().tolist()
    assert got[8:] == [-1] * 4
    tpos1, tpos2 = a["tpos"].cpu().numpy(), b["tpos"].cpu().numpy()
    assert got[:8] == [97, 1, int(tpos1[97]) - 1, int(tpos2[97]) - 1, 200, 150, int(a["offsets"][97]), int(b["offsets"][97])]
    tlen = a["tlen"].cpu().numpy()[:200]
    assert [texts[0][int(p):int(p) + int(l)].decode() for p, l in zip(tpos1[:200], tlen)] == [f"read.{i}" for i in range(200)]   # every "/1" is gone


@pytest.mark.parametrize("merged", [False, True], ids=["hits", "merged_hits"])
def test_classify_text_paired_equals_classify_batch(merged):
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
    halves = [(t, q[:len(q) // 2], q[len(q) // 2:]) for t, q in reads if len(q) >= 2]   # each read's second half is its mate
    r1 = [(f"{t}/1 length={len(a)}", a) for t, a, _ in halves]
    r2 = [(f"{t}/2", b) for t, _, b in halves]
    thr = (0.0, 0.15, 0.5)
    R = len(halves)
    bases = np.frombuffer("".join(a for _, a, _ in halves).encode(), np.uint8)
    offsets = np.cumsum([0] + [len(a) for _, a, _ in halves]).astype(np.uint64)
    mbases = np.frombuffer("".join(b for _, _, b in halves).encode(), np.uint8)
    moffsets = np.cumsum([0] + [len(b) for _, _, b in halves]).astype(np.uint64)
    want = {h: s.classify_batch(bases, offsets, mbases, moffsets, thresholds=thr, with_hits=h, with_num_hits=True) for h in (True, False)}
    assert (want[True]["num_hits"] > 0).any() and want[True]["classified"].any()

    def same(got, P, with_hits):
        w = want[with_hits]
        assert got["titles"][:P] == [t for t, _, _ in halves[:P]]
        assert np.array_equal(got["offsets"], offsets[:P + 1]) and np.array_equal(got["mate_offsets"], moffsets[:P + 1])
        for key in ("taxon", "classified"):
            assert np.array_equal(got[key], w[key][:, :P]), key
        for key in ("num_distinct", "total_kmers"):
            assert np.array_equal(got[key], w[key][:P]), key
        if with_hits:
            assert np.array_equal(got["hit_offsets"], w["hit_offsets"][:P + 1])
            assert np.array_equal(got["hits"], w["hits"][:int(w["hit_offsets"][P])])

    for fmt1, fmt2 in COMBOS:
        text1, text2 = render(fmt1, r1), render(fmt2, r2, "\r\n")
        assert lockstep(MODEL[fmt1](text1), MODEL[fmt2](text2))[0] == halves
        for with_hits in (True, False):
            got = s.classify_text_paired(text1.encode(), fmt1, True, text2.encode(), fmt2, True, thresholds=thr, with_hits=with_hits)
            assert (got["P"], got["R1"], got["R2"], got["mismatch"]) == (R, R, R, False)
            assert (got["consumed1"], got["consumed2"]) == (len(text1), len(text2))
            same(got, R, with_hits)
    text1, text2 = render("fastq", r1), render("fastq", r2)
    # chunks of longer texts: the pairs they take, and where the next chunks start
    cut1, cut2 = len(text1) // 2, len(text2) // 3
    got = s.classify_text_paired(text1[:cut1].encode(), "fastq", False, text2[:cut2].encode(), "fastq", False, thresholds=thr)
    P = got["P"]
    assert 0 < P < R and got["R1"] > P == got["R2"] and not got["mismatch"]
    same(got, P, True)
    assert text1[got["consumed1"]:].startswith("@" + r1[P][0]) and text2[got["consumed2"]:].startswith("@" + r2[P][0])
    rest = s.classify_text_paired(text1[got["consumed1"]:].encode(), "fastq", True, text2[got["consumed2"]:].encode(), "fastq", True, thresholds=thr)
    assert rest["P"] == R - P and np.array_equal(rest["taxon"], want[True]["taxon"][:, P:]) and np.array_equal(rest["hits"], want[True]["hits"][int(want[True]["hit_offsets"][P]):])
    # mates out of order: the pairs before, and the flag
    j = 2 * R // 3
    swapped = r2[:j] + [r2[j + 1], r2[j]] + r2[j + 2:]
    got = s.classify_text_paired(text1.encode(), "fastq", True, render("fastq", swapped).encode(), "fastq", True, thresholds=thr)
    assert (got["P"], got["mismatch"], got["R1"], got["R2"]) == (j, True, R, R)
    same(got, j, True)
    assert got["titles"][j] == halves[j][0] and text1[got["consumed1"]:].startswith("@" + r1[j][0])
    s.close()
    ix.close()


@pytest.mark.parametrize("with_hits", [False, True], ids=["rows", "hits"])
def test_classify_text_paired_reruns_a_batch_whose_taxon_map_overflows(orc, with_hits):
    """slk_classify_text_paired on texts with one pair of more than 128 distinct taxa: the batch is classified again by the unbounded
    kernels (status bit 1) before its rows come down -- every pair against the oracle."""
    import manytaxa
    import synth
    w = manytaxa.world(orc, 4300)
    both = w["reads"]
    reads, mates = [r[:len(r) // 2] for r in both], [r[len(r) // 2:] for r in both]     # each read's second half is its mate
    bases, offsets = synth.pack(reads)
    mb, mo = synth.pack(mates)
    want = orc.classify_batch(w["p"], w["oix"], w["parents"], bases, offsets, mb, mo, thresholds=manytaxa.THR)
    text1 = render("fastq", [(f"r{i}/1", r.tobytes().decode()) for i, r in enumerate(reads)])
    text2 = render("fastq", [(f"r{i}/2", r.tobytes().decode()) for i, r in enumerate(mates)])
    got = w["st"].classify_text_paired(text1.encode(), "fastq", True, text2.encode(), "fastq", True, thresholds=manytaxa.THR, with_hits=with_hits)
    assert (got["P"], got["mismatch"]) == (len(reads), False)
    assert np.array_equal(got["offsets"], offsets) and np.array_equal(got["mate_offsets"], mo)
    manytaxa.check(orc, w, got, want, with_hits, reads, mates)
