"""The join of `compare` on the device (slacken_amd/csrc/compare.hip: slk_compare_*) through the binding and the command line,
against tests/compare_model.py: chunk seams at every position, lines and ids around the tile borders, colliding hashes, ids that are
prefixes of one another, growth from nothing, duplicates, bad lines, the pair counts' three levels, and `slacken-amd compare` on what
`classify` wrote.  Every comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import compare_model as cm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")


@pytest.fixture(scope="module")
def st():
    import slacken_amd
    ix = slacken_amd.Index(expected_records=1024)   # (a stream belongs to an index; the join needs nothing of it)
    s = ix.stream()
    yield s
    s.close()
    ix.close()


def handle(st, **env):
    """a fresh handle; the switches are read at create"""
    import slacken_amd
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return slacken_amd.Compare(stream=st)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def model(ref, test, id_col=2, taxon_col=3):
    rows, (read, dropped) = cm.reference_rows(ref, id_col, taxon_col)
    pairs, ref_taxa, n_test, n_joined = cm.join(rows, cm.kraken_rows(test))
    return sorted((r, t, n) for (r, t), n in pairs.items()), sorted(ref_taxa.items()), (read, dropped, len(rows), n_test, n_joined)


def result(c):
    r, t, n = c.pairs()
    taxa, rows = c.reference_taxa()
    return ([(int(a), int(b), int(k)) for a, b, k in zip(r, t, n)], [(int(a), int(k)) for a, k in zip(taxa, rows)], c.totals())


def feed(add, text, cuts=()):
    """the calls of a caller who receives the text cut at `cuts`: what a call did not consume goes in front of the next chunk"""
    carry, pos = b"", 0
    for cut in cuts:
        chunk = carry + text[pos:cut]
        pos = cut
        consumed = add(chunk, final=False)
        assert 0 <= consumed <= len(chunk)
        carry = chunk[consumed:]
    last = carry + text[pos:]
    assert add(last, final=True) == len(last)


def joined(st, ref, test, ref_cuts=(), test_cuts=(), id_col=2, taxon_col=3, **env):
    c = handle(st, **env)
    feed(lambda t, final: c.add_reference(t, id_col, taxon_col, final), ref, ref_cuts)
    c.begin_test()
    feed(c.add_test, test, test_cuts)
    got = result(c)
    c.close()
    return got


@pytest.mark.parametrize("eol", [b"\n", b"\r\n", b"\r"])
def test_whole_texts(st, eol):
    rng = np.random.default_rng(len(eol))
    ref, test = cc.case(rng, 2000, 1700, 300, eol=eol)
    ref, test = eol + ref[:-len(eol)], test + eol + eol           # empty lines, a last line without terminator
    want = model(ref, test)
    assert want[2][1] > 0 and want[2][4] == 1700
    assert joined(st, ref, test) == want


def test_chunk_seams(st):
    rng = np.random.default_rng(17)
    ids = cc.read_ids(rng, 12)
    ref = cc.reference_text(rng, ids[:6], eol=b"\r\n") + cc.reference_text(rng, ids[6:], eol=b"\r") + b"\n" + cc.reference_text(rng, ["tail"])[:-1]
    back = [i[:-2] if i.endswith("/1") else i for i in ids] + ["tail", "absent"]
    test = (cc.classified_text(rng, back[:5], eol=b"\r\n", hits_len=(1, 2)) + b"\r\r" + cc.classified_text(rng, back[5:10], eol=b"\r", hits_len=(1, 2))
            + cc.classified_text(rng, back[10:], hits_len=(1, 2))[:-1])
    assert 300 <= len(ref) <= 520 and 300 <= len(test) <= 520, (len(ref), len(test))
    want = model(ref, test)
    assert want[2][2] == 13 and want[2][4] == 13 and joined(st, ref, test) == want
    for cut in range(len(ref) + 1):                                # the reference cut at every position
        assert joined(st, ref, test, ref_cuts=(cut,)) == want, cut
    c = handle(st)                                                 # the test text cut at every position, the reference resident
    c.add_reference(ref)
    for cut in range(len(test) + 1):
        c.begin_test()
        feed(c.add_test, test, (cut,))
        assert result(c) == want, cut
    for a, b in rng.integers(0, len(test) + 1, (50, 2)):           # ... and at 50 random pairs of positions
        c.begin_test()
        feed(c.add_test, test, sorted((int(a), int(b))))
        assert result(c) == want, (a, b)
    c.close()
    for a, b in rng.integers(0, len(ref) + 1, (50, 2)):
        assert joined(st, ref, test, ref_cuts=sorted((int(a), int(b)))) == want, (a, b)


MIN_LINE = 48


def lines_ending_at(rng, targets, make_line, eol):
    """lines whose terminators start at the given offsets (ascending, far apart), random lines between them; make_line(L) is a
    line of exactly L >= MIN_LINE bytes"""
    out = b""
    for t in targets:
        while t - len(out) > 2 * MIN_LINE + 40:
            out += make_line(MIN_LINE + int(rng.integers(0, 31))) + eol
        out += make_line(t - len(out)) + eol
        assert len(out) == t + len(eol)
    return out


def tile_id(n):
    return f"r{n}_" + "q" * (n * 7 % 23)                           # (a function of the row alone: both texts name the same reads)


@pytest.mark.parametrize("delta", [-1, 0, 1, -5, 12])
def test_tiles(st, delta):
    """Line ends -- in the reference text, whose id is the last column, id ends -- right below, on and above the multiples of the tile;
    the line behind such a line starts there, and the id of a test row two bytes further."""
    from slacken_amd import capi
    T = capi.parse_tile_bytes()
    rng = np.random.default_rng(100 + delta)
    n = [0]

    def ref_line(L):                                               # other columns than 2 and 3: taxon first, id fourth
        n[0] += 1
        head, rid = f"{int(rng.choice(cc.REF_TAXA))}\t", "\t-\t" + tile_id(n[0]) + ("/1" if n[0] % 3 == 0 else "")
        line = head + "p" * (L - len(head) - len(rid)) + rid
        assert len(line) == L
        return line.encode()

    def test_line(L):
        n[0] += 1
        head = f"C\t{tile_id(n[0])}\t{int(rng.choice(cc.TEST_TAXA))}\t100\t"
        line = head + "7" * (L - len(head))
        assert len(line) == L
        return line.encode()

    targets = [k * T + delta for k in (1, 2, 3)]
    for eol in (b"\n", b"\r\n", b"\r"):
        n[0] = 0
        ref = lines_ending_at(rng, targets, ref_line, eol) + b"22\t-\t-\tlongline" + eol + eol + b"23\t-\t-\ttailrow/1"   # an empty line, no terminator
        n[0] = 0
        test = lines_ending_at(rng, targets, test_line, eol)
        # a line longer than three tiles: a long hit-list column behind the id and the taxon, then rows behind it
        long_hits = " ".join(f"{int(t)}:{int(c)}" for t, c in zip(rng.choice(cc.TEST_TAXA, 2200), rng.integers(1, 99, 2200))).encode()
        assert len(long_hits) > 3 * T
        test += b"C\tlongline\t21\t100\t" + long_hits + eol + eol + b"C\tabsentrow\t20\t1\tz" + eol + b"C\ttailrow\t22\t1\tz"
        want = model(ref, test, 4, 1)
        assert want[2][4] > 50 and want[2][3] > want[2][4]
        assert joined(st, ref, test, id_col=4, taxon_col=1) == want, (delta, eol)
        # the same texts in chunks cut on and beside the tile borders
        cuts = [T - 1, T, T + 1, 2 * T, 3 * T + 7]
        assert joined(st, ref, test, ref_cuts=cuts, test_cuts=cuts, id_col=4, taxon_col=1) == want, (delta, eol)


def test_collisions(st):
    """SLK_COMPARE_HASH_BITS=2: four hash values for 3 000 ids -- every chain collides, only the bytes tell the ids apart"""
    rng = np.random.default_rng(23)
    ids = cc.read_ids(rng, 3000)
    ref = cc.reference_text(rng, ids)
    back = [i[:-2] if i.endswith("/1") else i for i in rng.permutation(ids)[:1500]] + [f"absent{j}" for j in range(500)]
    test = cc.classified_text(rng, list(rng.permutation(back)))
    want = model(ref, test)
    assert want[2][2] == 3000 and want[2][3:] == (2000, 1500)
    assert joined(st, ref, test, SLK_COMPARE_HASH_BITS=2) == want
    assert joined(st, ref, test, ref_cuts=(len(ref) // 3, len(ref) // 2), SLK_COMPARE_HASH_BITS=2) == want
    assert joined(st, ref, test) == want


@pytest.mark.parametrize("bits", [64, 2])
def test_prefixes_and_first_mates(st, bits):
    ids = ["read", "read1", "read12", "read123", "reae", "rea", "r", "read/1x", "x/1read/1", "mate/1", "ab/1cd", "//11", "same_length_a", "same_length_b",
           "a" * 40, "a" * 41, "a" * 39 + "b"]
    ref = "".join(f"x\t{rid}\t{20 + i}\n" for i, rid in enumerate(ids)).encode()
    rows, _ = cm.reference_rows(ref)
    assert rows[b"readx"] == 27 and rows[b"xread"] == 28 and rows[b"mate"] == 29 and rows[b"abcd"] == 30 and rows[b"/1"] == 31
    tests = ["read", "read1", "read12", "read123", "read1234", "rea", "re", "r", "reae", "reaf", "readx", "read/1x", "xread", "mate", "mate/1", "abcd",
             "ab/1cd", "/1", "//11", "same_length_a", "same_length_b", "same_length_c", "a" * 40, "a" * 41, "a" * 42, "a" * 39 + "b", "a" * 39 + "c"]
    test = "".join(f"C\t{tid}\t{i}\t1\tz\n" for i, tid in enumerate(tests)).encode()
    want = model(ref, test)
    joined_ids = {tests[t] for _, t, _ in want[0]}
    # an id that equals a reference id only after /1 removal does not match while it still carries /1
    assert {"mate", "abcd", "readx", "xread", "/1"} <= joined_ids and not {"mate/1", "ab/1cd", "read/1x", "//11"} & joined_ids
    assert want[2][4] == len(ids) == 17                           # every reference id is found, and nothing else
    assert joined(st, ref, test, SLK_COMPARE_HASH_BITS=bits) == want


def test_growth_from_nothing(st):
    rng = np.random.default_rng(31)
    ids = cc.read_ids(rng, 20000)
    ref = cc.reference_text(rng, ids, second_mates=False)
    test = cc.classified_text(rng, [i[:-2] if i.endswith("/1") else i for i in rng.permutation(ids)[:5000]], hits_len=(1, 2))
    want = model(ref, test)
    cuts = list(range(4096, len(ref), 4096))
    assert len(cuts) > 100
    got = joined(st, ref, test, ref_cuts=cuts, test_cuts=list(range(4096, len(test), 4096)))
    assert got == want and got[2][:3] == (20000, 0, 20000) and got[2][4] == 5000


def test_device_text(st):
    import torch
    rng = np.random.default_rng(37)
    ref, test = cc.case(rng, 3000, 2500, 200)
    want = model(ref, test)
    d_ref = torch.frombuffer(bytearray(ref), dtype=torch.uint8).cuda()
    d_test = torch.frombuffer(bytearray(test), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    c = handle(st)
    cut = c.add_reference_device(d_ref.data_ptr(), 4096 * 5, final=False)
    assert 0 < cut <= 4096 * 5
    tail = d_ref[cut:].clone()                                     # (a fresh allocation: aligned)
    torch.cuda.synchronize()
    assert c.add_reference_device(tail.data_ptr(), tail.numel()) == tail.numel()
    c.begin_test()
    assert c.add_test_device(d_test.data_ptr(), d_test.numel()) == d_test.numel()
    assert result(c) == want
    import slacken_amd
    with pytest.raises(slacken_amd.SlackenError) as e:
        c.add_test_device(d_test.data_ptr() + 1, 100)
    assert e.value.code == slacken_amd.E_INVALID
    c.close()


def error_of(st, ref, test=None, ref_cuts=(), test_cuts=()):
    import slacken_amd
    c = handle(st)
    with pytest.raises(slacken_amd.SlackenError) as e:
        feed(lambda t, final: c.add_reference(t, 2, 3, final), ref, ref_cuts)
        assert test is not None
        c.begin_test()
        feed(c.add_test, test, test_cuts)
    assert e.value.code == slacken_amd.E_INVALID
    err = c.error()
    with pytest.raises(slacken_amd.SlackenError):                  # the handle is spent
        c.begin_test()
    c.close()
    return err


def test_duplicates(st):
    from slacken_amd import capi
    rng = np.random.default_rng(41)
    ids = cc.read_ids(rng, 400)
    ref = cc.reference_text(rng, ids, second_mates=False)
    dup_id = ids[7][:-2] if ids[7].endswith("/1") else ids[7] + "/1"            # equal after /1 removal only
    dup = f"x\t{dup_id}\t21\tg\n".encode()
    first = ref.rfind(b"\n", 0, ref.index(f"\t{ids[7]}\t".encode())) + 1
    mid = ref.rfind(b"\n", 0, 3000) + 1                             # a line start behind the first occurrence
    assert first < mid
    inside = ref[:mid] + dup + ref[mid:]
    for text, cuts, second in ((inside, (), mid), (inside, (mid,), mid), (ref + dup, (len(ref),), len(ref)), (ref + dup, (100, 5000), len(ref))):
        with pytest.raises(cm.CompareError):
            cm.reference_rows(text)
        offset, kind = error_of(st, text, ref_cuts=cuts)
        assert kind == capi.COMPARE_DUPLICATE_REFERENCE and offset in (first, second), (offset, first, second)
    # a joined test id twice; an unjoined one twice is no error
    back = [i[:-2] if i.endswith("/1") else i for i in ids[:50]]
    test = cc.classified_text(rng, back + ["absent", "absent"], hits_len=(1, 2))
    assert joined(st, ref, test) == model(ref, test)
    again = f"C\t{back[3]}\t20\t1\tz\n".encode()
    where = [test.index(f"\t{back[3]}\t".encode()) - 1, len(test)]
    for cuts in ((), (len(test),), (40,)):
        offset, kind = error_of(st, ref, test + again, test_cuts=cuts)
        assert kind == capi.COMPARE_DUPLICATE_TEST and offset in where
    # with every chain colliding
    os.environ["SLK_COMPARE_HASH_BITS"] = "2"
    try:
        offset, kind = error_of(st, ref + dup)
        assert kind == capi.COMPARE_DUPLICATE_REFERENCE and offset in (first, len(ref))
    finally:
        del os.environ["SLK_COMPARE_HASH_BITS"]


BAD = [b"x\tr1", b"x\t\t3", b"x\tr1\t", b"x\tr1\t12x", b"x\tr1\t2147483648", b"x\tr1\t-1", b"x\tr1\t3 ", b"x\tr1\t+", b"\tr1", b"x\tr1\t99999999999999999999"]


def test_bad_lines(st):
    from slacken_amd import capi
    rng = np.random.default_rng(43)
    good = cc.reference_text(rng, cc.read_ids(rng, 300), second_mates=False)
    head = good[:len(good) // 2].rsplit(b"\n", 1)[0] + b"\n"
    tail = good[len(head):]
    for bad in BAD:
        # two offending lines: the lowest is reported
        offset, kind = error_of(st, head + bad + b"\n" + tail + BAD[0] + b"\n")
        assert (offset, kind) == (len(head), capi.COMPARE_BAD_LINE), bad
        with pytest.raises(cm.CompareError) as e:
            cm.reference_rows(head + bad + b"\n" + tail)
        assert (e.value.kind, e.value.offset) == (cm.BAD_LINE, len(head))
        test = b"C\tq\t20\t1\tz\n" * 3 + bad.replace(b"x", b"C", 1) + b"\r\n" + b"C\tq\t20\t1\tz\n" * 50 + b"C\tonly-two\n"
        offset, kind = error_of(st, good, test, test_cuts=(20,))
        assert (offset, kind) == (33, capi.COMPARE_BAD_LINE), bad
    # Java's parseInt takes a sign: +7 is 7, -0 is 0; the largest int
    ref = b"x\ta\t+7\nx\tb\t-0\nx\tc\t2147483647\nx\td\t007\n"
    want = model(ref, b"C\ta\t+20\t1\tz\nC\tb\t-0\t1\tz\nU\tc\t0\nC\td\t2147483647\n")
    assert want[0] == [(0, 0, 1), (7, 20, 1), (7, 2147483647, 1), (2147483647, 0, 1)] and want[1] == [(0, 1), (7, 2), (2147483647, 1)]
    assert joined(st, ref, b"C\ta\t+20\t1\tz\nC\tb\t-0\t1\tz\nU\tc\t0\nC\td\t2147483647\n") == want


def test_pair_counting(st):
    rng = np.random.default_rng(47)
    ids = [f"read{i}" for i in range(9000)]
    # one pair for all rows
    ref = "".join(f"x\t{i}\t21\n" for i in ids).encode()
    test = "".join(f"C\t{i}\t20\t1\tz\n" for i in ids[:7000]).encode()
    assert joined(st, ref, test) == ([(21, 20, 7000)], [(21, 9000)], (9000, 0, 9000, 7000, 7000))
    # more distinct pairs than a block's LDS map holds (2048 slots), in two blocks: 70 x 70 pairs, some of them hot
    ids = [f"read{i}" for i in range(30000)]
    ref = "".join(f"x\t{i}\t{int(rng.integers(0, 70)) if k % 3 else 5}\n" for k, i in enumerate(ids)).encode()
    test = "".join(f"C\t{i}\t{int(rng.integers(0, 70)) if k % 2 else 9}\t1\tz\n" for k, i in enumerate(ids)).encode()
    want = model(ref, test)
    assert len(want[0]) > 2500
    assert joined(st, ref, test, SLK_COMPARE_BLOCKS=2) == want
    assert joined(st, ref, test) == want
    # two tests on one resident reference: the second carries nothing of the first
    c = handle(st, SLK_COMPARE_BLOCKS=2)
    c.add_reference(ref)
    other = "".join(f"C\t{i}\t{int(rng.integers(100, 130))}\t1\tz\n" for i in ids[4000:4600]).encode()
    for text in (test, other, test):
        c.begin_test()
        c.add_test(text)
        assert result(c) == model(ref, text)
    c.begin_test()                                                 # a test without rows
    assert result(c) == ([], want[1], (30000, 0, 30000, 0, 0))
    c.close()


def test_capacity_query_and_an_empty_handle(st):
    import ctypes as C
    import slacken_amd
    L = slacken_amd.lib()
    c = handle(st)
    assert result(c) == ([], [], (0, 0, 0, 0, 0)) and c.error() == (0, 0)
    c.begin_test()
    assert c.add_test(b"C\tq\t20\t1\tz\n") == 11 and c.add_test(b"") == 0      # a test without a reference joins nothing
    assert result(c) == ([], [], (0, 0, 0, 1, 0))
    c.add_reference(b"x\ta\t3\nx\tb\t4\n")
    c.begin_test()
    c.add_test(b"C\ta\t1\nC\tb\t2\n")
    n = C.c_uint64(0)
    a, b = np.zeros(1, np.int32), np.zeros(1, np.int32)
    k = np.zeros(1, np.uint64)
    assert L.slk_compare_pairs(c.h, C.byref(n), a.ctypes.data, b.ctypes.data, k.ctypes.data, 1) == -5 and n.value == 2      # SLK_E_CAPACITY
    assert (int(a[0]), int(b[0]), int(k[0])) == (3, 1, 1)
    assert c.add_reference(b"x\tc\t5", final=False) == 0           # no whole line: the chunk must grow
    with pytest.raises(slacken_amd.SlackenError):
        c.add_reference(b"x\tc\t5\n", id_col=2, taxon_col=2)
    assert result(c)[2] == (2, 0, 2, 2, 2)
    c.close()


# ---- the command line, end to end ----
def run(*args, **env):
    r = subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, env={**os.environ, **env})
    assert r.returncode == 0, r.stderr
    return r


def test_cli_on_what_classify_wrote(tmp_path):
    from test_host_classify_gpu import make_library
    g, loc, _, reads = make_library(tmp_path)
    tax_dir = loc + "_taxonomy"
    tax = cm.Taxonomy.load(tax_dir)
    rng = np.random.default_rng(53)
    called = {r["title"]: r["c0.0"][0] for r in g["reads"] if r["c0.0"][1]}
    defined = [t for t in range(2, tax.size) if tax.is_defined(t)]
    samples = ["s1", "s2", "s3", "s4"]
    fq = tmp_path / "reads.fq"
    with open(fq, "w") as f:                                       # 4 x 562 reads
        for s in samples:
            for t, seq in reads:
                f.write(f"@{s}_{t}\n{seq}\n+\n{'I' * len(seq)}\n")
    for s in samples:                                              # the truth: mostly what the classifier would call, some of it wrong
        os.makedirs(tmp_path / "truth" / f"sample{s}")
        with open(tmp_path / "truth" / f"sample{s}" / "reads_mapping.tsv", "w") as f:
            f.write("#anonymous_read_id\tread_id\ttax_id\n")
            for i, (t, _) in enumerate(reads[:-20]):               # (the last reads are not in the truth)
                taxon = called[t] if t in called and rng.random() < 0.8 else int(rng.choice(defined))
                f.write(f"a{i}\t{s}_{t}/1\t{taxon}\n" f"a{i}\t{s}_{t}/2\t{taxon}\n")
    out = tmp_path / "out" / "fam" / "grp" / "std_35_31_s7"
    run("classify", "-i", loc, "-o", out, "-c", "0.0", "0.15", "--sample-regex", "^(s[0-9]+)_", fq)
    os.rename(f"{out}_c0.15", f"{out}_c0.15_classified")           # the shape the reference's evaluation expects of a title
    dirs = [f"{out}_c0.00", f"{out}_c0.15_classified"]
    assert sorted(os.listdir(dirs[1]))[-4:] == [f"sample={s}" for s in samples]
    truth = str(tmp_path / "truth")
    args = ["compare", "-t", tax_dir, "-r", truth, "--header", "--multi-dirs"] + dirs
    dev = run(*args, "-o", tmp_path / "dev", SLK_COMPARE_CHUNK="30000")
    host = run(*args, "-o", tmp_path / "host", "--host")
    want_out, want_tsv = cm.run(tax_dir, truth, multi_dirs=dirs, header=True)
    assert dev.stdout == want_out == host.stdout
    assert (tmp_path / "dev_metrics.tsv").read_text() == want_tsv == (tmp_path / "host_metrics.tsv").read_text()
    rows = want_tsv.split("\n")[1:-1]
    assert len(rows) == 8 and rows[0].startswith("fam/grp/std_35_31_s7_c0.15_classified/sample=s1\tfam\tgrp\ts1\tstd\t35\t31\t0\t0\t7\t0.15\tGenus\t")
    assert want_out.count("Couldn't extract variables from filename: fam/grp/std_35_31_s7_c0.00/sample=") == 8
    assert "Total reads 0\n" not in want_out and "Classified 0 " not in want_out
    # one part file against one sample's truth
    part = os.path.join(dirs[0], "sample=s2", "part-00000.txt.gz")
    ref = os.path.join(truth, "samples2", "reads_mapping.tsv")
    dev = run("compare", "-t", tax_dir, "-r", ref, "--header", "-o", tmp_path / "one", "--test-files", part)
    host = run("compare", "-t", tax_dir, "-r", ref, "--header", "-o", tmp_path / "one_host", "--test-files", part, "--host")
    want_out, want_tsv = cm.run(tax_dir, ref, test_files=[part], header=True)
    assert dev.stdout == want_out == host.stdout and "Couldn't extract variables from filename: part-00000.txt.gz." in want_out
    assert (tmp_path / "one_metrics.tsv").read_text() == want_tsv == cm.HEADER + "\n"
    # a bad line ends the device's run too, naming file and line
    with gzip.open(tmp_path / "bad.txt.gz", "wb") as f:
        f.write(gzip.open(part).read() + b"C\tno-taxon\n")
    r = subprocess.run([CLI, "compare", "-t", tax_dir, "-r", ref, "--header", "-o", tmp_path / "bad", "--test-files", tmp_path / "bad.txt.gz"],
                       capture_output=True, text=True)
    n_lines = gzip.open(part).read().count(b"\n")
    assert r.returncode != 0 and f"bad.txt.gz line {n_lines + 1}: " in r.stderr and not os.path.exists(tmp_path / "bad_metrics.tsv")
