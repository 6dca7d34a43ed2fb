"""The host statement of `compare` (slacken_amd/host/compare.hpp: the lines, the fields, HostJoin, the metrics, Java's numbers):
compiled alone into a small program under AddressSanitizer and UBSan and compared with tests/compare_model.py on random inputs cut
into chunks of every size, then through `slacken-amd compare --host` on temporary trees in both layouts (no GPU is opened)."""
import bz2
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import compare_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")

MAIN = r"""
#include "compare.hpp"
#include <iostream>
using namespace slk_host;
// join TAXONOMY_DIR REFERENCE TEST ID_COL TAXON_COL HEADER CHUNK MULTI DATA_FILE: the join of two files by HostJoin, the text given in
//   chunks of CHUNK bytes; stdout: the location's report, then its two rows (or the complaints); a bad line or a duplicate: exit 3
//   and "kind offset" (the offset in the file: the header's bytes counted)
// numbers: stdin: doubles as hexadecimal bit patterns; stdout: Double.toString and formatPerc of each
// locate FILE OFFSET: the line number and the text of the line that starts there
int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "numbers") {
    std::string w;
    while (std::cin >> w) {
      const uint64_t bits = std::stoull(w, nullptr, 16);
      double d;
      memcpy(&d, &bits, 8);
      std::cout << java_double_string(d) << " " << (d >= 0 || std::isnan(d) ? java_format_perc(d) : std::string("-")) << "\n";
    }
    return 0;
  }
  if (mode == "locate" && argc == 4) {
    std::ifstream f(argv[2], std::ios::binary);
    std::string text;
    const uint64_t line = locate_line([&](char *dst, size_t cap) { f.read(dst, (std::streamsize)cap); return (size_t)f.gcount(); }, std::stoull(argv[3]), text);
    std::cout << line << "\t" << text << "\n";
    return 0;
  }
  if (mode != "join" || argc != 11) return 2;
  const Taxonomy tax = Taxonomy::load(argv[2]);
  const int id_col = atoi(argv[5]), taxon_col = atoi(argv[6]);
  const bool header = atoi(argv[7]) != 0, multi = atoi(argv[9]) != 0;
  const size_t chunk = (size_t)atol(argv[8]);
  HostJoin join;
  uint64_t skipped = 0;
  try {
    std::ifstream r(argv[3], std::ios::binary), t(argv[4], std::ios::binary);
    feed_text([&](char *dst, size_t cap) { r.read(dst, (std::streamsize)cap); return (size_t)r.gcount(); }, chunk, header,
              [&](const char *p, size_t n, bool final) {
                std::vector<char> exact(p, p + n);   // (exactly the chunk: a read past it is the sanitizer's to report)
                return join.add_reference(exact.data(), n, id_col, taxon_col, final);
              }, &skipped);
    skipped = 0;
    join.begin_test();
    feed_text([&](char *dst, size_t cap) { t.read(dst, (std::streamsize)cap); return (size_t)t.gcount(); }, chunk, false,
              [&](const char *p, size_t n, bool final) {
                std::vector<char> exact(p, p + n);
                return join.add_test(exact.data(), n, final);
              });
  } catch (const CompareTextError &e) {
    std::cout << e.kind << " " << e.offset + skipped << "\n";
    return 3;
  }
  const CompareCounts c = join.counts();
  LocationMetrics m;
  try {
    std::cout << location_report(tax, c, argv[10], multi, m);
  } catch (const std::runtime_error &e) {
    std::cout << "range\n";
    return 4;
  }
  for (int ri = 0; ri < 2; ri++) {
    std::string row;
    metrics_row(m, ri, row);
    std::cout << row << "\n";
  }
  std::cout << c.reference_rows << " " << c.dropped_second << " " << c.kept_ids << " " << c.test_rows << " " << c.joined_rows << "\n";
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("comparehost")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "comparer")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "slacken_amd", "host"), "-o", exe, str(d / "main.cpp")])
    return exe


@pytest.fixture(scope="module")
def tax_dir(tmp_path_factory):
    return cc.write_taxonomy(tmp_path_factory.mktemp("comparetax"))


def model_text(tax, ref, test, data_file, multi, id_col=2, taxon_col=3, header=False):
    rows, (read, dropped) = cm.reference_rows(ref, id_col, taxon_col, header)
    pairs, ref_taxa, n_test, n_joined = cm.join(rows, cm.kraken_rows(test))
    out, metrics = cm.location_metrics(tax, ref_taxa, pairs, data_file, multi)
    for title, rank, tm, rm in metrics:
        row, complaint = cm.metrics_row(title, rank, tm, rm)
        out.append(row or complaint)
    out.append(f"{read} {dropped} {len(rows)} {n_test} {n_joined}")
    return "".join(line + "\n" for line in out)


def run_join(prog, d, tax_dir, ref, test, chunk, data_file="part-0.txt", multi=False, id_col=2, taxon_col=3, header=False):
    (d / "ref.tsv").write_bytes(ref)
    (d / "test.tsv").write_bytes(test)
    return subprocess.run([prog, "join", tax_dir, str(d / "ref.tsv"), str(d / "test.tsv"), str(id_col), str(taxon_col), str(int(header)), str(chunk),
                           str(int(multi)), data_file], capture_output=True, text=True)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n", b"\r"])
@pytest.mark.parametrize("chunk", [1, 7, 64, 1 << 20])
def test_host_join_equals_the_model(prog, tax_dir, tmp_path, chunk, eol):
    rng = np.random.default_rng(chunk + len(eol))
    tax = cm.Taxonomy.load(tax_dir)
    ref, test = cc.case(rng, eol=eol)
    ref = ref[:-len(eol)]                                         # the last line without terminator
    test = eol + test + eol + eol                                 # empty lines
    title = "out/fam/grp/std_35_31_s7_c0.15_classified/sample=S0"
    for multi, data_file in ((False, "a/part-0.txt"), (True, title)):
        r = run_join(prog, tmp_path, tax_dir, ref, test, chunk, data_file, multi)
        assert r.returncode == 0, r.stderr
        assert r.stdout == model_text(tax, ref, test, data_file, multi)
    assert "\tfam\tgrp\tS0\tstd\t35\t31\t0\t0\t7\t0.15\tSpecies\t" in r.stdout and "Reference contains unknown taxon" in r.stdout


def test_columns_header_and_a_text_where_nothing_joins(prog, tax_dir, tmp_path):
    rng = np.random.default_rng(3)
    tax = cm.Taxonomy.load(tax_dir)
    ids = cc.read_ids(rng, 50)
    ref = b"\n#taxon\textra\tread\n" + b"".join(f"{int(rng.choice(cc.REF_TAXA))}\tx\t{i}\n".encode() for i in ids)
    test = cc.classified_text(rng, [i[:-2] if i.endswith("/1") else i for i in ids])
    for chunk in (5, 1 << 16):
        r = run_join(prog, tmp_path, tax_dir, ref, test, chunk, id_col=3, taxon_col=1, header=True)
        assert r.returncode == 0 and r.stdout == model_text(tax, ref, test, "part-0.txt", False, 3, 1, True)
    none = cc.classified_text(rng, [f"q{i}" for i in range(20)])
    for t in (none, b""):
        r = run_join(prog, tmp_path, tax_dir, ref, t, 64, id_col=3, taxon_col=1, header=True)
        assert r.returncode == 0 and r.stdout == model_text(tax, ref, t, "part-0.txt", False, 3, 1, True)
        assert "Total reads 0\nClassified 0 NaN%\n" in r.stdout and "PPV 0.00% Sensitivity NaN%" in r.stdout
    r = run_join(prog, tmp_path, tax_dir, b"", test, 64)
    assert r.returncode == 0 and r.stdout == model_text(tax, b"", test, "part-0.txt", False) and "Filtered reference size: 0\n" in r.stdout


BAD = [b"x\tr1", b"x\t\t3", b"x\tr1\t", b"x\tr1\t12x", b"x\tr1\t2147483648", b"x\tr1\t-1", b"x\tr1\t3 ", b"x\tr1\t+", b"\tr1"]


@pytest.mark.parametrize("chunk", [3, 1 << 16])
def test_bad_lines_duplicates_and_ranges(prog, tax_dir, tmp_path, chunk):
    good = b"x\tok\t20\nx\tok2/1\t+21\nx\tok2/2\t21\n"
    for bad in BAD:
        ref = good + bad + b"\n" + BAD[0] + b"\n"
        r = run_join(prog, tmp_path, tax_dir, ref, b"", chunk)
        assert (r.returncode, r.stdout) == (3, f"{cm.BAD_LINE} {len(good)}\n"), bad       # the lowest offending line
        test = b"C\tok\t20\t1\tz\n" + bad.replace(b"x", b"C", 1) + b"\n"
        r = run_join(prog, tmp_path, tax_dir, good, test, chunk)
        assert (r.returncode, r.stdout) == (3, f"{cm.BAD_LINE} 12\n"), bad
    # with a header the offset still counts the file's bytes
    r = run_join(prog, tmp_path, tax_dir, b"h\th\th\n" + good + BAD[0], b"", chunk, header=True)
    assert (r.returncode, r.stdout) == (3, f"{cm.BAD_LINE} {6 + len(good)}\n")
    r = run_join(prog, tmp_path, tax_dir, good + b"y\tok2\t22\n", b"", chunk)             # equal after /1 removal
    assert (r.returncode, r.stdout) == (3, f"{cm.DUPLICATE_REFERENCE} {len(good)}\n")
    test = b"C\tok\t20\nC\tnone\t20\nC\tnone\t20\nC\tok2\t20\nC\tok\t21\n"
    r = run_join(prog, tmp_path, tax_dir, good, test, chunk)
    assert (r.returncode, r.stdout) == (3, f"{cm.DUPLICATE_TEST} {len(test) - 8}\n")
    r = run_join(prog, tmp_path, tax_dir, good, test[:-8], chunk)                         # the unjoined id twice: no error
    assert r.returncode == 0 and "Total reads 2\n" in r.stdout
    for ref, test in ((good + b"x\tbig\t43\n", b""), (good, b"C\tok\t43\n")):
        assert run_join(prog, tmp_path, tax_dir, ref, test, chunk).returncode == 4
    assert run_join(prog, tmp_path, tax_dir, good, b"C\tabsent\t43\n", chunk).returncode == 0     # (only joined rows reach the taxonomy)


def test_java_numbers(prog):
    rng = np.random.default_rng(1)
    xs = [0.0, 0.5, 1.0, 1 / 3, 2 / 3, 0.001, 0.0009, 1.234e-5, 9999999.0, 1e7, 1.25e10, 123456.789, 8.4, 0.00125, 0.12345, 0.99995, 1e-3, 1e-4,
          12345678.9, 1.7976931348623157e308, math.nan, math.inf, -0.75, -math.inf, 2.5, 0.125, 0.375, 0.045, 1.005]
    xs += [float(a) / float(b) for a, b in zip(rng.integers(0, 1000, 300), rng.integers(1, 1000, 300))]
    xs += [float(v) for v in np.exp(rng.uniform(-40, 25, 200))]
    out = subprocess.run([prog, "numbers"], input="".join(np.float64(x).view(np.uint64).item().__format__("x") + "\n" for x in xs),
                         capture_output=True, text=True, check=True).stdout.split("\n")
    for x, line in zip(xs, out):
        want = cm.java_double(x) + " " + (cm.format_perc(x) if x >= 0 or x != x else "-")
        assert line == want, x


def test_locate_line(prog, tmp_path):
    text = b"a\r\nbb\rccc\n\nd\te\n"
    (tmp_path / "t").write_bytes(text)
    for offset, want in ((0, "1\ta"), (3, "2\tbb"), (6, "3\tccc"), (11, "5\td\te")):
        assert subprocess.run([prog, "locate", str(tmp_path / "t"), str(offset)], capture_output=True, text=True, check=True).stdout == want + "\n"


# ---- the command on temporary trees, --host ----
def run_cli(args, **env):
    return subprocess.run([CLI, "compare"] + [str(a) for a in args] + ["--host"], capture_output=True, text=True, env={**os.environ, **env})


def make_multi_tree(d, rng, eol=b"\n"):
    """two classification runs of three samples: D/fam/grp/std_35_31_s7_c<thr>_classified/sample=<id>/part-*, plain and .gz parts, files
    that do not count, and truth/sample<id>/reads_mapping.tsv"""
    dirs = []
    truth = {}
    for s in ("1", "2", "x=3"):
        ids = cc.read_ids(rng, 150, sample=f"S{s}")
        truth[s] = ids
        os.makedirs(d / "truth" / f"sample{s}")
        (d / "truth" / f"sample{s}" / "reads_mapping.tsv").write_bytes(b"#anonymous\tread\ttaxon\tgenome\n" + cc.reference_text(rng, ids, eol=eol))
    for thr in ("0.00", "0.15"):
        run = d / "out" / "fam" / "grp" / f"std_35_31_s7_c{thr}_classified"
        dirs.append(str(run))
        for s, ids in truth.items():
            sub = run / f"sample={s}"
            os.makedirs(sub)
            back = [i[:-2] if i.endswith("/1") else i for i in rng.permutation(ids)[:130]] + [f"other{j}" for j in range(15)]
            text = cc.classified_text(rng, back).split(b"\n")[:-1]
            (sub / "part-00000.txt").write_bytes(b"".join(line + eol for line in text[:60]))
            with gzip.open(sub / "part-00001.txt.gz", "wb") as f:
                f.write(b"".join(line + b"\n" for line in text[60:]))
            (sub / "_SUCCESS").write_bytes(b"")
            (sub / ".part-00000.txt.crc").write_bytes(b"not a line")
        os.makedirs(run / "reports")                              # a subdirectory that is no sample
        (run / "1_kreport.txt").write_text("not a directory")
    return dirs


@pytest.mark.parametrize("chunk", ["97", "0"])
def test_cli_host_multi_dirs(tmp_path, tax_dir, chunk):
    rng = np.random.default_rng(8)
    dirs = make_multi_tree(tmp_path, rng, eol=b"\r\n" if chunk == "97" else b"\n")
    args = ["-t", tax_dir, "-r", tmp_path / "truth", "-o", tmp_path / "eval" / "run", "--header", "--multi-dirs"] + dirs
    r = run_cli(args, SLK_COMPARE_CHUNK=chunk)
    assert r.returncode == 0, r.stderr
    want_out, want_tsv = cm.run(tax_dir, str(tmp_path / "truth"), multi_dirs=dirs, header=True)
    assert r.stdout == want_out
    assert (tmp_path / "eval" / "run_metrics.tsv").read_text() == want_tsv
    rows = want_tsv.split("\n")
    assert len(rows) == 1 + 2 * 3 * 2 + 1 and rows[1].split("\t")[:12] == [
        "fam/grp/std_35_31_s7_c0.00_classified/sample=1", "fam", "grp", "1", "std", "35", "31", "0", "0", "7", "0.00", "Genus"]
    assert "sample=x=3\tfam\tgrp\tx=3\t" in want_tsv and "Couldn't extract" not in want_out


def test_cli_host_test_files(tmp_path, tax_dir):
    rng = np.random.default_rng(9)
    ref, test = cc.case(rng)
    (tmp_path / "truth.tsv.gz").write_bytes(gzip.compress(ref))
    (tmp_path / "part-0.txt").write_bytes(test)
    (tmp_path / "part-1.txt.bz2").write_bytes(bz2.compress(cc.classified_text(rng, ["nothing", "joins"])))
    os.makedirs(tmp_path / "dir")
    (tmp_path / "dir" / "b.txt").write_bytes(test[:len(test) // 2].rsplit(b"\n", 1)[0] + b"\n")
    (tmp_path / "dir" / "a.txt.gz").write_bytes(gzip.compress(cc.classified_text(rng, ["more", "others"])))
    files = [str(tmp_path / "part-0.txt"), str(tmp_path / "part-1.txt.bz2"), str(tmp_path / "dir")]
    r = run_cli(["-t", tax_dir, "-r", tmp_path / "truth.tsv.gz", "-o", tmp_path / "o", "--test-files"] + files)
    assert r.returncode == 0, r.stderr
    want_out, want_tsv = cm.run(tax_dir, str(tmp_path / "truth.tsv.gz"), test_files=files)
    assert r.stdout == want_out and (tmp_path / "o_metrics.tsv").read_text() == want_tsv == cm.HEADER + "\n"
    assert r.stdout.count("Couldn't extract variables from filename: ") == 6 and r.stdout.count("Filtered reference size: ") == 3
    # other columns: the same mapping with its columns moved
    moved = b"".join(b"\t".join((f[2], b"-", b"-", f[1])) + b"\n" for f in (line.split(b"\t") for line in ref.split(b"\n")[:-1]))
    (tmp_path / "moved.tsv").write_bytes(moved)
    r2 = run_cli(["-t", tax_dir, "--reference", tmp_path / "moved.tsv", "--output", tmp_path / "o2", "--id-col", "4", "-T", "1", "--noheader",
                  "--test-files", files[0]])
    assert r2.returncode == 0 and r2.stdout == cm.run(tax_dir, str(tmp_path / "truth.tsv.gz"), test_files=files[:1])[0]


def test_cli_errors_name_file_and_line(tmp_path, tax_dir):
    good = b"x\tok\t20\nx\tok2/1\t21\n"
    (tmp_path / "ref.tsv").write_bytes(b"header\n" + good + b"x\tr1\t12x\n")
    (tmp_path / "t.txt").write_bytes(b"C\tok\t20\n")
    base = ["-t", tax_dir, "-o", tmp_path / "o"]
    r = run_cli(base + ["-r", tmp_path / "ref.tsv", "--header", "--test-files", tmp_path / "t.txt"])
    assert r.returncode != 0 and "ref.tsv line 4: " in r.stderr and not os.path.exists(tmp_path / "o_metrics.tsv")
    (tmp_path / "ref.tsv").write_bytes(good + b"x\tok2\t22\n")
    r = run_cli(base + ["-r", tmp_path / "ref.tsv", "--test-files", tmp_path / "t.txt"])
    assert r.returncode != 0 and "ref.tsv line 3: " in r.stderr and "twice" in r.stderr and "(ok2)" in r.stderr
    (tmp_path / "ref.tsv").write_bytes(good)
    os.makedirs(tmp_path / "loc")
    (tmp_path / "loc" / "a.txt").write_bytes(b"C\tok\t20\n\nC\tq\t20\n")
    (tmp_path / "loc" / "b.txt").write_bytes(b"C\tq\t20\r\nC\tok\t21\r\n")
    r = run_cli(base + ["-r", tmp_path / "ref.tsv", "--test-files", tmp_path / "loc"], SLK_COMPARE_CHUNK="5")
    assert r.returncode != 0 and "b.txt line 2: " in r.stderr and "(ok)" in r.stderr
    (tmp_path / "loc" / "b.txt").write_bytes(b"C\tq\t20\nC\tok2\t43\n")
    r = run_cli(base + ["-r", tmp_path / "ref.tsv", "--test-files", tmp_path / "loc"])
    assert r.returncode != 0 and "43" in r.stderr and "taxonomy" in r.stderr


def test_cli_usage_and_refusals(tmp_path, tax_dir):
    (tmp_path / "ref.tsv").write_bytes(b"x\tok\t20\n")
    (tmp_path / "t.txt").write_bytes(b"C\tok\t20\n")
    base = ["-t", tax_dir, "-r", tmp_path / "ref.tsv", "-o", tmp_path / "o"]
    assert run_cli(base + ["--test-files", tmp_path / "t.txt"]).returncode == 0
    for bad in (base, base + ["--test-files", tmp_path / "t.txt", "--multi-dirs", tmp_path], base + ["--test-files"],
                base[2:] + ["--test-files", tmp_path / "t.txt"], base + ["--test-files", tmp_path / "t.txt", "--shard-table"],
                base + ["--test-files", tmp_path / "t.txt", "--devices", "0,1"], base + ["--test-files", tmp_path / "t.txt", "--devices", "all"],
                base + ["--test-files", tmp_path / "t.txt", "--id-col", "3"], base + ["--test-files", tmp_path / "t.txt", "--id-col", "0"],
                base + ["--test-files", tmp_path / "t.txt", "--nonsense"], base + ["--multi-dirs", tmp_path / "t.txt"],
                base + ["--test-files", tmp_path / "missing.txt"]):
        r = run_cli(bad)
        assert r.returncode != 0 and r.stderr.startswith("slacken-amd: "), bad
    assert "--shard-table is not supported by compare" in run_cli(base + ["--test-files", tmp_path / "t.txt", "--shard-table"]).stderr
    assert "compare takes one device" in run_cli(base + ["--test-files", tmp_path / "t.txt", "--devices", "0,1"]).stderr


def test_compare_and_compare_index_both_resolve():
    a = subprocess.run([CLI, "compare"], capture_output=True, text=True)
    b = subprocess.run([CLI, "compare-index"], capture_output=True, text=True)
    assert a.returncode != 0 and "usage: compare -t TAXONOMY_DIR" in a.stderr
    assert b.returncode != 0 and "usage: compare-index -i SUBJECT" in b.stderr
    c = subprocess.run([CLI, "comparison"], capture_output=True, text=True)
    assert c.returncode != 0 and "unknown command line" in c.stderr and "`compare`" in c.stderr and "`compare-index`" in c.stderr
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
    assert "slacken-amd compare -t TAXONOMY_DIR -r REFERENCE -o OUTPUT" in h and "--multi-dirs fam/grp/std_35_31_s7_c0.15_classified" in h
