"""The host statement of low-complexity masking (slacken_amd/host/mask.hpp: mask_sequence_host, the FASTA walk, the file protocol):
compiled alone into a small program under AddressSanitizer and UBSan and compared letter for letter with the recurrence of
tests/mask_model.py, then through `slacken-amd mask --host` on a temporary library (no GPU is opened)."""
import os
import subprocess

import numpy as np
import pytest

import mask_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slacken_amd", "bin", "slacken-amd")

MAIN = r"""
#include "mask.hpp"
#include <cstdlib>
#include <iostream>
// argv: window threshold replacement threads; stdin: one sequence per line (an empty line: an empty sequence).
// stdout: the masked sequences, a line each, then the letters changed
int main(int argc, char **argv) {
  if (argc != 5) return 2;
  slk_mask_config cfg{(uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), (uint8_t)atoi(argv[3])};
  cfg = slk_host::mask_config_defaults(&cfg);
  if (!slk_host::mask_config_ok(cfg)) return 3;
  std::vector<uint8_t> bases;   // (exactly the letters: a read or write past them is the sanitizer's to report)
  std::vector<uint64_t> offsets(1, 0);
  std::string line;
  while (std::getline(std::cin, line)) { bases.insert(bases.end(), line.begin(), line.end()); offsets.push_back(bases.size()); }
  const uint64_t changed = slk_host::mask_sequences_host(bases.data(), offsets.data(), offsets.size() - 1, cfg, (size_t)atoi(argv[4]));
  for (size_t i = 0; i + 1 < offsets.size(); i++) std::cout << std::string(bases.begin() + offsets[i], bases.begin() + offsets[i + 1]) << "\n";
  std::cout << changed << "\n";
  return 0;
}
"""


@pytest.fixture(scope="module")
def masker(tmp_path_factory):
    d = tmp_path_factory.mktemp("maskhost")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "masker")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-pthread", "-I", os.path.join(ROOT, "slacken_amd", "host"), "-o", exe, str(d / "main.cpp")])
    return exe


def run_masker(exe, seqs, window=64, threshold=20, replacement=ord("x"), threads=1):
    out = subprocess.run([exe, str(window), str(threshold), str(replacement), str(threads)], input="".join(s + "\n" for s in seqs),
                         check=True, capture_output=True, text=True).stdout.split("\n")
    return out[:len(seqs)], int(out[len(seqs)])


def model(seqs, **kw):
    b = np.frombuffer("".join(seqs).encode(), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    out, n = mm.mask_dp(b, offsets, **kw)
    text = bytes(out).decode()
    return [text[int(offsets[i]):int(offsets[i + 1])] for i in range(len(seqs))], n


KNOWN = ["A" * 6, "A" * 7, "AC" * 5, "AC" * 6, "A" * 6 + "N" + "A" * 6, "A" * 7 + "N" + "A" * 7, "AAAA", "AAAA", "", "A", "AC", "ACG",
         "u" * 7, "aAaAaAa", "TUtuTUt", "acacacACACAC", "GATTACA" + "A" * 7 + "N"]


@pytest.mark.parametrize("replacement", [ord("x"), ord("N"), 0])
def test_known_answers(masker, replacement):
    got = run_masker(masker, KNOWN, replacement=replacement)
    assert got == model(KNOWN, replacement=replacement)
    r = chr(replacement) if replacement else "a"
    assert got[0][:4] == ["A" * 6, r * 7, "AC" * 5, (r * 12 if replacement else "ac" * 6)]
    assert got[0][6:8] == ["AAAA", "AAAA"]                      # two sequences: the run does not cross the border


@pytest.mark.parametrize("threshold", [10, 20, 40])
@pytest.mark.parametrize("window", [8, 16, 64])
def test_random_families_and_run_lengths(masker, window, threshold):
    rng = np.random.default_rng(7 * window + threshold)
    seqs = []
    for alphabet in ("AC", "AAAC", "ACG", "AACG", "ACGT", "AAAAACGT"):
        seqs += [mm.skewed(rng, int(rng.integers(3, 200)), alphabet) for _ in range(3)]
        seqs.append("".join(c if c in alphabet else alphabet[0] for c in mm.planted(rng, 300, 3, 3, 14, 60)))
    # runs of window - 1, window, window + 1 letters: one letter, a dinucleotide, and skewed text
    for n in (window - 1, window, window + 1):
        seqs += ["A" * n, ("AC" * n)[:n], mm.skewed(rng, n, "AAAC"), "G" + "T" * (n - 1) + "NN" + "T" * n]
    want, n_want = model(seqs, window=window, threshold=threshold)
    got, n_got = run_masker(masker, seqs, window=window, threshold=threshold, threads=3)
    assert got == want and n_got == n_want
    total = sum(len(s) for s in seqs)
    if (window, threshold) != (8, 40):                            # (8, 40) masks nothing by arithmetic: see test_mask_model.py
        assert 0 < n_got < total


def test_a_run_of_5000_letters(masker):
    rng = np.random.default_rng(11)
    text = list(mm.planted(rng, 5000, 25, 4, 20, 300))
    seq = "".join(text)
    want, n_want = model([seq])
    got, n_got = run_masker(masker, [seq])
    assert got == want and n_got == n_want and 0 < n_got < 5000


def test_invalid_parameters_are_refused(masker):
    for w, t in ((7, 20), (65, 20), (64, 256)):
        assert subprocess.run([masker, str(w), str(t), "120", "1"], input="AAAAAAAA\n", capture_output=True, text=True).returncode == 3


# ---- the command on a temporary library, --host ----
def wrap(seq, width, eol="\n"):
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def make_library(d, rng):
    """three files: plain, CRLF line ends with lower-case stretches, and one with an empty record and a record without line end"""
    g = [mm.planted(rng, n, 8, 4, 20, 120) for n in (3000, 1700, 2500, 900, 64)]
    lib = d / "library" / "bacteria"
    lib.mkdir(parents=True)
    (lib / "a.fna").write_text(">s1 first genome\n" + wrap(g[0], 60) + ">s2\n" + wrap(g[1], 80))
    low = g[2][:500] + g[2][500:1200].lower() + g[2][1200:]
    (lib / "b.fna").write_bytes((">s3 crlf\r\n" + wrap(low, 70, "\r\n")).encode())
    (lib / "c.fna").write_text(">empty\n>s4\n" + wrap(g[3], 61) + ">s5 no line end\n" + g[4][:32] + "NNNN" + "A" * 28)
    return [lib / "a.fna", lib / "b.fna", lib / "c.fna"]


def expected_text(text, **kw):
    """the file's text with the letters of every record masked by the model: headers, line ends and everything else as they are"""
    out, seqs, pos = bytearray(text), [], []
    in_record, i = False, 0
    while i < len(text):
        if text[i:i + 1] == b">" and (i == 0 or text[i - 1:i] == b"\n"):
            in_record = True
            seqs.append([])
            pos.append([])
            j = text.find(b"\n", i)
            i = len(text) if j < 0 else j + 1
            continue
        if in_record and text[i:i + 1] not in (b"\n", b"\r"):
            seqs[-1].append(text[i])
            pos[-1].append(i)
        i += 1
    flat = np.array([c for s in seqs for c in s], np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    masked, n = mm.mask_dp(flat, offsets, **kw)
    for j, p in enumerate(p for ps in pos for p in ps):
        out[p] = masked[j]
    return bytes(out), n, len(flat)


@pytest.mark.parametrize("mode", ["default", "soft", "small-pieces"])
def test_cli_host_masks_a_library(tmp_path, mode):
    rng = np.random.default_rng(3)
    files = make_library(tmp_path, rng)
    before = [f.read_bytes() for f in files]
    marked = tmp_path / "library" / "bacteria" / "done.fna"
    marked.write_text(">done\n" + "A" * 100 + "\n")
    (tmp_path / "library" / "bacteria" / "done.fna.masked").write_text("")
    (tmp_path / "library" / "notes.txt").write_text(">not a genome\nAAAAAAAAAAAAAAAA\n")
    env = dict(os.environ)
    if mode == "small-pieces":
        env["SLK_MASK_BATCH_BASES"] = "1000"                      # every record a piece of its own
    args = [CLI, "mask", "-l", str(tmp_path), "--host"] + (["--soft"] if mode == "soft" else [])
    out = subprocess.run(args, check=True, capture_output=True, text=True, env=env).stdout
    kw = dict(replacement=0) if mode == "soft" else {}
    letters = masked = 0
    for f, text in zip(files, before):
        want, n, nl = expected_text(text, **kw)
        got = f.read_bytes()
        assert got == want, f
        assert n > 0 and got != text
        assert os.path.exists(str(f) + ".masked") and not os.path.exists(str(f) + ".tmp")
        letters += nl
        masked += n
    assert marked.read_text() == ">done\n" + "A" * 100 + "\n"     # the marked file is skipped
    assert (tmp_path / "library" / "notes.txt").read_text().startswith(">not a genome\nAAAA")
    assert f" {letters} letters read, {masked} letters masked" in out and "1 files skipped" in out and "3 files," in out
    # a second run skips all four
    out = subprocess.run(args, check=True, capture_output=True, text=True, env=env).stdout
    assert "4 files skipped" in out and " 0 letters masked" in out


def test_cli_host_takes_files_and_parameters(tmp_path):
    f = tmp_path / "one.fasta"
    text = b">r\nACGTACGTAAAAAAAAAACGATCGATTAGC\nACACACACACACACACGGATC\n"
    f.write_bytes(text)
    subprocess.run([CLI, "mask", str(f), "--host", "--window", "16", "--threshold", "10", "--replace", "N"], check=True, capture_output=True)
    want, n, _ = expected_text(text, window=16, threshold=10, replacement=ord("N"))
    assert f.read_bytes() == want and n > 0 and os.path.exists(str(f) + ".masked")
    for bad in (["--window", "7"], ["--threshold", "0"], ["--replace", "a"], ["--shard-table"], ["--nonsense"]):
        g = tmp_path / "two.fasta"
        g.write_bytes(text)
        r = subprocess.run([CLI, "mask", str(g), "--host"] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and g.read_bytes() == text and not os.path.exists(str(g) + ".masked")
    assert subprocess.run([CLI, "mask", str(tmp_path / "missing.fna"), "--host"], capture_output=True).returncode != 0


def test_cli_a_failed_write_leaves_the_original(tmp_path):
    f = tmp_path / "g.fna"
    text = ">r\n" + "A" * 50 + "\n"
    f.write_text(text)
    (tmp_path / "g.fna.tmp").mkdir()                              # FILE.tmp cannot be written: it is a directory
    r = subprocess.run([CLI, "mask", str(f), "--host"], capture_output=True, text=True)
    assert r.returncode != 0 and "g.fna.tmp" in r.stderr
    assert f.read_text() == text and not os.path.exists(str(f) + ".masked")
