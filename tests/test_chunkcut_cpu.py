"""The host's chunk cutter (slacken_amd/csrc/chunkcut.h: group_end, cut_chunks), which library construction, coverage and support
share: compiled alone into a small program under AddressSanitizer and UBSan and compared with a few lines of Python, at the lengths
around one and two chunks, for both kinds of seam, with a skipped sequence in the middle and groups forced small."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "chunkcut.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
// argv: k cw exact_seams group_bytes skipped_sequence len...
int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const uint32_t k = (uint32_t)atoi(argv[1]), cw = (uint32_t)atoi(argv[2]);
  const bool exact = atoi(argv[3]) != 0;
  const uint64_t group = strtoull(argv[4], nullptr, 10), skipped = strtoull(argv[5], nullptr, 10);
  std::vector<uint64_t> offsets(1, 0);   // (exactly R + 1 entries: a read past them is the sanitizer's to report)
  for (int a = 6; a < argc; a++) offsets.push_back(offsets.back() + strtoull(argv[a], nullptr, 10));
  const uint64_t R = offsets.size() - 1;
  for (uint64_t i = 0, j; i < R; i = j) {
    j = slk::group_end(offsets.data(), i, R, group);
    slk::cut_chunks(offsets.data(), i, j, k, cw, exact, [&](uint64_t q) { return q == skipped; },
                    [&](uint64_t q, uint64_t start, uint32_t bases, uint32_t early) {
                      printf("%llu %llu %llu %u %u\n", (unsigned long long)i, (unsigned long long)q, (unsigned long long)start, bases, early);
                    });
  }
  return 0;
}
"""


def model(lens, skipped, k, cw, exact, group):
    """(first sequence of the group, sequence, start in the group, bases, early) of every chunk"""
    offs, out, i = [sum(lens[:q]) for q in range(len(lens) + 1)], [], 0
    while i < len(lens):
        j = i + 1
        while j < len(lens) and offs[j + 1] - offs[i] <= group:
            j += 1
        for q in range(i, j):
            windows = lens[q] - k + 1 if q != skipped else 0
            for w0 in range(0, max(windows, 0), cw):
                early = 1 if exact and w0 else 0
                out.append((i, q, offs[q] - offs[i] + w0 - early, min(cw, windows - w0) + k - 1 + early, early))
        i = j
    return out


@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunkcut")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "cutter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "slacken_amd", "csrc"), "-o", exe, str(d / "main.cpp")])
    return exe


@pytest.mark.parametrize("exact", [0, 1], ids=["overlap-k-1", "exact-seams"])
@pytest.mark.parametrize("k,cw", [(35, 512), (5, 4)])
def test_cuts_match_the_model(cutter, k, cw, exact):
    edge = [k - 1, k, k + cw - 2, k + cw - 1, k + cw, k + 2 * cw - 1]
    lens = edge[:3] + [k + cw] + edge[3:] + [0, 3 * cw + k]       # sequence 3 is skipped; an empty one; one of four chunks
    for group in (1, 2 * (k + cw), 1 << 30):                      # every sequence a group; a few groups; one group
        out = subprocess.run([cutter, str(k), str(cw), str(exact), str(group), "3", *map(str, lens)], check=True, capture_output=True, text=True)
        got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
        assert got == model(lens, 3, k, cw, exact, group)
        # and what the scan relies on, stated apart from the model: every window of every kept sequence belongs to exactly one chunk
        offs = [sum(lens[:q]) for q in range(len(lens) + 1)]
        owned = {}
        for i, q, start, bases, early in got:
            assert start >= 0 and offs[i] + start + bases <= offs[q + 1] and offs[i] + start >= offs[q]
            first = offs[i] + start + early - offs[q]
            for w in range(first, first + bases - early - (k - 1)):
                assert (q, w) not in owned
                owned[(q, w)] = True
            assert 1 <= bases - early - (k - 1) <= cw and early == (1 if exact and first else 0)
        assert len(owned) == sum(max(n - k + 1, 0) for q, n in enumerate(lens) if q != 3)
        if group == 1:
            assert all(i == q for i, q, *_ in got)
        if group == 1 << 30:
            assert all(i == 0 for i, *_ in got)
