"""The shared resolveTree core (slacken_amd/csrc/resolve.h: resolve_best + resolve_lift on Euler-tour intervals, resolve_walk_best +
resolve_walk_lift on parent walks, tax_lca, the tour of build_tour -- the one index.hip uploads -- and the rule for ids outside the
taxonomy): compiled alone, without HIP, into a small program under AddressSanitizer and UBSan, and compared line by line with the
oracle's resolve_tree and lca.  Exact.  The maps come in the two forms the kernels hold them in: one per lane (NONE never enters, at
most 12 entries) and staged (NONE kept among the entries, up to about 200)."""
import os
import subprocess

import numpy as np
import pytest

import taxgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "resolve.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>
using namespace slk;
// stdin, a line each:
//   T n p0 .. p(n-1)                              the taxonomy for the lines that follow; its tour is build_tour's
//   M form nreq req.. n taxon count ..            a map (form 0: one per lane, no NONE; form 1: staged, NONE kept) -> "best iv walk iv walk .."
//   L a b                                         -> tax_lca(a, b)
// Every array is allocated at its exact size: a read past one is the sanitizer's to report.
template <class T> struct Arr {
  std::unique_ptr<T[]> p;
  explicit Arr(size_t n) : p(new T[n]) {}
  T &operator[](size_t i) const { return p[i]; }
};
struct LaneForm {    // intervals stored beside the entries (lane.hip, bracken.hip)
  const Arr<int32_t> &t, &c;
  const Arr<uint32_t> &in, &out;
  int len;
  int n() const { return len; }
  int32_t taxon(int j) const { return t[j]; }
  int32_t count(int j) const { return c[j]; }
  uint32_t tin(int j) const { return in[j]; }
  uint32_t tout(int j) const { return out[j]; }
  bool live(int) const { return true; }
};
struct StagedForm {  // intervals looked up again where they are needed, NONE kept and not live (kernels.hip)
  const Arr<int32_t> &t, &c;
  Tour tour;
  int len;
  int n() const { return len; }
  int32_t taxon(int j) const { return t[j]; }
  int32_t count(int j) const { return c[j]; }
  uint32_t tin(int j) const { return tour.node(t[j]).tin; }
  uint32_t tout(int j) const { return tour.node(t[j]).tout; }
  bool live(int j) const { return t[j] != 0; }
};
int main() {
  std::string line;
  std::unique_ptr<int32_t[]> parents;
  std::unique_ptr<TourNode[]> nodes;
  int32_t T = 0;
  while (std::getline(std::cin, line)) {
    char *p = &line[0];
    const char what = *p++;
    const auto next = [&p]() { return strtol(p, &p, 10); };
    if (what == 'T') {
      T = (int32_t)next();
      parents.reset(new int32_t[T]);
      for (int32_t i = 0; i < T; i++) parents[i] = (int32_t)next();
      const std::vector<TourNode> tour = build_tour(parents.get(), T);
      nodes.reset(new TourNode[T]);
      for (int32_t i = 0; i < T; i++) nodes[i] = tour[i];
      printf("ok\n");
    } else if (what == 'L') {
      const int32_t a = (int32_t)next(), b = (int32_t)next();
      printf("%d\n", tax_lca(parents.get(), T, a, b));
    } else if (what == 'M') {
      const int form = (int)next(), nreq = (int)next();
      Arr<double> req(nreq);
      for (int i = 0; i < nreq; i++) req[i] = (double)next();
      const int n = (int)next();
      Arr<int32_t> t(n), c(n);
      Arr<uint32_t> in(n), out(n);
      const Tour tour{nodes.get(), T};
      const Parents par{parents.get(), T};
      for (int j = 0; j < n; j++) {
        t[j] = (int32_t)next(); c[j] = (int32_t)next();
        const TourNode nd = tour.node(t[j]);
        in[j] = nd.tin; out[j] = nd.tout;
      }
      const LaneForm lane{t, c, in, out, n};
      const StagedForm staged{t, c, tour, n};
      const Best best = form == 0 ? resolve_best(lane, tour) : resolve_best(staged, tour);
      const int32_t wbest = resolve_walk_best(lane, par);
      printf("%d %d", best.taxon, wbest);
      for (int i = 0; i < nreq; i++)
        printf(" %d %d", form == 0 ? resolve_lift(lane, tour, best, req[i]) : resolve_lift(staged, tour, best, req[i]), resolve_walk_lift(lane, par, wbest, req[i]));
      printf("\n");
    } else {
      fprintf(stderr, "unknown line %c\n", what);
      return 2;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("resolve")
    (d / "main.cpp").write_text(MAIN)
    path = str(d / "resolver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "slacken_amd", "csrc"), "-o", path, str(d / "main.cpp")])
    return path


def run_lines(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True)
    return out.stdout.splitlines()


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SEED = 20261021
LANE_MAP = 12          # entries of a lane's map (lane.hip: OMAP)
COUNTS = (1, 1, 1, 2, 3, 7, 8191)


def forest(size, cuts, rng):
    """taxgen's taxonomy with `cuts` of its nodes detached from their parents: each is the top of a tree of its own"""
    parents = taxgen.taxonomy(size, rng)
    defined = [t for t in taxgen.defined_taxa(parents) if t != 1]
    for t in rng.choice(defined, size=min(cuts, len(defined)), replace=False):
        parents[t] = 0
    return parents


def chain(depth, rng):
    """ROOT, a chain of `depth` nodes below it, and a leaf hanging off every fourth of them"""
    parents = [0, 0] + list(range(1, depth + 1))
    for t in range(2, depth + 2, 4):
        parents.append(t)
    return np.array(parents, np.int32)


def make_map(parents, form, n, rng):
    """n distinct taxa with counts: any id that may stand in a map -- defined taxa, unused ids in range, ids outside the taxonomy --
    drawn at random, along one lineage, or with equal counts (ties); staged maps usually keep a NONE entry somewhere among them"""
    T = len(parents)
    pool = list(range(1, T)) + [T, T + 1, T + 7, (1 << 22) + 5]
    style = rng.integers(0, 4)
    taxa = []
    if style == 0 and n >= 2:      # a lineage, bottom up or shuffled, and now and then a taxon off it
        deep = max((int(t) for t in rng.choice(np.arange(1, T), size=min(8, T - 1), replace=False)), key=lambda t: len(taxgen.path_to_root(parents, t)))
        taxa = taxgen.path_to_root(parents, deep)
        rng.shuffle(taxa)
    while len(taxa) < n:
        t = int(pool[rng.integers(0, len(pool))])
        if t not in taxa:
            taxa.append(t)
    taxa = taxa[:n]
    if style in (1, 2):            # ties: equal counts
        counts = [int(COUNTS[rng.integers(0, len(COUNTS))])] * n
    else:
        counts = [int(COUNTS[rng.integers(0, len(COUNTS))]) for _ in range(n)]
    if form == 1 and rng.integers(0, 4) != 0:
        at = int(rng.integers(0, len(taxa) + 1))
        taxa.insert(at, 0)
        counts.insert(at, int(COUNTS[rng.integers(0, len(COUNTS))]))
    total = sum(counts)
    reqs = [0, 1, total, total + 1] + [int(r) for r in rng.integers(0, total + 2, size=3)]
    return dict(form=form, taxa=taxa, counts=counts, reqs=reqs)


def make_cases():
    """[(parents, [map, ..], [(a, b), ..])]: a fixed seed, about 3 500 maps, of which about 700 take the one-per-lane form"""
    rng = np.random.default_rng(SEED)
    taxonomies = [taxgen.taxonomy(8, rng), taxgen.taxonomy(30, rng), taxgen.taxonomy(100, rng), taxgen.taxonomy(300, rng),
                  forest(30, 4, rng), forest(100, 10, rng), forest(300, 25, rng), forest(30, 12, rng), chain(40, rng),
                  taxgen.sparse_relabel(taxgen.taxonomy(100, rng), 2000, rng)[0]]
    out = []
    for parents in taxonomies:
        T = len(parents)
        maps = []
        for n in (0, 1, 2, LANE_MAP):
            maps += [make_map(parents, 0, min(n, T - 1), rng) for _ in range(5)]
        maps += [make_map(parents, 0, int(rng.integers(2, LANE_MAP + 1)), rng) for _ in range(50)]
        for n in (0, 1, 2, LANE_MAP, LANE_MAP + 1):
            maps += [make_map(parents, 1, min(n, T - 1), rng) for _ in range(5)]
        maps += [make_map(parents, 1, int(rng.integers(2, min(40, T))), rng) for _ in range(250)]
        if T > 200:
            maps += [make_map(parents, 1, n, rng) for n in (199, 200, 200, 201)]
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, T + 3, size=(60, 2))] + [(0, 0), (1, 1), (0, T + 5), (T + 5, T + 5), (T + 5, T + 6), (1, T)]
        out.append((parents, maps, pairs))
    return out


# ---- what a case exercises, from the parents and the map alone ----------------------------------------------------------------------
def root_path(parents, t):
    out = []
    while t != 0:
        out.append(t)
        t = int(parents[t]) if 0 <= t < len(parents) else 0
    return out


def traits(parents, m):
    """which of resolve.h's branches this map must take, by the reference's own walk (LowestCommonAncestor.scala:101-146)"""
    entries = [(t, c) for t, c in zip(m["taxa"], m["counts"]) if t != 0]
    count = dict(entries)
    paths = {t: root_path(parents, t) for t, _ in entries}
    score = {t: sum(count.get(x, 0) for x in paths[t]) for t, _ in entries}
    top = max(score.values(), default=0)
    tied = [t for t, _ in entries if score[t] == top]
    tie = any(a not in paths[b] and b not in paths[a] for i, a in enumerate(tied) for b in tied[i + 1:])
    never_meet = False
    lca = 0
    for t in tied:                                 # LowestCommonAncestor.apply :49-78, folded in map order
        if lca == 0:
            lca = t
            continue
        pa = root_path(parents, lca)
        hit = next((x for x in paths[t] if x in pa), None)
        never_meet |= hit is None
        lca = 1 if hit is None else hit
    sum_all = sum(c for _, c in entries)
    side = above = whole = False
    for req in m["reqs"]:
        for cand in root_path(parents, lca):
            clade = sum(c for t, c in entries if cand in paths[t])
            if clade >= req:
                break
            if clade == sum_all:
                whole = True
                break
            outside = [t for t, _ in entries if cand not in paths[t]]
            if any(t not in root_path(parents, cand) for t in outside):
                side = True
            else:
                above = True
    return dict(tie=tie, never_meet=tie and never_meet, side=side, above=above, whole=whole)


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def test_the_cases_reach_every_branch(cases):
    """not vacuous: the counts of maps that must take the tie's climb, the ROOT fallback, the side-branch lift, the jump to the nearest
    map taxon above, and the early end -- with the sizes, counts and ids the kernels meet"""
    seen = dict.fromkeys(("tie", "never_meet", "side", "above", "whole"), 0)
    sizes, lane_sizes, n_maps, n_lane, outside, big = set(), set(), 0, 0, 0, 0
    for parents, maps, _ in cases:
        for m in maps:
            for k, v in traits(parents, m).items():
                seen[k] += bool(v)
            live = sum(t != 0 for t in m["taxa"])
            sizes.add(live)
            n_maps += 1
            if m["form"] == 0:
                assert 0 not in m["taxa"] and live <= LANE_MAP
                lane_sizes.add(live)
                n_lane += 1
            outside += any(t >= len(parents) for t in m["taxa"])
            big += 8191 in m["counts"] and 1 in m["counts"]
    print(seen, n_maps, n_lane)
    assert seen["tie"] >= 100 and seen["never_meet"] >= 20 and seen["side"] >= 100 and seen["above"] >= 100 and seen["whole"] >= 50
    assert n_maps >= 3000 and n_lane >= 300
    assert {0, 1, 2, 12, 13, 199, 200, 201} <= sizes and {0, 1, 2, 12} <= lane_sizes
    assert outside >= 100 and big >= 100
    assert any(max(len(root_path(p, t)) for t in range(1, len(p))) >= 40 for p, _, _ in cases)     # the chain


def test_resolve_matches_the_oracle(exe, orc, cases):
    for parents, maps, _ in cases:
        lines = ["T %d " % len(parents) + " ".join(map(str, parents))]
        for m in maps:
            flat = " ".join(f"{t} {c}" for t, c in zip(m["taxa"], m["counts"]))
            lines.append(f"M {m['form']} {len(m['reqs'])} " + " ".join(map(str, m["reqs"])) + f" {len(m['taxa'])} {flat}")
        got = run_lines(exe, lines)
        assert got[0] == "ok" and len(got) == len(lines)
        for m, line in zip(maps, got[1:]):
            best = orc.resolve_tree(parents, m["taxa"], m["counts"], 0)
            want = [best, best]
            for req in m["reqs"]:
                want += [orc.resolve_tree(parents, m["taxa"], m["counts"], req)] * 2
            assert [int(x) for x in line.split()] == want, (m, list(parents))


def test_lca_matches_the_oracle(exe, orc, cases):
    for parents, _, pairs in cases:
        got = run_lines(exe, ["T %d " % len(parents) + " ".join(map(str, parents))] + [f"L {a} {b}" for a, b in pairs])
        assert [int(x) for x in got[1:]] == [orc.lca(parents, a, b) for a, b in pairs]
