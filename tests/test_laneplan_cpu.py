"""The host's plan of a classify batch (slacken_amd/csrc/laneplan.h: plan_lane, piece_layout, shard_side_per_tile; layouts.h: HandOn,
piece_map_cap): compiled alone, without HIP, into a small program under AddressSanitizer and UBSan and compared with a few lines of
Python that restate the rules -- the routing, the piece route's switch, that the bounds planned from a batch's totals cover what
its fragments need (a bound too small is a device buffer too small), the carving of the scratch, the sharded step's rule."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "laneplan.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace slk;
// stdin, a case a line, `name=value` separated by blanks; one line out per case.
//   plan:  R bases paired hits w k split_long split_hits taxa | lens=a,b,.. (sets R and bases) host=1 (plan from the offsets)
//          switches: force_wave long_max route_first seg_min_len seg_hits piece_min_len piece_hits piece_windows | env=1 (read them)
//   lists: R long_cap route_first          shard: scans R bases w lookups          consts          scan: w lds (the device's bytes per workgroup)
//   setenv SLK_NAME=value ...: moves the process's environment for the lines that follow (an empty value unsets); prints "ok"
int main() {
  char line[1 << 16];
  while (fgets(line, sizeof(line), stdin)) {
    PlanInput in;
    PlanSwitches sw;
    std::vector<uint64_t> offsets(1, 0);   // (exactly R + 1 entries: a read past them is the sanitizer's to report)
    bool host = false, env = false;
    unsigned long long scans = 0, long_cap = 0, lookups = 0, route = 0, lds = 0;
    std::string what;
    for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
      char *eq = strchr(tok, '=');
      if (!eq) { what = tok; continue; }
      const std::string name(tok, eq - tok);
      const long long v = atoll(eq + 1);
      if (what == "setenv") {
        if (name.compare(0, 4, "SLK_") != 0) { fprintf(stderr, "setenv takes SLK_ names, not %s\n", name.c_str()); return 2; }
        if (eq[1]) setenv(name.c_str(), eq + 1, 1); else unsetenv(name.c_str());
        continue;
      }
      if (name == "R") in.R = (uint64_t)strtoull(eq + 1, nullptr, 10);
      else if (name == "bases") in.all_bases = (uint64_t)strtoull(eq + 1, nullptr, 10);
      else if (name == "paired") in.paired = v != 0;
      else if (name == "hits") in.want_hits = v != 0;
      else if (name == "w") in.w = (int)v;
      else if (name == "k") in.k = (int)v;
      else if (name == "split_long") in.split_long = v;
      else if (name == "split_hits") in.split_hits = v != 0;
      else if (name == "taxa") in.taxa_bound = (uint32_t)v;
      else if (name == "host") host = v != 0;
      else if (name == "env") env = v != 0;
      else if (name == "lens") {
        for (const char *p = eq + 1; *p;) {
          char *end;
          offsets.push_back(offsets.back() + strtoull(p, &end, 10));
          p = *end == ',' ? end + 1 : end;
        }
        in.R = offsets.size() - 1; in.all_bases = offsets.back();
      }
      else if (name == "force_wave") sw.force_wave = v != 0;
      else if (name == "long_max") sw.long_max = (long)v;
      else if (name == "route_first") { sw.route_first = (int)v; route = (unsigned long long)v; }
      else if (name == "seg_min_len") sw.seg_min_len = {true, v};
      else if (name == "seg_hits") sw.seg_hits = v != 0;
      else if (name == "piece_min_len") sw.piece_min_len = {true, v};
      else if (name == "piece_hits") sw.piece_hits = (int)v;
      else if (name == "piece_windows") sw.piece_windows = (long)v;
      else if (name == "scans") scans = (unsigned long long)v;
      else if (name == "long_cap") long_cap = (unsigned long long)v;
      else if (name == "lookups") lookups = strtoull(eq + 1, nullptr, 10);
      else if (name == "lds") lds = strtoull(eq + 1, nullptr, 10);
      else { fprintf(stderr, "unknown name %s\n", name.c_str()); return 2; }
    }
    if (what == "consts") {
      printf("frag=%zu record=%zu hit=%zu hdr_words=%d hand_words=%d min_windows=%u default_windows=%u default_min_len=%lld map_bytes=%llu per_base=%llu\n",
             sizeof(PieceFrag), sizeof(PieceRecord), sizeof(PieceHitRecord), (int)PieceHdr::WORDS, (int)HandOn::WORDS, PIECE_MIN_WINDOWS,
             PIECE_DEFAULT_WINDOWS, (long long)PIECE_DEFAULT_MIN_LEN, (unsigned long long)PIECE_DEFAULT_MAP_BYTES, (unsigned long long)PIECE_DEFAULT_MAP_PER_BASE);
    } else if (what == "setenv") {
      printf("ok\n");
    } else if (what == "scan") {
      const ScanLaunch L = plan_scan(in.w);
      printf("block=%d lds=%zu max_window=%d\n", L.block, L.lds, scan_max_window((size_t)lds));
    } else if (what == "lists") {
      for (int l = 0; l < HandOn::LISTS; l++) printf("%llu ", (unsigned long long)HandOn::list_at(l, in.R, long_cap));
      printf("%llu %llu\n", (unsigned long long)HandOn::ordered_at(in.R, long_cap), (unsigned long long)HandOn::entries(in.R, long_cap, route != 0));
    } else if (what == "shard") {
      printf("%u\n", shard_side_per_tile(scans != 0, in.R, in.all_bases, in.w, lookups));
    } else {
      if (host) in.h_offsets = offsets.data();
      const LanePlan p = plan_lane(in, env ? read_plan_switches() : sw);
      const PieceLayout l = piece_layout(p);
      printf("lane=%d route_first=%d seg_on=%d long_max=%u b0=%u b1=%u b2=%u seg_min_len=%u wave_min=%u wave_ratio_q10=%u long_cap=%llu hand_bytes=%zu "
             "piece_min_len=%u piece_windows=%u piece_frags=%llu piece_units=%llu piece_map=%llu piece_hits=%d "
             "frags_at=%zu units_at=%zu records_at=%zu scratch_bytes=%zu maps_bytes=%zu hits_bytes=%zu\n",
             p.lane, p.route_first, p.seg_on, p.long_max, p.long_bound[0], p.long_bound[1], p.long_bound[2], p.seg_min_len, p.wave_min, p.wave_ratio_q10,
             (unsigned long long)p.long_cap, p.hand_bytes, p.piece_min_len, p.piece_windows, (unsigned long long)p.piece_frags,
             (unsigned long long)p.piece_units, (unsigned long long)p.piece_map, p.piece_hits, l.frags_at, l.units_at, l.records_at, l.scratch_bytes,
             l.maps_bytes, l.hits_bytes);
    }
  }
  return 0;
}
"""

ENV_NAMES = {"force_wave": "SLK_FORCE_WAVE", "long_max": "SLK_LANE_LONG_MAX", "route_first": "SLK_ROUTE_FIRST", "seg_min_len": "SLK_SEG_MIN_LEN",
             "seg_hits": "SLK_SEG_HITS", "piece_min_len": "SLK_PIECE_MIN_LEN", "piece_hits": "SLK_PIECE_HITS", "piece_windows": "SLK_PIECE_WINDOWS"}
K = 35


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("laneplan")
    (d / "main.cpp").write_text(MAIN)
    path = str(d / "planner")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "slacken_amd", "csrc"), "-o", path, str(d / "main.cpp")])
    return path


def run_lines(exe, lines, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SLK_")}
    e.update(env or {})
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, env=e)
    return out.stdout.splitlines()


def case_line(c):
    parts = []
    for name, v in c.items():
        parts.append(f"{name}=" + (",".join(map(str, v)) if name == "lens" else str(int(v))))
    return " ".join(parts)


def plans(exe, cases, env=None):
    """the program's plan and layout of every case (a dict of names to values)"""
    return [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in run_lines(exe, [case_line(c) for c in cases], env)]


@pytest.fixture(scope="module")
def consts(exe):
    c = {k: int(v) for k, v in (t.split("=") for t in run_lines(exe, ["consts"])[0].split())}
    # what the model below takes from the documents (include/slacken_amd.h on slk_stream_set_split_long), not from the code
    assert (c["min_windows"], c["default_windows"], c["default_min_len"], c["map_bytes"], c["per_base"]) == (64 * 64, 64 * 1024, 300000, 2 << 30, 8)
    assert c["hdr_words"] == 8 and c["hand_words"] == 32
    return c


def map_cap(nwin, taxa):
    """entries of a fragment's map: a power of two, at least 64, that holds min(windows, taxa) + 1 taxa at a load of a half"""
    cap = 64
    while cap < 2 * (min(nwin, taxa) + 1):
        cap *= 2
    return cap


def need(lens, min_len, windows, taxa, k=K):
    """(fragments, pieces, map entries) the cut makes of a batch, fragment by fragment"""
    cut = [n - k + 1 for n in lens if n >= min_len]
    return len(cut), sum(-(-nw // windows) for nw in cut), sum(map_cap(nw, taxa) for nw in cut)


def model(c):
    """the plan, restated; c as the program takes it, switches absent when unset.  The class borders are not modelled (a test of their own)."""
    lens = c.get("lens")
    R, bases = (len(lens), sum(lens)) if lens is not None else (c["R"], c["bases"])
    paired, hits, w, k, taxa = c.get("paired", 0), c.get("hits", 0), c.get("w", 0), c.get("k", 0), c.get("taxa", 0)
    p = dict.fromkeys(("lane", "route_first", "seg_on", "long_max", "seg_min_len", "wave_min", "wave_ratio_q10", "long_cap", "hand_bytes", "piece_min_len",
                       "piece_windows", "piece_frags", "piece_units", "piece_map", "piece_hits"), 0)
    if c.get("force_wave", 0) or R >= 2 ** 32 - 1:
        return p
    p["lane"] = 1
    p["long_cap"] = min(R, bases // 1001 + 1)
    raw = min(c.get("long_max", 4999), 8191)
    p["long_max"] = raw if raw > 1000 else 0
    p["route_first"] = int(raw > 1000 and (c["route_first"] == 1 if "route_first" in c else bases // 1000 > R))
    p["hand_bytes"] = 32 * 8 + 4 * ((7 + p["route_first"]) * R + 9 * p["long_cap"])
    over = max(p["long_max"], 1000) + 1     # the shortest fragment the passes behind the lane kernel's two share among them
    seg_min = c["seg_min_len"] if "seg_min_len" in c else min(250000, max(16000, bases >> 14))
    seg_ok = not paired and w == 5 and seg_min > 0
    p["seg_on"] = int(seg_ok and (not hits or c.get("seg_hits", 0)))
    p["seg_min_len"] = max(seg_min, over) if p["seg_on"] else 0
    p["wave_min"], p["wave_ratio_q10"] = over, 1792
    piece_min = c["piece_min_len"] if "piece_min_len" in c else c.get("split_long", -1)
    unasked = piece_min < 0
    hits_on = c["piece_hits"] == 1 if "piece_hits" in c else c.get("split_hits", 0)
    if (seg_ok and hits_on and piece_min > 0) if hits else (p["seg_on"] and (p["route_first"] if unasked else piece_min > 0)):
        windows = min(max(-(-max(1, c.get("piece_windows", 64 * 1024)) // 64) * 64, 64 * 64), 1 << 30)
        if unasked:
            piece_min = max(300000, 2 * windows)
        min_len = min(max(piece_min, over), 2 ** 31 - 1)
        if c.get("host", 0):
            frags, units, entries = need(lens, min_len, windows, taxa, k)
        else:
            frags = min(R, bases // min_len)
            units = bases // windows + frags
            entries = 4 * min(bases, frags * taxa) + 64 * frags
        if frags and not (unasked and (8 * entries > 2 << 30 or 8 * entries > 8 * bases)):
            p.update(piece_windows=windows, piece_min_len=min_len, piece_frags=frags, piece_units=units, piece_map=entries, piece_hits=int(hits))
            p["seg_min_len"] = min(p["seg_min_len"], min_len) if p["seg_on"] else min_len
            p["seg_on"] = 1
        else:
            p.update(piece_windows=windows, piece_frags=frags, piece_map=entries)   # (considered and dropped: the sums stay, nothing is sized from them)
    return p


def check(exe, cases, env=None):
    got = plans(exe, cases, env)
    for c, g in zip(cases, got):
        want = model(c)
        assert {k: g[k] for k in want} == want, c
    return got


READS = dict(R=1000, bases=150000, w=5, k=K, taxa=1 << 18)       # a batch of short reads
LONG = dict(R=1000, bases=20_000_000, w=5, k=K, taxa=1 << 18)    # fragments of 20 000 bases on average


def test_routing(exe, consts):
    cases = [dict(READS, R=2 ** 32 - 1, bases=2 ** 33), dict(READS, R=2 ** 32 - 2, bases=2 ** 33), dict(READS, force_wave=1)]
    # route_first on either side of bases / 1000 = R, and forced both ways
    cases += [dict(READS, bases=1_000_999), dict(READS, bases=1_001_000), dict(READS, route_first=1), dict(LONG, route_first=0)]
    cases += [dict(LONG, long_max=v) for v in (0, 1000, 1001, 4999, 8191, 8192, 100000)] + [dict(READS, long_max=1001, route_first=1), dict(READS, long_max=1000, route_first=1)]
    # seg_min_len: floor, in between, ceiling; under the long variant's limit; off for pairs, other windows, hit lists
    cases += [dict(LONG, bases=16000 << 14), dict(LONG, bases=(16000 << 14) - 1), dict(LONG, bases=100_000 << 14), dict(LONG, bases=(250_000 << 14) + 5),
              dict(LONG, bases=1 << 40), dict(LONG, seg_min_len=1), dict(LONG, seg_min_len=4999), dict(LONG, seg_min_len=5000), dict(LONG, seg_min_len=900, long_max=0),
              dict(LONG, seg_min_len=0), dict(LONG, paired=1), dict(LONG, w=4), dict(LONG, w=6), dict(LONG, hits=1), dict(LONG, hits=1, seg_hits=1)]
    got = check(exe, cases)
    assert [g["lane"] for g in got[:3]] == [0, 1, 0]
    assert [g["route_first"] for g in got[3:7]] == [0, 1, 1, 0]
    assert [g["long_max"] for g in got[7:14]] == [0, 0, 1001, 4999, 8191, 8191, 8191]
    assert [g["route_first"] for g in got[14:16]] == [1, 0]
    assert [g["seg_min_len"] for g in got[16:21]] == [16000, 16000, 100_000, 250_000, 250_000]
    for c, g in zip(cases, got):
        if g["lane"]:
            assert g["seg_min_len"] == 0 or g["seg_min_len"] > max(g["long_max"], 1000), c
            assert g["wave_min"] == max(g["long_max"], 1000) + 1
    assert [g["seg_on"] for g in got[25:]] == [0, 0, 0, 0, 0, 1]


def test_class_borders_form_a_geometric_ladder(exe):
    limits = (1001, 1500, 4999, 8191)
    for v, g in zip(limits, plans(exe, [dict(LONG, long_max=v) for v in limits])):
        ratio = (v / 1000) ** 0.25
        ladder = [1000] + [g[f"b{i}"] for i in range(3)] + [v]
        assert ladder == sorted(ladder)
        for i in range(3):   # (truncated to whole bases: within one of the exact border)
            assert abs(g[f"b{i}"] - 1000 * ratio ** (i + 1)) <= 1
    g = plans(exe, [dict(LONG, long_max=1000)])[0]
    assert (g["b0"], g["b1"], g["b2"]) == (0, 0, 0)


PROTOTYPE = [100, 400_000, 150, 1_000_000]


def test_piece_route_on_or_off(exe, consts):
    contigs = dict(w=5, k=K, taxa=1 << 10, lens=[400_000, 150, 1_000_000], host=1)
    cases = []
    for split_long in (-1, 0, 350_000):                      # the stream's setting against the switch, set and unset
        cases += [dict(contigs, split_long=split_long)] + [dict(contigs, split_long=split_long, piece_min_len=v) for v in (-1, 0, 500_000)]
    got = check(exe, cases)
    assert [g["piece_min_len"] for g in got] == [300_000, 300_000, 0, 500_000, 0, 300_000, 0, 500_000, 350_000, 300_000, 0, 500_000]
    assert [g["piece_frags"] for g in got if g["piece_min_len"]] == [2, 2, 1, 2, 1, 2, 2, 1]
    # unasked: only with route_first ...
    got = check(exe, [dict(contigs, route_first=0), dict(contigs, route_first=0, split_long=300_000), dict(contigs, lens=[400_000] + [150] * 500)])     # (475 000 bases in 501 fragments: a batch of reads)
    assert [g["piece_min_len"] for g in got] == [0, 300_000, 0] and got[2]["route_first"] == 0
    # ... and under both caps of the map scratch.  Per base: one fragment of 2^18 or more windows and as many taxa has a map of 2^20
    # entries, 8 MiB, which is 8 bytes a base at 2^20 bases.  In all: sixteen fragments of 2^24 bases and 2^22 taxa make 2^28 entries, 2 GiB.
    per_base = [dict(w=5, k=K, taxa=1 << 18, host=1, lens=[n]) for n in (1 << 20, (1 << 20) - 1)]
    in_all = [dict(w=5, k=K, taxa=1 << 22, host=1, lens=[1 << 24] * n) for n in (16, 17)]
    proto = dict(w=5, k=K, taxa=1 << 18, host=1, lens=PROTOTYPE)
    got = check(exe, per_base + in_all + [proto, dict(proto, split_long=300_000), dict(in_all[1], split_long=300_000)])
    assert [g["piece_min_len"] for g in got] == [300_000, 0, 300_000, 0, 0, 300_000, 300_000]
    assert got[0]["maps_bytes"] == 8 << 20 and got[2]["maps_bytes"] == 2 << 30 and got[6]["maps_bytes"] == 17 << 27
    # with hit lists: a threshold, and split_hits or the switch
    hits = dict(contigs, hits=1)
    cases = [dict(hits), dict(hits, split_hits=1), dict(hits, split_long=300_000), dict(hits, split_long=300_000, split_hits=1),
             dict(hits, split_long=300_000, piece_hits=1), dict(hits, split_long=300_000, split_hits=1, piece_hits=0),
             dict(hits, split_long=300_000, split_hits=1, paired=1), dict(hits, split_long=300_000, split_hits=1, seg_hits=1, seg_min_len=500_000)]
    got = check(exe, cases)
    assert [g["piece_min_len"] for g in got] == [0, 0, 0, 300_000, 300_000, 0, 0, 300_000]
    assert [(g["piece_hits"], g["hits_bytes"] != 0, g["seg_on"]) for g in got] == [(0, False, 0)] * 3 + [(1, True, 1)] * 2 + [(0, False, 0)] * 2 + [(1, True, 1)]
    assert got[3]["seg_min_len"] == 300_000 and got[7]["seg_min_len"] == 300_000     # the segment pass is on for the cut's sake, at most at its threshold
    # the segment pass's threshold never lies above the cut's; windows in whole tiles of 64, at least PIECE_MIN_WINDOWS
    windows = {1: 4096, 4096: 4096, 4097: 4160, 65536: 65536, 65537: 65600, 0: 4096, -5: 4096, 1 << 40: 1 << 30}
    got = check(exe, [dict(contigs, split_long=20_000, piece_windows=v) for v in windows] + [dict(contigs, split_long=20_000, seg_min_len=v) for v in (6000, 20_000, 30_000)])
    assert [g["piece_windows"] for g in got[:len(windows)]] == list(windows.values())
    for g in got:
        assert g["piece_min_len"] == 20_000 and g["seg_min_len"] <= g["piece_min_len"] and g["piece_windows"] % 64 == 0 and g["piece_windows"] >= consts["min_windows"]
    assert plans(exe, [dict(contigs, lens=[3_000_000], piece_windows=1 << 20)])[0]["piece_min_len"] == 2 << 20     # unasked: never under two pieces


def test_bounds_cover_what_the_fragments_need(exe):
    rng = random.Random(20)
    cases, needs = [], []
    for i in range(300):
        top = rng.choice((2000, 50_000, 400_000, 3_000_000))
        lens = [rng.choice((K - 1, K, rng.randint(K - 1, top), rng.randint(K - 1, 3000))) for _ in range(rng.randint(1, 40))]
        c = dict(w=5, k=K, taxa=1 << rng.choice((4, 10, 18, 22)), lens=lens, split_long=rng.choice((1200, 5000, 20_000, 300_000, 1_000_000)),
                 piece_windows=rng.choice((4096, 8192, 65536)))
        if i % 3 == 0:
            c.update(hits=1, split_hits=1)
        if i % 5 == 0:
            c.update(long_max=rng.choice((0, 2000, 8191)))
        cases += [dict(c, host=1), c]
        needs.append(need(lens, max(c["split_long"], max(min(c.get("long_max", 4999), 8191), 1000) + 1), c["piece_windows"], c["taxa"]))
    got = check(exe, cases)
    some = 0
    for (frags, units, entries), exact, bound, c in zip(needs, got[0::2], got[1::2], cases[0::2]):
        assert (exact["piece_frags"], exact["piece_units"] if frags else 0, exact["piece_map"]) == (frags, units, entries), c
        if frags == 0:     # no fragment at or above the threshold: nothing of the route is planned
            assert exact["piece_min_len"] == 0 and exact["piece_units"] == 0
            continue
        some += 1
        assert bound["piece_min_len"] == exact["piece_min_len"] != 0, c
        for name in ("piece_frags", "piece_units", "piece_map", "scratch_bytes", "maps_bytes", "hits_bytes"):
            assert bound[name] >= exact[name], (name, c)
    assert 100 < some < 300


def test_layout(exe, consts):
    cases = [dict(w=5, k=K, taxa=1 << 18, lens=PROTOTYPE, split_long=300_000, host=h, hits=hits, split_hits=1) for h in (0, 1) for hits in (0, 1)]
    cases += [dict(w=5, k=K, taxa=1 << 4, lens=[5000] * 7 + [4999, 100], split_long=5000, piece_windows=64, host=1), dict(READS)]
    for c, g in zip(cases, check(exe, cases)):
        regions = [(0, 8 * consts["hdr_words"]), (g["frags_at"], g["piece_frags"] * consts["frag"]), (g["units_at"], g["piece_units"] * 8),
                   (g["records_at"], g["piece_units"] * consts["record"])]
        end = 0
        for at, size in regions:     # disjoint, in order, without gaps, on 8-byte borders
            assert at == end and at % 8 == 0
            end = at + size
        assert g["scratch_bytes"] == end
        assert g["maps_bytes"] == g["piece_map"] * 8
        assert g["hits_bytes"] == (g["piece_units"] * consts["hit"] if c.get("hits") else 0) and g["piece_hits"] == c.get("hits", 0)
    assert consts["frag"] % 8 == 0 and consts["record"] % 8 == 0


@pytest.mark.parametrize("route_first", [0, 1])
def test_hand_on_lists_do_not_overlap(exe, consts, route_first):
    shapes = [(R, cap) for R in (1, 64, 65) for cap in (1, R)]
    lines = run_lines(exe, [f"lists R={R} long_cap={cap} route_first={route_first}" for R, cap in shapes])
    plan = plans(exe, [dict(R=R, bases=1001 * (cap - 1), w=5, k=K, taxa=16, route_first=route_first) for R, cap in shapes])
    for (R, cap), line, p in zip(shapes, lines, plan):
        *at, ordered, entries = map(int, line.split())
        assert len(at) == 16
        # lists 0..5 and the short ones (15, only with a routing kernel) may hold every fragment, the others the long ones; the ordered list all
        held = [(at[l], R if l < 6 or l == 15 else cap) for l in range(16) if l < 15 or route_first] + [(ordered, R)]
        end = 0
        for start, size in sorted(held):
            assert start >= end
            end = start + size
        assert end <= entries
        assert p["long_cap"] == cap and p["hand_bytes"] == consts["hand_words"] * 8 + 4 * entries


def test_shard_step_rule(exe):
    def rule(scans, R, bases, w, lookups):
        if not scans or not lookups:
            return 0
        tiles, batches = -(-R // 64), -(-lookups // 64)
        per_tile = -(-batches // tiles)
        return per_tile if per_tile <= 3 * (2 / (w + 1) * bases / 64 / tiles) + 8 else 0
    cases = [(0, 1000, 150_000, 5, 64 * 100), (1, 1000, 150_000, 5, 0)]
    for R in (1, 64, 65, 64 * 64, 64 * 64 + 1, 64 * 65):
        tiles = -(-R // 64)
        bases = 64 * 64 * tiles      # own = 2 / 6 * 64 = 21.33 batches a tile: the limit lies at 72 a tile
        cases += [(1, R, bases, 5, 64 * n * tiles + d) for n in (1, 71, 72) for d in (-63, 0, 1)]
        cases += [(1, R, 0, 5, 64 * 8 * tiles), (1, R, 0, 5, 64 * 8 * tiles + 1), (1, R, 192 * tiles, 1, 64 * 11 * tiles), (1, R, 192 * tiles, 1, 64 * 11 * tiles + 1)]
    got = [int(x) for x in run_lines(exe, [f"shard scans={s} R={R} bases={b} w={w} lookups={n}" for s, R, b, w, n in cases])]
    assert got == [rule(*c) for c in cases]
    assert got[:2] == [0, 0]
    at, above = cases.index((1, 65, 64 * 64 * 2, 5, 64 * 72 * 2)), cases.index((1, 65, 64 * 64 * 2, 5, 64 * 72 * 2 + 1))
    assert (got[at], got[above]) == (72, 0)
    assert got[cases.index((1, 1, 0, 5, 64 * 8))] == 8 and got[cases.index((1, 1, 0, 5, 64 * 8 + 1))] == 0


def test_switches_are_read_as_the_plan_takes_them(exe):
    """read_plan_switches: the environment's values give the plan the same values give as arguments; unset is unset"""
    base = dict(w=5, k=K, taxa=1 << 10, lens=[400_000, 150, 1_000_000], host=1)
    for sw in ({}, dict(long_max=2000, route_first=0, seg_min_len=30_000, piece_min_len=350_000, piece_windows=5000), dict(route_first=1, seg_hits=1, piece_hits=1, force_wave=1),
               dict(seg_min_len=0), dict(piece_min_len=0), dict(piece_min_len=-1, piece_hits=0, long_max=9000)):
        for c in (dict(base), dict(base, hits=1, split_hits=1, split_long=300_000)):
            env = {ENV_NAMES[name]: str(v) for name, v in sw.items()}
            assert plans(exe, [dict(c, env=1)], env) == plans(exe, [dict(c, **sw)])


def test_the_ab_switches_move_within_one_process(exe):
    """SLK_FORCE_WAVE and SLK_FORCE_V1 are read with the rest, per call: one process of the planner sees them come and go"""
    c = case_line(dict(READS, env=1))
    lines = [c, "setenv SLK_FORCE_WAVE=1", c, "setenv SLK_FORCE_WAVE=0", c, "setenv SLK_FORCE_WAVE=1 SLK_FORCE_V1=1", c, "setenv SLK_FORCE_WAVE=", c,
             "setenv SLK_FORCE_V1=", c]
    out = run_lines(exe, lines)
    assert out[1::2] == ["ok"] * 5
    lane = [int(dict(t.split("=") for t in line.split())["lane"]) for line in out[0::2]]
    assert lane == [1, 0, 1, 0, 1, 1]          # (force_v1 is not the plan's to act on: classify.hip takes the staged kernels before any plan)
    # ... and a process started with the switch set can drop it
    out = run_lines(exe, [c, "setenv SLK_FORCE_WAVE=", c], {"SLK_FORCE_WAVE": "1"})
    assert [int(dict(t.split("=") for t in line.split())["lane"]) for line in (out[0], out[2])] == [0, 1]


def test_scan_ring_fits_what_the_device_gives(exe):
    """plan_scan / scan_max_window: 256 lanes while 2048 w bytes fit 64 KiB, halved down to one wave; a wave's ring is 512 w bytes, and
    the widest window is the device's LDS per workgroup over 512, at most 512 (MI355X_MICROARCH: 160 KiB -- 320 m-mers)"""
    ws = (1, 5, 32, 33, 64, 65, 128, 129, 320, 321, 512)
    got = [{k: int(v) for k, v in (t.split("=") for t in line.split())} for line in run_lines(exe, [f"scan w={w} lds=163840" for w in ws])]
    for w, g in zip(ws, got):
        block = 256 if w <= 32 else 128 if w <= 64 else 64
        assert (g["block"], g["lds"]) == (block, block * w * 8) and g["max_window"] == 320
        assert g["lds"] <= 65536 or (g["block"] == 64 and w > 128)
        assert (g["lds"] <= 163840) == (w <= g["max_window"])          # what is accepted is what fits
    limits = {65536: 128, 65535: 127, 163840: 320, 163839: 319, 262144: 512, 1 << 20: 512, 0: 0}
    got = run_lines(exe, [f"scan w=5 lds={v}" for v in limits])
    assert [int(line.split()[2].split("=")[1]) for line in got] == list(limits.values())
