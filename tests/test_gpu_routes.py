"""Every classify implementation as a batch's ONLY route, against the oracle, bit for bit.

The classify path holds three independently written implementations of scan, lookup and resolveTree: the lane-per-fragment kernels
(lane.hip) with what they hand on, the wave-per-fragment kernel (fused.hip), the staged scan / probe / classify (kernels.hip).  One
case -- a library, a batch of about 600 reads, the oracle's answers -- is classified under the default switches, under
SLK_FORCE_WAVE=1 and under SLK_FORCE_V1=1 (both read once per classify call), each leg with and without hit lists, unpaired and
with ragged mates, and slk_stream_last_route must show exactly the kernels the leg is about.  The staged kernels' own range,
windows of more than 32 m-mers, follows at the host entry up to the widest window a workgroup's LDS holds; beyond it the splitter is
refused at slk_index_create.

The conditions that keep a comparison from passing on empty answers are asserted on the oracle's output alone
(test_cases_are_not_vacuous: no GPU), so they hold wherever the cases are built."""
import re

import numpy as np
import pytest

import routecases as rc
from routecases import MIN_HIT_GROUPS, SCALARS, THRESHOLDS

gpu = pytest.mark.gpu

SPLITTERS = {
    "k35m31s7": rc.splitter(35, 31, 7),                                # the defaults
    "k35m31s7-noncanonical": rc.splitter(35, 31, 7, canonical=False),
    "k31m31s0": rc.splitter(31, 31, 0),                                # w = 1
    "k13m13s0": rc.splitter(13, 13, 0),                                # the shape of test_gpu_fuzz.py's seed 295
    "k21m12s5": rc.splitter(21, 12, 5),
    "k45m32s16": rc.splitter(45, 32, 16),                              # full 64-bit key
    "k51m20s2": rc.splitter(51, 20, 2),                                # w = 32
    "k5m2s0-kat": rc.splitter(5, 2, 0, xor_mask=0, canonical=False),   # the reference's KAT configuration
}
ROUTES = {"default": None, "wave": "SLK_FORCE_WAVE", "v1": "SLK_FORCE_V1"}
# the wave kernel's four waves a block, the lane kernel's 64-read tile, the staged kernels' 256-lane block
PREFIXES = (1, 4, 5, 64, 65, 256, 257)
WIDE_WINDOWS = (33, 64, 65, 128, 129, 320, 321, 512)
WIDE_CASES = [(w, False) for w in WIDE_WINDOWS] + [(65, True)]
WIDE_PREFIXES = (64, 65, 128, 129)      # either side of the scan's shrunken blocks (128 lanes from w = 33, 64 from w = 65)

_cases = {}


def case_of(orc, name):
    """the case of a name, built once per session: the oracle's work is shared by every route's leg"""
    if name not in _cases:
        if name == "many-taxa":
            _cases[name] = rc.many_taxa_case(orc)
        elif name.startswith("wide"):
            w, canonical = int(name.split("-")[1]), name.endswith("canonical")
            _cases[name] = rc.wide_case(orc, w, canonical, seed=4000 + w)
        else:
            _cases[name] = rc.splitter_case(orc, SPLITTERS[name], seed=3000 + sorted(SPLITTERS).index(name))
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    """the cases -- the oracle's indexes, the engine's tables -- go when the module is through, not when the interpreter is"""
    yield
    _cases.clear()


def wide_name(w, canonical):
    return f"wide-{w}" + ("-canonical" if canonical else "")


@pytest.mark.parametrize("name", sorted(SPLITTERS))
def test_cases_are_not_vacuous(orc, name):
    """per case, on the oracle's output: at least half of the library-derived reads classify at threshold 0, a read has no hit at all
    (unpaired: a pair always has its mate border's entry), ten reads or more hit two or more distinct taxa, min_hit_groups and every threshold decide something; the lengths are all there"""
    case = case_of(orc, name)
    case.check_not_vacuous()
    k = case.ps["k"]
    assert {0, 1, k - 1, k, k + 1, 150, 1000, 1001, 2500} <= {len(r) for r in case.reads} and 550 <= len(case.reads) <= 650
    text = b"|".join(r.tobytes() for r in case.reads)
    assert b"N" in text and b"N" * 40 in text and b"a" in text and b"U" in text and b"u" in text
    assert len(case.reads) > max(PREFIXES)


def test_many_taxa_case_overflows_both_maps(orc):
    case_of(orc, "many-taxa")     # (asserted where it is built: over 12 taxa in 100 reads or more, over 128 in two to five)


def names(mask):
    from slacken_amd import capi
    return {n for bit, n in capi.ROUTE_NAMES.items() if mask & bit}


def expect_route(st, route, reran=False, first="lane"):
    """slk_stream_last_route of the call that just returned: exactly the kernels of the leg.  first: what opens the default route --
    the lane kernel's first pass, or in a batch whose fragments average over 1000 bases the routing kernel that stands for it"""
    got = names(st.last_route())
    extra = {"rerun"} if reran else set()
    if route == "wave":
        assert got == {"wave"} | extra, got
    elif route == "v1":
        assert got == {"staged"}, got          # (an unbounded map from the start: nothing is run again)
    else:
        assert first in got and not got & ({"staged", "routing", "lane"} - {first}) and ("rerun" in got) == reran, got


def compare(case, st, paired, mhg, with_hits, R=None, merged=False, packed=False):
    """one call of slk_classify_batch[_packed] over the case's batch (or its first R reads alone) against the oracle: every scalar of
    every read, and with hit lists the offsets and every entry of every list"""
    from test_gpu_parity import merged_lists
    b, o, mb, mo = case.packed[paired] if R is None else case.prefix(paired, R)
    n = len(o) - 1
    want = case.want(paired, mhg)
    got = st.classify_batch(b, o, mb, mo, min_hit_groups=mhg, thresholds=THRESHOLDS, with_hits=with_hits, with_num_hits=True, packed=packed)
    ctx = (case.ps, dict(paired=paired, mhg=mhg, with_hits=with_hits, R=R, merged=merged, packed=packed))
    for key in SCALARS:
        if key == "num_hits" and merged:
            continue
        assert got[key].shape == want[key][..., :n].shape and np.array_equal(got[key], want[key][..., :n]), (key, ctx)
    if with_hits:
        off, tx, cn = case.lists(paired)
        off = off[:n + 1]
        tx, cn = tx[:int(off[n])], cn[:int(off[n])]
        if merged:
            hits = np.zeros(len(tx), got["hits"].dtype)
            hits["taxon"], hits["count"] = tx, cn
            off, hits = merged_lists(off, hits)
            tx, cn = hits["taxon"], hits["count"]
        assert np.array_equal(got["hit_offsets"], off), ("hit_offsets", ctx)
        assert np.array_equal(got["hits"]["taxon"], tx) and np.array_equal(got["hits"]["count"], cn), ("hits", ctx)


def run_leg(case, st, route, paired, reran=False, prefixes=PREFIXES):
    for mhg in MIN_HIT_GROUPS:
        for with_hits in (True, False):
            compare(case, st, paired, mhg, with_hits)
            expect_route(st, route, reran)
    st.set_merged_hits(True)       # the lists merged on the device (slk_stream_set_merged_hits) against merged_lists over the oracle's
    try:
        compare(case, st, paired, 1, True, merged=True)
        expect_route(st, route, reran)
    finally:
        st.set_merged_hits(False)
    compare(case, st, paired, 3, True, packed=True)       # the packed entry
    expect_route(st, route, reran)
    compare(case, st, paired, 1, False, packed=True)
    for R in prefixes:
        for with_hits in (True, False):
            compare(case, st, paired, 1, with_hits, R=R)
        b, o, mb, mo = case.prefix(paired, R)
        long_batch = (int(o[-1]) + (int(mo[-1]) if paired else 0)) // 1000 > R       # (a lone read of 2500 bases: laneplan.h, route_first)
        expect_route(st, route, first="routing" if long_batch else "lane")


def set_route(monkeypatch, route):
    for env in ("SLK_FORCE_WAVE", "SLK_FORCE_V1"):
        monkeypatch.delenv(env, raising=False)
    if ROUTES[route]:
        monkeypatch.setenv(ROUTES[route], "1")


@gpu
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", sorted(SPLITTERS))
def test_route_matrix(orc, monkeypatch, name, route, paired):
    case = case_of(orc, name)
    case.check_not_vacuous()
    _, st = case.engine()
    set_route(monkeypatch, route)
    run_leg(case, st, route, paired)


@gpu
@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_many_taxa_by_every_route(orc, monkeypatch, route, paired):
    """Reads that name more than 12 taxa leave the lane kernel's map, a few that name more than 128 the wave kernel's: under
    SLK_FORCE_WAVE (and by default) the batch is then classified again by the unbounded re-run, under SLK_FORCE_V1 nothing is."""
    case = case_of(orc, "many-taxa")
    _, st = case.engine()
    set_route(monkeypatch, route)
    run_leg(case, st, route, paired, reran=route != "v1", prefixes=())
    # without the fragments of more than 128 taxa the same stream runs nothing again
    few = [i for i, nd in enumerate(case.want(paired, 1)["num_distinct"]) if nd <= 128][:64]
    import synth
    b, o = synth.pack([case.reads[i] for i in few])
    mb, mo = synth.pack([case.mates[i] for i in few]) if paired else (None, None)
    got = st.classify_batch(b, o, mb, mo, min_hit_groups=1, thresholds=THRESHOLDS, with_hits=False, with_num_hits=True)
    for key in SCALARS:
        assert np.array_equal(got[key], case.want(paired, 1)[key][..., few]), key
    expect_route(st, route, reran=False)


@gpu
def test_switches_move_between_calls_of_one_process(orc, monkeypatch):
    """(what the matrix relies on, stated once: one stream, one process, three routes in a row and back)"""
    case = case_of(orc, "k35m31s7")
    _, st = case.engine()
    for route in ("v1", "default", "wave", "v1", "wave", "default"):
        set_route(monkeypatch, route)
        compare(case, st, False, 1, False, R=65)
        expect_route(st, route)


# ---- windows of more than 32 m-mers at the host entry: the staged kernels' own range, and where it ends ----

LDS_PER_WORKGROUP = 160 * 1024      # MI355X: what one workgroup may declare (the part's LDS per CU), the only part the library loads on
WIDEST = LDS_PER_WORKGROUP // 512   # 320: the scan's ring is 8 bytes per lane and m-mer of the window, a wave of 64 lanes at least
ACCEPTED_WIDE = [(w, c) for w, c in WIDE_CASES if w <= WIDEST]


def lds_limit():
    """what slk_index_create says a workgroup of this device has, in its refusal of the widest window (512 m-mers: a ring of 256 KiB)"""
    import slacken_amd
    with pytest.raises(slacken_amd.SlackenError) as e:
        slacken_amd.Index(k=9 + 511, m=9, spaces=0, canonical=False, expected_records=16, max_taxon=7)
    assert e.value.code == slacken_amd.capi.E_UNSUPPORTED
    return int(re.search(r"workgroup of this device has (\d+)", str(e.value)).group(1))


@pytest.mark.parametrize("w,canonical", ACCEPTED_WIDE, ids=[wide_name(w, c) for w, c in ACCEPTED_WIDE])
def test_wide_cases_are_not_vacuous(orc, w, canonical):
    """the same conditions on the oracle's output for the windows of 33 .. 320 m-mers (no GPU), and the reads' lengths: k-1 .. 3k"""
    case = case_of(orc, wide_name(w, canonical))
    case.check_not_vacuous()
    k = case.ps["k"]
    lens = {len(r) for r in case.reads}
    assert {0, k - 1, k, k + 1, 3 * k} <= lens and max(lens) == 3 * k and len(case.reads) == 301 and len(case.reads) > max(WIDE_PREFIXES)


@gpu
@pytest.mark.parametrize("w,canonical", WIDE_CASES, ids=[wide_name(w, c) for w, c in WIDE_CASES])
def test_wide_windows_at_the_host_entry(orc, monkeypatch, w, canonical):
    """w in 33 .. 512 with m = 9, k = m + w - 1.  Up to 320 m-mers -- 512 w bytes of ring within the 160 KiB a workgroup of an MI355X
    may have -- the batch MUST classify: by the staged kernels alone, with and without hit lists, unpaired and paired, and scanned
    through spans_batch.  321 and 512 MUST be refused at create, with the numbers in the message.  Which side a window is on is this
    file's arithmetic, not the library's answer; nothing is launched whose LDS request the part cannot hold."""
    import slacken_amd
    from test_gpu_parity import oracle_spans
    set_route(monkeypatch, "default")
    ps = rc.splitter(9 + w - 1, 9, 0, canonical=canonical)
    if w > WIDEST:
        with pytest.raises(slacken_amd.SlackenError) as e:
            slacken_amd.Index(**ps, expected_records=16, max_taxon=7)
        assert e.value.code == slacken_amd.capi.E_UNSUPPORTED
        msg = str(e.value)
        assert f"k - m + 1 = {w} " in msg and f"{512 * w} bytes of LDS" in msg and f"has {LDS_PER_WORKGROUP} " in msg and f"at most {WIDEST} m-mers" in msg
        return
    case = case_of(orc, wide_name(w, canonical))
    case.check_not_vacuous()
    _, st = case.engine()
    for paired in (False, True):
        for mhg in MIN_HIT_GROUPS:
            for with_hits in (True, False):
                compare(case, st, paired, mhg, with_hits)
                expect_route(st, "v1")
        for R in WIDE_PREFIXES:
            compare(case, st, paired, 1, True, R=R)
            compare(case, st, paired, 3, False, R=R)
        # the scan alone, through spans_batch: every span of the first 129 reads
        b, o, mb, mo = case.prefix(paired, 129)
        got_off, got = st.spans_batch(b, o, mb, mo)
        want_off, want = oracle_spans(orc, case.p, case.reads[:129], case.mates[:129] if paired else None)
        assert got_off.tolist() == want_off
        assert [(int(s["key"]), int(s["kmers"]), int(s["flag"]), int(s["distinct"])) for s in got] == [(int(a), b_, c, d) for a, b_, c, d in want]


@gpu
def test_the_lds_bound_is_where_the_arithmetic_puts_it():
    """the device says 160 KiB a workgroup, and the last window accepted is 320 m-mers, the first refused 321"""
    import slacken_amd
    assert lds_limit() == LDS_PER_WORKGROUP
    slacken_amd.Index(k=9 + WIDEST - 1, m=9, spaces=0, expected_records=16, max_taxon=7)
    with pytest.raises(slacken_amd.SlackenError) as e:
        slacken_amd.Index(k=9 + WIDEST, m=9, spaces=0, expected_records=16, max_taxon=7)
    assert e.value.code == slacken_amd.capi.E_UNSUPPORTED and f"{512 * (WIDEST + 1)} bytes" in str(e.value)
    # two id columns keep their own bound (w x columns <= 128: 64 KiB)
    with pytest.raises(slacken_amd.SlackenError) as e:
        slacken_amd.Index(k=40 + 64, m=40, spaces=0, expected_records=16, max_taxon=7)
    assert e.value.code == slacken_amd.capi.E_UNSUPPORTED
