"""The paired device route's boundary without a GPU: the entry points are declared, exported and bound, the command line refuses what
--device-pairs does not serve before it opens a device, and the lockstep model agrees with the reference's join where it should."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostmodel
import slacken_amd
from pairparse_model import lockstep, strip
from slacken_amd import capi
from test_host_cli import CLI, ROOT
from test_textparse_cpu import _library_stub, _refused

NEW = ["slk_pair_device", "slk_parse_text_paired", "slk_classify_text_paired"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", ROOT, "slacken_amd/bin/slacken-amd"])


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "slacken_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = slacken_amd.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/slacken_amd.h"
        assert name in capi.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert re.search(r"\bslk_pair_record\b", code)
    for name in ("parse_text_paired", "parse_text_paired_raw", "classify_text_paired"):
        assert hasattr(capi.Stream, name)
    # every entry cites the reference's join, and the parse section no longer calls itself single-end
    assert header.count("InputReader.scala:105-131") >= 3
    limits = re.search(r"Limits:[^\n]*", header).group(0)
    assert "single-end" not in limits and "paired" in limits


def test_every_refusal_happens_before_any_device(tmp_path):
    loc, fa = _library_stub(tmp_path)
    o = str(tmp_path / "o")
    err = _refused("classify", "-i", loc, "-o", o, "--device-pairs", fa, fa)
    assert "--device-pairs" in err and "-p" in err and err.count("\n") == 1
    err = _refused("classify", "-i", loc, "-o", o, "-p", "--device-pairs", "--device-parse", fa, fa)
    assert "--device-pairs" in err and "--device-parse" in err and err.count("\n") == 1
    err = _refused("classify", "-i", loc, "-o", o, "-p", "--shard-table", "--device-pairs", fa, fa)
    assert "--device-pairs" in err and "--shard-table" in err and err.count("\n") == 1
    err = _refused("classify2", "-i", loc, "-o", o, "--library", str(tmp_path), "-p", "--device-pairs", fa, fa)
    assert "--device-pairs" in err and "classify2" in err and err.count("\n") == 1
    err = _refused("classify", "-i", loc, "-o", o, "-p", "--device-pairs", fa, fa, fa)
    assert "pairs of files" in err and "3 files" in err and err.count("\n") == 1
    wide, fa = _library_stub(tmp_path, m=45, k=63)
    err = _refused("classify", "-i", wide, "-o", o, "-p", "--device-pairs", fa, fa)
    assert "--device-pairs" in err and "m=45" in err and err.count("\n") == 1


def test_device_parse_with_paired_input_keeps_its_message(tmp_path):
    loc, fa = _library_stub(tmp_path)
    err = _refused("classify", "-i", loc, "-o", str(tmp_path / "o"), "-p", "--device-parse", fa, fa)
    assert "--device-parse" in err and "unpaired" in err and "--device-pairs" not in err


def test_help_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--device-pairs" in r.stdout + r.stderr


def test_strip_removes_one_suffix():
    assert strip("a/1", "/1") == "a" and strip("a/1/1", "/1") == "a/1" and strip("/1", "/1") == "" and strip("a/2", "/1") == "a/2"
    assert strip("a", "/1") == "a" and strip("", "/1") == "" and strip("1", "/1") == "1"


def _records(rng, n, suffixes):
    titles = [f"read{i}.{int(rng.integers(0, 1 << 30))}" for i in range(n)]
    seq = lambda: "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 30))))
    return ([(t + suffixes[0], seq()) for t in titles], [(t + suffixes[1], seq()) for t in titles])


@pytest.mark.parametrize("suffixes", [("/1", "/2"), ("", ""), ("/1", ""), ("", "/2")])
def test_lockstep_equals_the_join_on_unique_titles_in_the_same_order(suffixes):
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 65, 300):
        r1, r2 = _records(rng, n, suffixes)
        for extra1, extra2 in ((0, 0), (3, 0), (0, 3)):   # (a surplus at the end of either file: the inner join drops it)
            a = r1 + [(f"only1.{i}/1", "AC") for i in range(extra1)]
            b = r2 + [(f"only2.{i}/2", "GT") for i in range(extra2)]
            pairs, P, mismatch = lockstep(a, b)
            assert pairs == hostmodel.paired_join(a, b) and P == n
            assert not mismatch   # (the shorter file ended: its partner's surplus is no disagreement)


def test_lockstep_stops_where_the_join_would_reorder():
    rng = np.random.default_rng(4)
    r1, r2 = _records(rng, 10, ("/1", "/2"))
    r2[4], r2[7] = r2[7], r2[4]
    pairs, P, mismatch = lockstep(r1, r2)
    join = hostmodel.paired_join(r1, r2)
    assert (P, mismatch) == (4, True) and pairs == join[:4] and len(join) == 10
    # a record missing in the middle of file 2 shifts every later mate: the join still finds them, the walk stops
    pairs, P, mismatch = lockstep(r1, r2[:2] + r2[3:])
    assert (P, mismatch) == (2, True) and len(hostmodel.paired_join(r1, r2[:2] + r2[3:])) == 9
    # "/2" in file 1 and "/1" in file 2 are not stripped
    assert lockstep([("a/2", "A")], [("a/2", "C")]) == ([], 0, True)
    assert lockstep([("a/1", "A")], [("a/1", "C")]) == ([], 0, True)
    assert lockstep([("a/1/1", "A")], [("a/1/2", "C")]) == ([("a/1", "A", "C")], 1, False)
