"""The device parser's boundary without a GPU: the new entry points are declared, exported and bound, and the command line refuses what
--device-parse does not serve before it opens a device."""
import os
import re
import subprocess

import pytest

import slacken_amd
from slacken_amd import capi
from test_host_cli import CLI, ROOT

NEW = ["slk_parse_tile_bytes", "slk_parse_device", "slk_parse_text", "slk_classify_text"]


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
    assert re.search(r"#define\s+SLK_FORMAT_FASTA\s+0\b", code) and re.search(r"#define\s+SLK_FORMAT_FASTQ\s+1\b", code)
    assert (capi.FORMAT_FASTA, capi.FORMAT_FASTQ) == (0, 1)
    assert capi._format("fasta") == 0 and capi._format("FASTQ") == 1
    with pytest.raises(ValueError):
        capi._format("sam")
    t = capi.parse_tile_bytes()   # (host arithmetic: no device is opened)
    assert t > 0 and t % 16 == 0
    assert hasattr(capi.Stream, "parse_text") and hasattr(capi.Stream, "classify_text")


def test_constants_the_scale_tests_are_sized_by():
    """tests/test_gpu_textparse_scale.py places its texts right below, on and above the parser's scan block, grid and line tile and the
    command line's default chunk: whoever retunes one of these moves the ladder of that file along with it."""
    source = open(os.path.join(ROOT, "slacken_amd", "csrc", "textparse.hip")).read()
    revisit = "revisit SB, G, LB and the sizes of tests/test_gpu_textparse_scale.py"
    for name, value in (("TP_SCAN_BLOCK", 1024), ("TP_MAX_GRID", 2048), ("TP_BLOCK", 256), ("TP_LANE_BYTES", 16)):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, source)
        assert m, f"{name} is no longer a plain constant of textparse.hip: {revisit}"
        assert int(m.group(1)) == value, f"{name} is {m.group(1)}, the scale tests assume {value}: {revisit}"
    assert re.search(r"constexpr\s+uint32_t\s+TP_TILE\s*=\s*TP_BLOCK\s*\*\s*TP_LANE_BYTES\s*;", source), f"TP_TILE: {revisit}"
    assert capi.parse_tile_bytes() == 256 * 16, revisit
    seqio = open(os.path.join(ROOT, "slacken_amd", "host", "seqio.hpp")).read()
    body = re.search(r"inline\s+size_t\s+io_chunk_bytes\s*\(\s*\)\s*\{(.*?)\n\}", seqio, re.S)
    assert body, f"io_chunk_bytes() is gone from host/seqio.hpp: {revisit}"
    assert re.search(r":\s*\(size_t\)\s*8\s*<<\s*20\s*;", body.group(1)), f"the default chunk is no longer 8 << 20 bytes: {revisit}"
    assert 2048 * capi.parse_tile_bytes() == 8 << 20   # the default chunk is exactly one grid of tiles: any carry makes the blocks stride


def _library_stub(tmp_path, m=31, k=35):
    loc = str(tmp_path / "lib")
    with open(loc + ".properties", "w") as f:
        f.write(f"k={k}\nm={m}\nversion=1\nsplitter=randomXOR\nminimizerSpaces=7\n")
    (tmp_path / "r.fa").write_text(">a\nACGT\n")
    return loc, str(tmp_path / "r.fa")


def _refused(*args):
    # (no device may be opened: with every GPU hidden, opening one would be the error reported instead)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([CLI, *args], capture_output=True, text=True, env=env)
    assert r.returncode != 0
    assert "slk_" not in r.stderr, r.stderr
    return r.stderr


def test_device_parse_with_paired_input_is_refused_before_any_device(tmp_path):
    loc, fa = _library_stub(tmp_path)
    err = _refused("classify", "-i", loc, "-o", str(tmp_path / "o"), "-p", "--device-parse", fa, fa)
    assert "--device-parse" in err and "unpaired" in err
    assert err.count("\n") == 1   # one sentence


def test_the_other_refusals_need_no_device_either(tmp_path):
    loc, fa = _library_stub(tmp_path)
    err = _refused("classify", "-i", loc, "-o", str(tmp_path / "o"), "--shard-table", "--device-parse", fa)
    assert "--device-parse" in err and "--shard-table" in err and err.count("\n") == 1
    err = _refused("classify2", "-i", loc, "-o", str(tmp_path / "o"), "--library", str(tmp_path), "--device-parse", fa)
    assert "--device-parse" in err and "classify2" in err and err.count("\n") == 1
    wide, fa = _library_stub(tmp_path, m=45, k=63)
    err = _refused("classify", "-i", wide, "-o", str(tmp_path / "o"), "--device-parse", fa)
    assert "--device-parse" in err and "m=45" in err and err.count("\n") == 1


def test_help_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--device-parse" in r.stdout + r.stderr
