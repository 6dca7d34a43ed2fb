"""tests/compare_model.py against the reference's own test (MappingComparisonTest.scala:27-57) and against hand-worked cases of
every rule the issue of `compare` states: the yardstick is checked before anything is measured with it.  No GPU, no native code."""
import math

import pytest

import compare_model as cm

SPECIES = cm.SPECIES[1]

# the six-node taxonomy of MappingComparisonTest.scala:28-34
SIX = cm.Taxonomy([(1, 1, "root"), (2, 1, "genus"), (3, 2, "species"), (4, 3, "species"), (5, 4, "species"), (6, 2, "species")])

# its eight cases (:41-56) as data: (ref, test, class, index)
EIGHT = [(2, 2, "TruePos", 0), (3, 2, "VaguePos", 1), (4, 2, "VaguePos", 1), (3, 1, "VaguePos", 8), (3, 6, "FalsePos", 9),
         (4, 3, "TruePos", 0), (3, cm.NONE, "FalseNeg", 9), (3, 5, "TruePos", 0)]


@pytest.mark.parametrize("ref,test,cls,index", EIGHT)
def test_hit_categories_of_the_reference_test(ref, test, cls, index):
    assert cm.hit_category(SIX, ref, test, SPECIES) == (cls, index)


def test_vague_pos_minus_one():
    """the reference's ancestor at the level is ROOT (the truth IS the root) and the test taxon is not on its path: the branch of
    :321-324 yields VaguePos(standardStepsToAncestor) = VaguePos(-1)"""
    assert SIX.standard_ancestor_at_level(1, SPECIES) is None
    assert cm.hit_category(SIX, 1, 3, SPECIES) == ("VaguePos", -1)
    assert cm.hit_category(SIX, 1, 1, SPECIES) == ("TruePos", 0)
    # and it enters the read index as -1
    m, _ = cm.per_read(SIX, {(1, 3): 2, (3, 3): 2}, cm.SPECIES)
    assert m == (4, 4, 2, 0, 2, 0, 1.0, 0.5, -0.5)


def test_taxonomy_helpers():
    assert [SIX.depth(t) for t in (0, 1, 2, 3, 4, 5, 6)] == [-1, 0, 7, 8, 8, 8, 8]
    assert SIX.standard_ancestor_at_level(5, 8) == 3 and SIX.standard_ancestor_at_level(5, 7) == 2      # S, not S1 or S2
    assert SIX.standard_ancestor_at_level(2, 8) is None and SIX.standard_ancestor_at_level(0, 7) is None
    assert SIX.has_ancestor(5, 5) and SIX.has_ancestor(5, 1) and not SIX.has_ancestor(3, 6) and not SIX.has_ancestor(0, 1)
    assert SIX.standard_steps_to_ancestor(5, 2) == 1 and SIX.standard_steps_to_ancestor(5, 6) == -1
    assert SIX.taxa_with_ancestors([5, 6]) == {1, 2, 3, 4, 5, 6} and SIX.taxa_with_ancestors([]) == set()
    # an id the taxonomy does not define: a path of just itself, no depth, no ancestor at any level
    t = cm.Taxonomy([(1, 1, "root"), (2, 1, "genus"), (9, 2, "species")])
    assert not t.is_defined(5) and t.path_to_root(5) == [5] and t.depth(5) == -1 and t.standard_ancestor_at_level(5, 7) is None


def test_reference_rows_are_filtered():
    tax = cm.Taxonomy([(1, 1, "root"), (2, 1, "genus"), (3, 2, "species"), (4, 2, "species")], merged=[(7, 4)])
    text = (b"x\tr1/1\t3\n" b"x\tr1/2\t3\n"            # the second mate's row goes, the first loses its /1
            b"x\ta/1b/1\t3\r\n"                        # /1 twice in one id: both go, wherever they are
            b"\n"                                      # an empty line
            b"x\tr5\t5\r"                              # a taxon the taxonomy does not define
            b"x\tr6\t7\n"                              # a merged id: counted under its primary
            b"x\tr7\t+4")                              # Java's parseInt takes the sign; no line end
    rows, (read, dropped) = cm.reference_rows(text)
    assert rows == {b"r1": 3, b"ab": 3, b"r5": 5, b"r6": 7, b"r7": 4} and (read, dropped) == (6, 1)
    _, ref_taxa, _, _ = cm.join(rows, [])
    by_taxon, unknown = cm.filtered_reference(tax, ref_taxa)
    assert by_taxon == {3: 2, 4: 2} and unknown == [5]
    out, _ = cm.location_metrics(tax, ref_taxa, {}, "f", False)
    assert out[:3] == ["Reference contains unknown taxon, not known to taxonomy: 5. It will be filtered out.", "Filtered reference size: 4",
                       "--------f--------"]
    # a header line is the first non-empty one; other columns
    rows, _ = cm.reference_rows(b"\nid\ttaxon\nq\t3\n", id_col=1, taxon_col=2, header=True)
    assert rows == {b"q": 3}


def test_the_join_is_on_the_raw_test_id():
    rows, _ = cm.reference_rows(b"x\tr1/1\t3\nx\tr2\t4\nx\tr3x/1\t3\nx\tr3\t4\n")
    assert rows == {b"r1": 3, b"r2": 4, b"r3x": 3, b"r3": 4}
    tests = cm.kraken_rows(b"C\tr1\t3\t100\t3:1\nC\tr1/1\t3\t100\t3:1\nU\tr2\t0\t100\t\nC\tr3\t3\t1\tz\nC\tr\t3\t1\tz\nC\tr3x/1\t3\t1\tz\n")
    pairs, ref_taxa, n_test, n_joined = cm.join(rows, tests)
    assert pairs == {(3, 3): 1, (4, 0): 1, (4, 3): 1} and ref_taxa == {3: 2, 4: 2} and (n_test, n_joined) == (6, 3)


def test_bad_lines_and_duplicates():
    for bad in (b"x\tr1\n", b"x\t\t3\n", b"x\tr1\t\n", b"x\tr1\t12x\n", b"x\tr1\t2147483648\n", b"x\tr1\t-1\n", b"x\tr1\t \n"):
        with pytest.raises(cm.CompareError) as e:
            cm.reference_rows(b"x\tok\t3\n" + bad)
        assert (e.value.kind, e.value.offset) == (cm.BAD_LINE, 7)
    assert cm.reference_rows(b"x\tr1\t+7\n")[0] == {b"r1": 7} and cm.reference_rows(b"x\tr1\t2147483647\n")[0] == {b"r1": 2**31 - 1}
    with pytest.raises(cm.CompareError) as e:
        cm.reference_rows(b"x\tr1/1\t3\nx\tr1\t3\n")               # equal only after /1 removal: still twice
    assert e.value.kind == cm.DUPLICATE_REFERENCE and e.value.offset == 9
    rows, _ = cm.reference_rows(b"x\tr1\t3\n")
    with pytest.raises(cm.CompareError) as e:
        cm.join(rows, cm.kraken_rows(b"C\tr1\t3\nC\tr9\t3\nC\tr1\t4\n"))
    assert e.value.kind == cm.DUPLICATE_TEST and e.value.offset == 14
    assert cm.join(rows, cm.kraken_rows(b"C\tr9\t3\nC\tr9\t3\n"))[0] == {}        # an unjoined id may repeat
    tax = cm.Taxonomy([(1, 1, "root"), (2, 1, "genus")])
    with pytest.raises(cm.CompareError) as e:
        cm.location_metrics(tax, {3: 1}, {}, "f", False)
    assert e.value.kind == cm.TAXON_RANGE


@pytest.mark.parametrize("rows,counted", [(9, False), (10, True)])
def test_a_taxon_counts_with_ten_reads(rows, counted):
    # truth: species 3 and 6; the classifier reports 3 for `rows` reads and genus 2 (vague at species level: no ancestor there) for 12
    ref_by_taxon = {3: 20, 6: 5}
    joined = {(3, 3): rows, (3, 2): 12, (6, 5): 10}
    (cmp_n, ref_n, precision, recall), out = cm.per_taxon(SIX, ref_by_taxon, joined, cm.SPECIES)
    # 5 is S2 below 3: ten reads at 5 count for 3 at the species level, so 3 is found either way; without them:
    assert (cmp_n, ref_n, precision, recall) == (1, 2, 1.0, 0.5)
    joined = {(3, 3): rows, (6, 2): 12}
    (cmp_n, ref_n, precision, recall), out = cm.per_taxon(SIX, ref_by_taxon, joined, cm.SPECIES)
    if counted:
        assert (cmp_n, ref_n, precision, recall) == (1, 2, 1.0, 0.5) and out[2] == "TP 1, VP 0 FP 0, FN 1}"
    else:
        assert (cmp_n, ref_n) == (0, 2) and math.isnan(precision) and recall == 0.0 and out[2] == "TP 0, VP 0 FP 0, FN 2}"
        assert out[3] == "Precision NaN% recall 0.00%"
    # at genus level the genus is the truth's ancestor: ref = {2}, and the 12 genus reads find it
    (cmp_n, ref_n, precision, recall), out = cm.per_taxon(SIX, ref_by_taxon, joined, cm.GENUS)
    assert (cmp_n, ref_n, precision, recall) == (1, 1, 1.0, 1.0)
    assert out[0] == "*** Per taxon comparison (minimum 10) at level Some(Genus)" and out[1] == "Total ref taxa 1, total classified taxa 1"


def test_vague_and_false_taxa():
    tax = cm.Taxonomy([(1, 1, "root"), (2, 1, "genus"), (3, 2, "species"), (6, 2, "species"), (7, 1, "genus"), (8, 7, "species")])
    # truth {3}; found: 3 (true), 6 (false), 8 (false); at genus level truth {2}, found 2 (true) and 7 (false)
    joined = {(3, 3): 10, (3, 6): 10, (3, 8): 11, (3, 2): 50, (3, 1): 50}
    m, out = cm.per_taxon(tax, {3: 100}, joined, cm.SPECIES)
    assert m == (3, 1, 1 / 3, 1.0) and out[2] == "TP 1, VP 0 FP 2, FN 0}" and out[3] == "Precision 33.33% recall 100.00%"
    m, out = cm.per_taxon(tax, {3: 100}, joined, cm.GENUS)
    assert m == (2, 1, 0.5, 1.0) and out[2] == "TP 1, VP 0 FP 1, FN 0}"
    # a vague taxon is an ancestor of a truth taxon that is no truth taxon itself: truth {3} and {7}'s species 8 at genus level
    m, out = cm.per_taxon(tax, {2: 5, 8: 5}, {(8, 7): 10, (2, 2): 10}, cm.GENUS)
    assert m == (2, 2, 1.0, 1.0)


def test_java_numbers():
    for x, s in [(0.5, "0.5"), (1.0, "1.0"), (0.0, "0.0"), (100.0, "100.0"), (1 / 3, "0.3333333333333333"), (2 / 3, "0.6666666666666666"),
                 (0.001, "0.001"), (0.0009, "9.0E-4"), (1.234e-5, "1.234E-5"), (9999999.0, "9999999.0"), (1e7, "1.0E7"), (1.25e10, "1.25E10"),
                 (123456.789, "123456.789"), (-0.75, "-0.75"), (8.4, "8.4"), (math.nan, "NaN"), (math.inf, "Infinity"), (-math.inf, "-Infinity")]:
        assert cm.java_double(x) == s
    for x, s in [(0.5, "50.00%"), (1.0, "100.00%"), (0.0, "0.00%"), (0.00125, "0.13%"), (0.12345, "12.35%"), (2 / 3, "66.67%"),
                 (0.99995, "100.00%"), (math.nan, "NaN%"), (math.inf, "Infinity%")]:
        assert cm.format_perc(x) == s


def test_titles_and_rows():
    assert cm.title_of("out/fam/grp/std_35_31_s7_c0.15_classified/sample=S1", True) == "fam/grp/std_35_31_s7_c0.15_classified/sample=S1"
    assert cm.title_of("a/b/part-0.txt", False) == "part-0.txt" and cm.title_of("b/sample=1/", True) == "b/sample=1"
    tm, rm = (3, 4, 0.75, math.nan), (90, 100, 80, 5, 5, 10, 80 / 85, 0.8, 1.25)
    row, complaint = cm.metrics_row("fam/grp/std_35_31_s7_c0.15_classified/sample=S1", cm.GENUS, tm, rm)
    assert complaint is None
    assert row == ("fam/grp/std_35_31_s7_c0.15_classified/sample=S1\tfam\tgrp\tS1\tstd\t35\t31\t0\t0\t7\t0.15\tGenus\t3\t4\t0.75\tNaN\t"
                   "90\t100\t80\t5\t5\t10\t0.9411764705882353\t0.8\t1.25")
    assert len(row.split("\t")) == len(cm.HEADER.split("\t")) == 25
    # the library's name may hold underscores and digits; the greedy groups take the last ones
    row, _ = cm.metrics_row("x/f/g/my_lib_2_35_31_s7_c0.00_classified/sample=a=b", cm.SPECIES, tm, rm)
    assert row.split("\t")[1:7] == ["x/f", "g", "a=b", "my_lib_2", "35", "31"]
    for title in ("part-0.txt", "grp/std_35_31_s7_c0.15_classified/sample=S1", "fam/grp/std_35_31_s7_c0.15/sample=S1",
                  "fam/grp/std_35_31_s7_c0.15_classified/sample=S1\n"):
        row, complaint = cm.metrics_row(title, cm.GENUS, tm, rm)
        assert row is None and complaint == f"Couldn't extract variables from filename: {title}. Omitting from output."


def test_run_on_a_tree(tmp_path):
    import compare_cases as cc
    import numpy as np
    rng = np.random.default_rng(5)
    tax_dir = cc.write_taxonomy(tmp_path / "tax")
    ref, test = cc.case(rng)
    (tmp_path / "truth.tsv").write_bytes(ref)
    (tmp_path / "part-0.txt").write_bytes(test)
    stdout, tsv = cm.run(tax_dir, str(tmp_path / "truth.tsv"), str(tmp_path / "o"), test_files=[str(tmp_path / "part-0.txt")])
    assert tsv == cm.HEADER + "\n" and (tmp_path / "o_metrics.tsv").read_text() == tsv       # --test-files: the header alone
    lines = stdout.split("\n")
    assert lines[0].startswith("Reference contains unknown taxon") and "Filtered reference size: " in stdout
    assert lines[-3:-1] == [f"Couldn't extract variables from filename: part-0.txt. Omitting from output."] * 2 and lines[-1] == ""
    assert "*** Per-read comparison at level Some(Genus)" in stdout and "*** Per taxon comparison (minimum 10) at level Some(Species)" in stdout
