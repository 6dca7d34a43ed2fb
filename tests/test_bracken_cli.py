"""The host side of Bracken weights, without a GPU: the kmer_distrib writer (BrackenWeights.writeKmerDistrib,
S/slacken/BrackenWeights.scala:377-431) through `slacken-amd kmer-distrib`, and the command line of bracken-build and
classify2 --bracken-length."""
import subprocess

from test_host_cli import CLI, _built, run  # noqa: F401


def parse_kmer_distrib(text):
    """The file as Bracken's est_abundance.py reads it: a header line, then `dest \\t src:count:total src:count:total ...`"""
    lines = text.split("\n")
    assert lines[-1] == ""
    head, body = lines[0], lines[1:-1]
    assert head == "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers"
    out = {}
    for line in body:
        dest, rest = line.split("\t")
        for item in rest.split(" "):
            src, cnt, tot = item.split(":")
            out[(int(dest), int(src))] = (int(cnt), int(tot))
    return out


def kmer_distrib_of(triples):
    """The text the writer must give for {(dest, source): count}: dests ascending, sources ascending within a line"""
    total = {}
    for (d, s), c in triples.items():
        total[s] = total.get(s, 0) + c
    lines = ["mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers"]
    for d in sorted({d for d, _ in triples}):
        srcs = sorted(s for dd, s in triples if dd == d)
        lines.append(f"{d}\t" + " ".join(f"{s}:{triples[(d, s)]}:{total[s]}" for s in srcs))
    return "\n".join(lines) + "\n"


def test_kmer_distrib_writer(tmp_path):
    # the reference's expected triples for its tiny dataset (T/slacken/Testing.scala:171-173), given out of order and one split
    triples = [(455631, 455631, 3924809), (0, 455631, 201425), (0, 526997, 29747), (526997, 526997, 3040666),
               (1, 455631, 31), (0, 9606, 100000), (9606, 9606, 639961), (0, 9606, 59860)]
    f = tmp_path / "t.tsv"
    f.write_text("".join(f"{d}\t{s}\t{c}\n" for d, s, c in triples))
    text = run("kmer-distrib", f)
    assert text == ("mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n"
                    "0\t9606:159860:799821 455631:201425:4126265 526997:29747:3070413\n"
                    "1\t455631:31:4126265\n"
                    "9606\t9606:639961:799821\n"
                    "455631\t455631:3924809:4126265\n"
                    "526997\t526997:3040666:3070413\n")
    parsed = parse_kmer_distrib(text)
    assert parsed[(0, 9606)] == (159860, 799821)
    merged = {}
    for d, s, c in triples:
        merged[(d, s)] = merged.get((d, s), 0) + c
    assert text == kmer_distrib_of(merged)


def test_kmer_distrib_empty(tmp_path):
    f = tmp_path / "t.tsv"
    f.write_text("")
    assert run("kmer-distrib", f) == "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n"


def test_bracken_command_line():
    r = subprocess.run([CLI, "classify2", "--bracken-length", "100"], capture_output=True, text=True)
    assert r.returncode != 0
    assert "not supported" not in r.stderr and "usage: classify2" in r.stderr
    for bad in ("0", "-5"):
        r = subprocess.run([CLI, "classify2", "--bracken-length", bad], capture_output=True, text=True)
        assert r.returncode != 0 and "--bracken-length must be a positive" in r.stderr
    r = subprocess.run([CLI, "bracken-build", "-i", "x", "--library", "y", "--read-len", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "--read-len must be a positive" in r.stderr
    r = subprocess.run([CLI, "classify2", "--index-reports"], capture_output=True, text=True)
    assert "not supported" in r.stderr
    for args in ([], ["-i", "x"], ["--library", "y"]):
        r = subprocess.run([CLI, "bracken-build", *args], capture_output=True, text=True)
        assert r.returncode != 0 and "usage: bracken-build" in r.stderr
    r = subprocess.run([CLI, "bracken-build", "-i", "x", "--library", "y", "--shard-table"], capture_output=True, text=True)
    assert r.returncode != 0 and "--shard-table" in r.stderr
    assert "bracken-build" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
