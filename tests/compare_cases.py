"""What the tests of `compare` share: a small taxonomy with every shape the rank arithmetic meets, written as NCBI dump files, and
random reference mappings and classification texts over it."""
import os

import numpy as np

# (taxon, parent, rank title).  Species with sublevels (30 under 20 is ranked species too: S1; 31, 32 are strains without rank), a genus
# inside an unranked clade (14 in 13), a species without genus (25), ids the taxonomy does not define (6..9, 15..19, 26..29, 33..39).
NODES = [(1, 1, "no rank"), (2, 1, "superkingdom"), (3, 2, "phylum"), (4, 3, "family"), (5, 3, "family"),
         (10, 4, "genus"), (11, 4, "genus"), (12, 5, "genus"), (13, 5, "no rank"), (14, 13, "genus"),
         (20, 10, "species"), (21, 10, "species"), (22, 11, "species"), (23, 12, "species"), (24, 14, "species"), (25, 5, "species"),
         (30, 20, "species"), (31, 21, "no rank"), (32, 30, "no rank")]
MERGED = [(40, 20), (41, 12), (42, 39)]                            # 42 is merged into an id that is not defined
T = 43
REF_TAXA = [20, 21, 22, 23, 24, 25, 30, 31, 32, 40, 10, 14, 1, 7, 42, 33]     # where truth mappings point: mostly species and below
TEST_TAXA = [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 25, 30, 31, 32, 40, 41, 42, 8]


def write_taxonomy(d, nodes=NODES, merged=MERGED):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for t, p, rank in nodes:
            f.write(f"{t}\t|\t{p}\t|\t{rank}\t|\n")
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for t, _, _ in nodes:
            f.write(f"{t}\t|\tNode {t}\t|\t\t|\tscientific name\t|\n")
    with open(os.path.join(d, "merged.dmp"), "w") as f:
        for s, p in merged:
            f.write(f"{s}\t|\t{p}\t|\n")
    return str(d)


def read_ids(rng, n, sample="S0"):
    """n distinct ids in the style of CAMI's simulated reads; about a third are first mates and carry /1"""
    out = []
    for i in range(n):
        rid = f"{sample}R{int(rng.integers(0, 10**6)):06d}x{i}"
        out.append(rid + "/1" if rng.random() < 0.35 else rid)
    return out


def reference_text(rng, ids, taxa=REF_TAXA, eol=b"\n", second_mates=True):
    """a reads_mapping.tsv: anonymous id, read id, taxon, a trailing column; every first mate is followed by its /2 row"""
    lines = []
    for i, rid in enumerate(ids):
        t = int(rng.choice(taxa))
        lines.append(f"a{i}\t{rid}\t{t}\tgenome{t}".encode())
        if second_mates and rid.endswith("/1"):
            lines.append(f"a{i}\t{rid[:-2]}/2\t{t}\tgenome{t}".encode())
    return b"".join(line + eol for line in lines)


def classified_text(rng, ids, taxa=TEST_TAXA, eol=b"\n", hits_len=(1, 6)):
    """per-read lines as `classify` writes them: C/U, id, taxon, length, hit list"""
    lines = []
    for rid in ids:
        t = int(rng.choice(taxa))
        hits = " ".join(f"{int(rng.choice(taxa))}:{int(rng.integers(1, 40))}" for _ in range(int(rng.integers(*hits_len))))
        lines.append(f"{'C' if t else 'U'}\t{rid}\t{t}\t{int(rng.integers(80, 151))}\t{hits}".encode())
    return b"".join(line + eol for line in lines)


def case(rng, n_ref=300, n_test=260, n_absent=40, eol=b"\n"):
    """(reference text, test text): n_test of the reference's reads come back classified (under the id WITHOUT /1, as classify writes
    a pair), with n_absent reads the reference does not have; rows in random order"""
    ids = read_ids(rng, n_ref)
    ref = reference_text(rng, ids, eol=eol)
    back = [rid[:-2] if rid.endswith("/1") else rid for rid in rng.permutation(ids)[:n_test]]
    absent = [f"X{i}_{int(rng.integers(0, 10**6))}" for i in range(n_absent)]
    test = classified_text(rng, list(rng.permutation(back + absent)), eol=eol)
    return ref, test
