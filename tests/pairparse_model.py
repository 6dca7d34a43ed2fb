"""The lockstep pairing of two mate files as the device route defines it, restated over the records that
hostmodel.parse_fasta / parse_fastq give: PairedInputReader.getFragments (S/kmers/input/InputReader.scala:105-131) while both files list
their mates in the same order."""
import hostmodel

MODEL = {"fasta": hostmodel.parse_fasta, "fastq": hostmodel.parse_fastq}


def strip(title, suffix):
    """header.replaceAll(suffix + "$", ""): ONE trailing suffix is removed"""
    return title[:-len(suffix)] if title.endswith(suffix) else title


def lockstep(records1, records2):
    """records: [(title, seq)] -> (pairs [(title, seq1, seq2)], P, mismatch): the leading records whose titles agree once "/1" is taken off
    the first and "/2" off the second; mismatch: the walk stopped before the shorter list ended."""
    M = min(len(records1), len(records2))
    pairs = []
    for (t1, s1), (t2, s2) in zip(records1, records2):
        if strip(t1, "/1") != strip(t2, "/2"):
            break
        pairs.append((strip(t1, "/1"), s1, s2))
    return pairs, len(pairs), len(pairs) < M


def lockstep_texts(text1, fmt1, text2, fmt2):
    return lockstep(MODEL[fmt1](text1), MODEL[fmt2](text2))
