"""The rule that joins the HIT LISTS of the pieces of a split fragment, stated in Python on top of the oracle and of
pieces_model's record of a piece's two ends.

Each piece is taken through the oracle as a read of its own: its list holds one entry (taxon, k-mers) per span, in ordinal order.  The
fragment's list is the pieces' lists one after the other, except that an entry which a border cut in two is ONE entry:

  * where the piece DIRECTLY before ends inside a super-mer, this piece begins with a k-mer of a sequence run and the two keys are
    equal -- or where that piece ends inside an ambiguous span and this one begins inside one -- this piece's first entry is no entry
    of its own: its k-mers go to the last entry before it;
  * "the last entry before it" is the last entry of the list so far, wherever it came from: a piece that holds nothing but the
    continuation of an earlier entry contributes no entry, and the piece after it may continue the same entry again (20 000 Ns over
    pieces of 4 096 windows; one minimizer value throughout a fragment)."""
import pieces_model as pm


def piece_list(orc, p, oix, parents, bases):
    """[(taxon, k-mers)] of one piece, as the oracle lists a read's hits"""
    return orc.classify_read(p, oix, parents, bases.tobytes(), None, 2, 0.0)[1]


def cut_entry(prev, rec):
    """the border between two neighbouring pieces runs through one span (pieces_model.merge counts it once for the same reason)"""
    cut_supermer = prev["ends_open"] and rec["starts_seq"] and prev["last_key"] == rec["first_key"]
    cut_ambiguous = prev["end_amb"] and rec["first_amb"]
    return bool(cut_supermer or cut_ambiguous)


def stitch(records, lists):
    """the fragment's list from its pieces' records (pieces_model.piece_record) and lists.  Also -> per piece (where its entries begin
    in the list, whether its first entry was cut, the entries it stores): the plan the move kernel works from"""
    out, plan = [], []
    prev = None
    for rec, lst in zip(records, lists):
        lst = list(lst)
        cut = prev is not None and cut_entry(prev, rec)
        if cut:
            taxon, kmers = lst.pop(0)                 # (a cut entry is the piece's first: both rules look at its first window)
            assert out and out[-1][0] == taxon, "a cut entry continues an entry of the same taxon"
            out[-1] = (taxon, out[-1][1] + kmers)
        plan.append((len(out), cut, len(lst)))
        out += lst
        prev = rec
    return out, plan


def by_pieces(orc, p, oix, parents, read, piece_windows):
    pieces = [read[a:a + n] for a, n in pm.cut(len(read), p.k, piece_windows)]
    records = [pm.piece_record(orc, p, oix, b) for b in pieces]
    lists = [piece_list(orc, p, oix, parents, b) for b in pieces]
    for rec, lst in zip(records, lists):
        assert rec["n_out"] == len(lst)
    return stitch(records, lists)


def whole(orc, p, oix, parents, read):
    return orc.classify_read(p, oix, parents, read.tobytes(), None, 2, 0.0)[1]
