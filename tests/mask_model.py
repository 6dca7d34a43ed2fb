"""Low-complexity masking (symmetric DUST, Morgulis et al. 2006) stated twice in integer Python, for the tests of
slacken_amd/csrc/mask.hip and slacken_amd/host/mask.hpp:

  mask_brute   the definition, literally: every interval of every run is scored and compared with every one of its sub-intervals;
  mask_dp      the recurrence M(a, b) = max(score(a, b), M(a + 1, b), M(a, b - 1)) that the engine runs.

Both take the layout of slk_index_add_sequences -- sequence i is bases[offsets[i] .. offsets[i+1]), no whitespace -- and return
(masked bases, letters changed).  No floating point, no division: scores are pairs (S, l - 1) compared by cross-multiplication."""
import numpy as np

CODE = {c: v for v, cs in enumerate(("Aa", "Cc", "Gg", "TtUu")) for c in cs.encode()}


def runs_of(seq):
    """(start, end) of every maximal run of valid letters (ACGTU, either case) of one sequence"""
    out, start = [], None
    for i, c in enumerate(seq):
        if c in CODE:
            if start is None:
                start = i
        elif start is not None:
            out.append((start, i))
            start = None
    if start is not None:
        out.append((start, len(seq)))
    return out


def triplets_of(run):
    return [CODE[run[i]] << 4 | CODE[run[i + 1]] << 2 | CODE[run[i + 2]] for i in range(len(run) - 2)]


def score(trip, a, b):
    """S of the interval [a, b] of triplets: sum over the triplet values of c (c - 1) / 2"""
    counts = {}
    for v in trip[a:b + 1]:
        counts[v] = counts.get(v, 0) + 1
    return sum(c * (c - 1) // 2 for c in counts.values())


def run_mask_brute(run, window, threshold):
    """True for every letter of the run that lies in a perfect interval"""
    trip, marks = triplets_of(run), [False] * len(run)
    for a in range(len(trip)):
        for b in range(a + 1, min(len(trip), a + window - 2)):
            l, s = b - a + 1, score(trip, a, b)
            if not 10 * s > threshold * (l - 1):
                continue
            if all(score(trip, a2, b2) * (l - 1) <= s * (b2 - a2) for a2 in range(a, b) for b2 in range(a2 + 1, b + 1)):
                for p in range(a, b + 3):
                    marks[p] = True
    return marks


def _check_parameters(window, threshold):
    if not 8 <= window <= 64 or not 1 <= threshold <= 255:
        raise ValueError("window 8..64, threshold 1..255")


def _replace(src, marks, replacement):
    out = src.copy()
    out[marks] = replacement if replacement else src[marks] | 0x20
    return out, int((out != src).sum())


_LUT = np.full(256, 4, np.int64)
for _c, _v in CODE.items():
    _LUT[_c] = _v


def dp_marks(bases, offsets, window, threshold):
    """The recurrence in lockstep, every start a of every run at the same length d = b - a: M(a, b - 1) is the start's own value of
    the step before and M(a + 1, b) its right neighbour's.  Integer numpy arrays over the letters; True for every masked letter."""
    src = np.asarray(bases, np.uint8)
    n = src.size
    marks = np.zeros(n, bool)
    if n < 3:
        return marks
    code = _LUT[src]
    pos = np.arange(n, dtype=np.int64)
    stop = code > 3                                   # a run cannot go on INTO such a letter: invalid, or the first of a sequence
    inner = np.asarray(offsets, np.int64)
    stop[inner[inner < n]] = True
    nxt = np.minimum.accumulate(np.where(stop, pos, n)[::-1])[::-1]
    run = np.where(code > 3, 0, np.append(nxt[1:], n) - pos)          # valid letters from here to the end of the run
    steps = np.clip(np.minimum(run, window) - 3, 0, None)            # lengths d = 1 .. steps: [a, a + d] needs letters a .. a + d + 2
    pad = np.append(code, [0, 0])
    trip = (pad[:-2] << 4 | pad[1:-1] << 2 | pad[2:]) & 63
    counts = np.zeros((n, 64), np.int16)
    live = np.nonzero(steps > 0)[0]
    counts[live, trip[live]] = 1
    S, mS, mD, reach = np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64), np.zeros(n, np.int64)   # M of one triplet: (0, 1)
    for d in range(1, window - 2):
        a = np.nonzero(steps >= d)[0]
        if a.size == 0:
            break
        v = trip[a + d]
        c = counts[a, v].astype(np.int64)
        S[a] += c
        counts[a, v] = c + 1
        uS, uD, lS, lD, s = mS[a + 1], mD[a + 1], mS[a], mD[a], S[a]   # (the neighbour's value is still the step before's: written below)
        up = uS * lD > lS * uD
        bS, bD = np.where(up, uS, lS), np.where(up, uD, lD)
        on_top = s * bD >= bS * d                                      # a tie keeps the interval
        perfect = on_top & (10 * s > threshold * d)
        reach[a[perfect]] = d + 3
        mS[a], mD[a] = np.where(on_top, s, bS), np.where(on_top, d, bD)
    until = np.maximum.accumulate(np.where(reach > 0, pos + reach, 0))
    return until > pos


def mask_brute(bases, offsets, window=64, threshold=20, replacement=ord("x")):
    """the definition, literally, run by run"""
    _check_parameters(window, threshold)
    src = np.asarray(bases, np.uint8)
    raw, marks = bytes(src), np.zeros(src.size, bool)
    for i in range(len(offsets) - 1):
        o = int(offsets[i])
        seq = raw[o:int(offsets[i + 1])]
        for r0, r1 in runs_of(seq):
            marks[o + r0:o + r1] = run_mask_brute(seq[r0:r1], window, threshold)
    return _replace(src, marks, replacement)


def mask_dp(bases, offsets, window=64, threshold=20, replacement=ord("x")):
    """the recurrence"""
    _check_parameters(window, threshold)
    src = np.asarray(bases, np.uint8)
    return _replace(src, dp_marks(src, offsets, window, threshold), replacement)


def mask_text(text, **kw):
    """one sequence given as str -> masked str (for the known answers)"""
    b = np.frombuffer(text.encode(), np.uint8)
    return bytes(mask_dp(b, [0, len(b)], **kw)[0]).decode()


def revcomp(text):
    return text[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


# ---- generators of the families the tests share: each holds masked and unmasked letters under the model ----
def skewed(rng, n, alphabet):
    """uniform draws from a multiset such as AAAC: homopolymer stretches beside mixed text"""
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def planted(rng, n, n_repeats=3, max_unit=4, min_len=20, max_len=60):
    """uniform ACGT with short tandem repeats planted at random places"""
    s = list(skewed(rng, n, "ACGT"))
    for _ in range(n_repeats):
        unit = skewed(rng, int(rng.integers(1, max_unit + 1)), "ACGT")
        ln = int(rng.integers(min_len, max_len + 1))
        at = int(rng.integers(0, max(1, n - ln)))
        for i in range(min(ln, n - at)):
            s[at + i] = unit[i % len(unit)]
    return "".join(s)
