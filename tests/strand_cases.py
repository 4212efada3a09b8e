"""Seeds on both strands: the expected answers and the case builders of test_strand_cpu.py and
test_gpu_strand.py (test infrastructure; numpy only, no GPU, no product import).

Semantics (include/kmer_hash_amd.h kh_locate_text_rc*, kh_seed_strand_*): rc(window) = the k bases in
reverse order, each complemented. w[i] = the position of rc(window i), KH_LOC_NONE where i has no
window or the k-mer is not located; v[i] = kh_locate_text's answer. Forward runs as in seed_cases. On
the reverse strand i continues i-1 when both are counted windows of the read, both located and
w[i-1] == w[i] + 1. The strand seed is the longer of the longest forward run and the longest reverse
run (the first on a tie within a strand, the forward one on a tie between them):
{start, value, run, strand, located_fwd, located_rc}, value = v at the run's first window (forward) or
w at its last window (reverse); {NONE, NONE, 0, 0, 0, 0} without a located window. Everything here
comes from the text alone."""
import numpy as np

import locate_cases as lc
import seed_cases as sc
import text_cases as tc
from cases import contigs_lines

LOC_NONE = lc.LOC_NONE
STRAND_WORDS = 6
EMPTY = (LOC_NONE, LOC_NONE, 0, 0, 0, 0)
_PAIR = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}
_cache = {}


def revcomp(text):
    """The bytes in reverse order, A<->T and C<->G swapped, every other byte kept."""
    return bytes(_PAIR.get(x, x) for x in reversed(bytes(tc.as_buf(text).tobytes())))


def expected_locate_text_rc(k, d, text):
    """(w uint64 [len], windows, located) of a query text against the position dict: for each window,
    d's position of the window's bases reversed and complemented."""
    buf = tc.as_buf(text)
    out = np.full(len(buf), LOC_NONE, np.uint64)
    at = np.flatnonzero(tc.window_mask(k, buf))
    if len(at):
        comp = np.arange(256, dtype=np.uint8)
        for a, b in _PAIR.items():
            comp[a] = b
        rcw = comp[buf[at[:, None] + (k - 1 - np.arange(k))[None, :]]]  # [m, k]: each window, rc
        got = lc.expected_locate(k, d, tc.pack_windows(k, rcw.ravel(), np.arange(len(at)) * k))
        out[at] = got
    located = int((out[at] != LOC_NONE).sum()) if len(at) else 0
    return out, len(at), located


def mirrored(k, u):
    """An answer u over revcomp(text) mirrored back onto the text: w[i] = u[len - k - i] for
    i <= len - k, NONE after that."""
    u = np.asarray(u, dtype=np.uint64)
    n = len(u)
    w = np.full(n, LOC_NONE, np.uint64)
    m = max(n - k + 1, 0)
    w[:m] = u[:m][::-1]
    return w


def expected_strand_seeds(k, v, w, read_off):
    """uint64 [n, 6] of two position arrays (one value per text byte each) and n + 1 read offsets."""
    v, w = np.asarray(v, dtype=np.uint64), np.asarray(w, dtype=np.uint64)
    assert len(v) == len(w)
    n = len(v)
    off = [int(x) for x in np.asarray(read_off, dtype=np.uint64)]
    out = np.zeros((len(off) - 1, STRAND_WORDS), np.uint64)
    for r in range(len(off) - 1):
        b, e = min(off[r], n), min(off[r + 1], n)
        bf = br = None  # best: (run, start, value)
        lf = lr = 0
        fs = fv = fr = 0
        rs = rr = 0
        pv = pw = LOC_NONE
        for i in range(b, e - k + 1):  # i + k <= e
            x, y = int(v[i]), int(w[i])
            if x != LOC_NONE:
                lf += 1
                if pv != LOC_NONE and x == pv + 1:
                    fr += 1
                else:
                    fs, fv, fr = i - b, x, 1
                if bf is None or fr > bf[0]:
                    bf = (fr, fs, fv)
            if y != LOC_NONE:
                lr += 1
                if pw != LOC_NONE and pw == y + 1:
                    rr += 1
                else:
                    rs, rr = i - b, 1
                if br is None or rr > br[0]:
                    br = (rr, rs, y)  # y: the value at the run's last window so far, its smallest
            pv, pw = x, y
        if bf is None and br is None:
            out[r] = EMPTY
        elif br is None or (bf is not None and bf[0] >= br[0]):
            out[r] = (bf[1], bf[2], bf[0], 0, lf, lr)
        else:
            out[r] = (br[1], br[2], br[0], 1, lf, lr)
    return out


def rev_runs_of(k, w, b, e):
    """Every reverse run of the read [b, e) as (start in the read, value at its last window, length)."""
    runs = []
    prev = LOC_NONE
    for i in range(b, min(e, len(w)) - k + 1):
        y = int(w[i])
        if y != LOC_NONE:
            if prev != LOC_NONE and prev == y + 1:
                runs[-1][1], runs[-1][2] = y, runs[-1][2] + 1
            else:
                runs.append([i - b, y, 1])
        prev = y
    return [tuple(x) for x in runs]


def expected_for(k, d, text, read_off):
    """The model's strand seeds of a text against a position dict."""
    return expected_strand_seeds(k, lc.expected_locate_text(k, d, text)[0], expected_locate_text_rc(k, d, text)[0],
                                 read_off)


def repacked(seeds):
    """[n, 6] strand seeds -> the [n, 4] seeds kh_seed_coverage_dev takes."""
    s = np.asarray(seeds, dtype=np.uint64).reshape(-1, STRAND_WORDS)
    return np.ascontiguousarray(np.concatenate([s[:, :3], (s[:, 4] + s[:, 5])[:, None]], axis=1))


# ---- case builders over text_cases.contig_case(k) ------------------------------------------------
def rc_length_reads(k):
    """revcomp of seed_cases.length_reads: [(read, offset of the substring in the contig text, windows)]."""
    return [(revcomp(read), at, w) for (read, at), w in zip(sc.length_reads(k), sc.WINDOW_COUNTS)]


def rc_carry_reads(k, windows=200):
    """revcomp of seed_cases.carry_reads(k), re-cut so that the DESCENDING run ends at window 62, 63 or
    64 of the read, or begins there: the forward read's runs (a, b) come out as (b, a), so the read is
    built from a forward read whose second run has the wanted length:
    [(read, (first reverse run, second reverse run))]."""
    c, _ = sc.longest(k)
    fwd = c[3:3 + windows + k - 1]
    out = []
    for w in (62, 63, 64):  # the first reverse run is windows 0 .. w: the forward read's last w + 1 windows
        out.append((revcomp(sc.substitute(fwd, windows - (w + 1) - 1)), (w + 1, windows - (w + 1) - k)))
    for s in (62, 63, 64):  # the second reverse run begins at window s: the forward read's first windows - s
        out.append((revcomp(sc.substitute(fwd, windows - s + k - 1)), (max(s - k, 0), windows - s)))
    return out


CHOICES = ((40, 40), (70, 30), (30, 70))


def choice_reads(k):
    """A forward piece of one contig and a reverse-complemented piece of another, joined in both
    orders, (a, b) = (forward windows, reverse windows) of CHOICES. The second contig's piece is
    chosen, by the model, so that the k - 1 joint windows lengthen neither run:
    [(read, (a, b), "fr" or "rf")]."""
    if ("choice", k) in _cache:
        return _cache[("choice", k)]
    case = tc.contig_case(k)
    d = lc.position_dict(k, case["truth"])
    two = sorted(case["contigs"], key=len)[-2:]
    x, y = two[0].encode(), two[1].encode()
    out = []
    for a, b in CHOICES:
        for order in ("fr", "rf"):
            for s in range(4, 60):
                f, r = x[2:2 + a + k - 1], revcomp(y[s:s + b + k - 1])
                read = f + r if order == "fr" else r + f
                v = lc.expected_locate_text(k, d, read)[0]
                w = expected_locate_text_rc(k, d, read)[0]
                fl = [t[2] for t in sc.runs_of(k, v, 0, len(read))]
                rl = [t[2] for t in rev_runs_of(k, w, 0, len(read))]
                if fl == [a] and rl == [b]:
                    out.append((read, (a, b), order))
                    break
            else:
                raise AssertionError(("no joint without a chance continuation", k, a, b, order))
    _cache[("choice", k)] = out
    return out


def shares_no_kmer(k, lines):
    """No k-mer stands twice in the lines (bytes each), within a line or across them."""
    seen = set()
    for line in lines:
        for i in range(len(line) - k + 1):
            x = line[i:i + k]
            if x in seen:
                return False
            seen.add(x)
    return True


def both_strands_case(k, n_contigs=4, seed=None):
    """A table that holds both strands: a few contigs of contig_case(k) and their revcomp as separate
    lines, chosen so that no k-mer stands twice in the line set: {"k", "lines" (the input text),
    "recs", "contigs", "truth"}."""
    key = ("both", k, n_contigs, seed)
    if key not in _cache:
        rng = np.random.default_rng(6300 + k if seed is None else seed)
        pool = [c for c in tc.contig_case(k)["contigs"] if len(c) >= k + 80]
        chosen = []
        for c in pool:
            trial = chosen + [c, revcomp(c.encode()).decode()]
            if shares_no_kmer(k, [t.encode() for t in trial]):
                chosen = trial
            if len(chosen) == 2 * n_contigs:
                break
        assert len(chosen) == 2 * n_contigs
        lines, contigs = contigs_lines(k, chosen, rng)
        _cache[key] = {"k": k, "lines": lines, "recs": tc.records_from_lines(k, lines), "contigs": contigs,
                       "truth": "".join(c + "\n" for c in contigs).encode()}
    return _cache[key]


def made_up_arrays(seed=78):
    """Two position arrays no index gave (v forward, w reverse) for kh_seed_strand_runs_dev: descending
    runs in w of every length round 64 and 128, a run that reaches 0 followed by NONE, ...FFFE next to
    NONE, values with rank bits above 2^48, an ascending run in w and a descending one in v (neither
    counts), and forward runs in v between them: (v, w)."""
    rng = np.random.default_rng(seed)
    vp, wp = [], []

    def both(vs, ws):
        assert len(vs) == len(ws)
        vp.append(np.asarray(vs, dtype=np.uint64))
        wp.append(np.asarray(ws, dtype=np.uint64))

    none = lambda n: np.full(n, LOC_NONE, np.uint64)  # noqa: E731
    for length in list(range(1, 6)) + [62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193, 300, 64, 64, 1]:
        base = (int(rng.integers(0, 8)) << 48) | int(rng.integers(1000, 2 ** 40))
        down = (base + length - 1 - np.arange(length)).astype(np.uint64)
        fl = int(rng.integers(0, length + 1))  # a forward run beside it, shorter, equal or absent
        fv = none(length)
        fv[:fl] = ((int(rng.integers(0, 8)) << 48) | int(rng.integers(0, 2 ** 40))) + np.arange(fl)
        both(fv, down)
        gap = int(rng.integers(0, 4))  # 0: the next run follows at once (its value does not)
        both(none(gap), none(gap))
    both(none(5), [4, 3, 2, 1, 0])                                   # down to 0 ...
    both(none(3), [LOC_NONE, LOC_NONE - 1, LOC_NONE])                # ... then NONE, ...FFFE, NONE
    both(none(3), [0, LOC_NONE, LOC_NONE - 1])                       # 0 is never continued
    both([9, 8, 7, 6, 5], [20, 21, 22, 23, 24])                      # descending v, ascending w: runs of 1
    both([LOC_NONE - 2, LOC_NONE - 1, LOC_NONE], [LOC_NONE - 1, LOC_NONE - 2, LOC_NONE - 3])
    both([5, 6, 7, LOC_NONE, LOC_NONE, LOC_NONE], [LOC_NONE, LOC_NONE, LOC_NONE, 9, 8, 7])  # a tie: forward
    both(none(200), none(200))
    return np.concatenate(vp), np.concatenate(wp)
