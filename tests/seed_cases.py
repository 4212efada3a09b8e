"""Seeds: the expected answers and the case builders of test_seed_cpu.py and test_gpu_seed.py (test
infrastructure; numpy only, no GPU, no product import).

Semantics (include/kmer_hash_amd.h kh_seed_*): read r is the bytes [off[r], min(off[r+1], len)); window i
of it counts when i + k <= the read's end; i continues i-1 when both count, both are located (their
value is not KH_LOC_NONE) and v[i] == v[i-1] + 1; a run is a maximal chain of continuations; the seed
is the longest run, the first on a tie: {start in the read, v at the run's first window, run,
located windows}, {NONE, NONE, 0, 0} without a located window. The values come from
locate_cases.expected_locate_text, so everything here comes from the text alone."""
import numpy as np

import locate_cases as lc
import text_cases as tc

LOC_NONE = lc.LOC_NONE
SEED_WORDS = 4
EMPTY = (LOC_NONE, LOC_NONE, 0, 0)
_cache = {}


def expected_seeds(k, pos, read_off):
    """uint64 [n, 4] of a position array (one value per text byte) and n + 1 read offsets."""
    pos = np.asarray(pos, dtype=np.uint64)
    n = len(pos)
    off = [int(x) for x in np.asarray(read_off, dtype=np.uint64)]
    out = np.zeros((len(off) - 1, SEED_WORDS), np.uint64)
    for r in range(len(off) - 1):
        b, e = min(off[r], n), min(off[r + 1], n)
        best, located = None, 0  # best: (run, start, value)
        start = value = run = 0
        prev = LOC_NONE
        for i in range(b, e - k + 1):  # i + k <= e
            v = int(pos[i])
            if v != LOC_NONE:
                located += 1
                if prev != LOC_NONE and v == prev + 1:
                    run += 1
                else:
                    start, value, run = i - b, v, 1
                if best is None or run > best[0]:  # strictly longer: a tie keeps the first
                    best = (run, start, value)
            prev = v
        out[r] = (best[1], best[2], best[0], located) if best else EMPTY
    return out


def runs_of(k, pos, b, e):
    """Every run of the read [b, e) as (start in the read, value, length), in order."""
    runs = []
    prev = LOC_NONE
    for i in range(b, min(e, len(pos)) - k + 1):
        v = int(pos[i])
        if v != LOC_NONE:
            if prev != LOC_NONE and v == prev + 1:
                runs[-1][2] += 1
            else:
                runs.append([i - b, v, 1])
        prev = v
    return [tuple(x) for x in runs]


def line_starts(text):
    buf = tc.as_buf(text)
    return np.concatenate([[0], np.flatnonzero(buf == 10)[:-1] + 1]).astype(np.uint64) if len(buf) else \
        np.zeros(0, np.uint64)


def expected_coverage(k, text, seeds, reads=None, bases=None):
    """(reads, bases) uint64 [lines of the newline-terminated text], added to the arrays given."""
    starts = line_starts(text)
    n = len(tc.as_buf(text))
    reads = np.zeros(len(starts), np.uint64) if reads is None else reads.copy()
    bases = np.zeros(len(starts), np.uint64) if bases is None else bases.copy()
    for _, v, run, _ in np.asarray(seeds, dtype=np.uint64).reshape(-1, SEED_WORDS).tolist():
        if run > 0 and v < n:  # KH_LOC_NONE is never below
            line = int(np.searchsorted(starts, np.uint64(v), side="right")) - 1
            reads[line] += np.uint64(1)
            bases[line] += np.uint64(run + k - 1)
    return reads, bases


def join_reads(reads, sep=b"\n"):
    """Reads (bytes) -> (text, uint64 [n + 1] offsets); each read's bytes and its separator are the read."""
    off, parts = [0], []
    for x in reads:
        parts.append(x + sep)
        off.append(off[-1] + len(x) + len(sep))
    return b"".join(parts), np.array(off, np.uint64)


def expected_for(k, d, text, read_off):
    """The model's seeds of a text against a position dict (locate_cases.position_dict)."""
    return expected_seeds(k, lc.expected_locate_text(k, d, text)[0], read_off)


# ---- case builders over text_cases.contig_case(k) ------------------------------------------------
def substitute(read, at):
    """The read with the base at `at` changed (A -> C -> G -> T -> A)."""
    nxt = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    return read[:at] + nxt[read[at]] + read[at + 1:]


def longest(k):
    """The longest contig of contig_case(k) (300 k-mers) and its offset in the contig text."""
    case = tc.contig_case(k)
    c = max(case["contigs"], key=len)
    return c.encode(), case["truth"].index(c.encode() + b"\n")


WINDOW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129)  # the 64-position chunk edges


def length_reads(k):
    """Substrings of the longest contig with WINDOW_COUNTS windows, each from another start:
    [(read, its offset in the contig text)]."""
    c, at = longest(k)
    return [(c[7 * j:7 * j + w + k - 1], at + 7 * j) for j, w in enumerate(WINDOW_COUNTS)]


def carry_reads(k, windows=200):
    """One substitution in a read of `windows` windows, so that a run ends at window 62, 63 or 64
    (the base at w + k changes: windows w+1 .. w+k die) or begins there (the base at s - 1 changes:
    windows s-k .. s-1 die): [(read, (first run, second run))]."""
    c, _ = longest(k)
    read = c[3:3 + windows + k - 1]
    out = []
    for w in (62, 63, 64):
        out.append((substitute(read, w + k), (w + 1, windows - (w + k + 1))))
    for s in (62, 63, 64):
        out.append((substitute(read, s - 1), (max(s - k, 0), windows - s)))
    return out


def tie_reads(k):
    """One substitution that leaves two runs: equal halves (40, 40), the longer first (70, 30), the
    longer second (30, 70): [(read, (first run, second run))]."""
    c, _ = longest(k)
    out = []
    for a, b in ((40, 40), (70, 30), (30, 70)):
        read = c[5:5 + a + k + b + k - 1]  # a windows, k dead ones, b windows
        out.append((substitute(read, a + k - 1), (a, b)))
    return out


def chimeric_reads(k):
    """Pieces of two contigs joined: the k - 1 windows over the joint hold no k-mer of the table:
    [(read, (windows of the first piece, of the second))]."""
    case = tc.contig_case(k)
    two = sorted(case["contigs"], key=len)[-2:]
    x, y = two[0].encode(), two[1].encode()
    out = []
    for a, b in ((90, 40), (40, 90)):
        end = 2 + a + k - 1
        # the second piece starts where neither piece's run goes on by one base into the other
        s = next(s for s in range(4, 40) if y[s] != x[end] and y[s - 1] != x[end - 1])
        out.append((x[2:end] + y[s:s + b + k - 1], (a, b)))
    return out


def long_read(k):
    """The 20 000-base line of text_cases.tile_case with three substitutions: (read, the runs' lengths)."""
    c = tc.tile_case(k)["contig"].encode()
    cuts = (5000, 5000 + 64 * 40 + k, 17011)
    read = c
    for at in cuts:
        read = substitute(read, at)
    w = len(c) - k + 1
    edges = [0] + [x for at in cuts for x in (at - k + 1, at + 1)] + [w]
    return read, tuple(edges[j + 1] - edges[j] for j in range(0, len(edges), 2))
