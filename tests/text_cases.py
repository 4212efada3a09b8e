"""Find over text: the expected answers and the case builders of test_find_text_cpu.py and
test_gpu_find_text.py (test infrastructure; numpy only, no GPU, no product import).

Semantics (include/kmer_hash_amd.h kh_find_text_dev): position i has a window iff bytes i .. i+k-1
lie in the text and are each one of A C G T; its answer is the {backward, forward} chars of the
k-mer's record, {0, 0} when no record has the k-mer, {0xFF, 0xFF} when there is no window."""
import re
import os

import numpy as np

from cases import RecordDict, contigs_text, contigs_truth

TEXT_NONE = 0xFF
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmer_hash_amd.h")
# the documented tile of the text kernels: the tile-edge cases are built around its multiples
TEXT_TILE = int(re.search(r"#define KH_TEXT_TILE (\d+)", open(_HDR).read()).group(1))

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def as_buf(text):
    if isinstance(text, np.ndarray):
        return np.ascontiguousarray(text, dtype=np.uint8).ravel()
    return np.frombuffer(bytes(text), dtype=np.uint8)


def window_mask(k, buf):
    """has[i] = position i has a window, from a running count of the non-ACGT bytes."""
    n = len(buf)
    has = np.zeros(n, bool)
    if n >= k:
        run = np.concatenate([[0], np.cumsum(_CODE[buf] > 3)])
        has[:n - k + 1] = (run[k:] - run[:n - k + 1]) == 0
    return has


def pack_windows(k, buf, pos):
    """pkmer_t bytes [m, PACKED] of the windows at `pos`: 2 bits per base, first base in the top bits
    of byte 0, A=0 C=1 G=2 T=3, the tail padded with 'A' (packing.hpp:77-92)."""
    KP = (k + 3) // 4
    out = np.zeros((len(pos), KP), np.uint8)
    for b0 in range(0, len(pos), 1 << 16):
        p = np.asarray(pos[b0:b0 + (1 << 16)], dtype=np.int64)
        c = np.zeros((len(p), 4 * KP), np.uint8)
        c[:, :k] = _CODE[buf[p[:, None] + np.arange(k)[None, :]]]
        assert (c < 4).all()
        c = c.reshape(len(p), KP, 4)
        out[b0:b0 + len(p)] = (c[:, :, 0] << 6) | (c[:, :, 1] << 4) | (c[:, :, 2] << 2) | c[:, :, 3]
    return out


def records_from_lines(k, text):
    """kmer_pair records [n, R] of fixed-width "KMER BF\\n" lines (read_kmers.hpp:62-76)."""
    buf = as_buf(text)
    w = k + 4
    n = len(buf) // w
    lines = buf[:n * w].reshape(n, w)
    return np.ascontiguousarray(np.concatenate(
        [pack_windows(k, buf, np.arange(n) * w), lines[:, k + 1:k + 3]], axis=1))


def expected_find_text(k, recs, text):
    """(ext uint8 [len, 2], windows, found) of the text against the records [n, R] (or a
    RecordDict of them), from the records alone."""
    KP = (k + 3) // 4
    buf = as_buf(text)
    ext = np.full((len(buf), 2), TEXT_NONE, np.uint8)
    pos = np.flatnonzero(window_mask(k, buf))
    keys = pack_windows(k, buf, pos)
    d = recs if isinstance(recs, RecordDict) else (RecordDict(k, recs) if len(recs) else None)
    if d is None:
        got, hit = np.zeros((len(pos), KP + 2), np.uint8), np.zeros(len(pos), np.uint8)
    else:
        got, hit = d.lookup(keys)
    ext[pos] = got[:, KP:KP + 2]  # an absent key's record is zeroed
    return ext, len(pos), int(hit.sum())


def classes(ext):
    """The answer classes a result holds."""
    none = (ext == TEXT_NONE).all(axis=1)
    absent = (ext == 0).all(axis=1)
    out = set()
    if none.any():
        out.add("none")
    if absent.any():
        out.add("absent")
    if (~none & ~absent).any():
        out.add("found")
    return out


def crosses_every_tile_edge(k, text, tile=None):
    """Every multiple T of the tile inside the text has a window [i, i + k) with i < T < i + k."""
    tile = tile or TEXT_TILE
    has = window_mask(k, as_buf(text))
    edges = range(tile, len(has), tile)
    return len(edges) > 0 and all(has[max(T - k + 1, 0):T].any() for T in edges)


# ---- case builders ------------------------------------------------------------------------------
K_COVER = (19, 29, 30, 31, 32, 51, 60)  # one / two-word slots, the hi_mask edge, both specialisations, KH_K_MAX
_cache = {}


def contig_case(k, seed=None):
    """About 40 contigs of 1 to 300 k-mers: {"k", "lines" (the input text), "recs", "contigs",
    "truth" (the contig text = the query)}. Built once per k."""
    seed = 4100 + k if seed is None else seed
    if (k, seed) not in _cache:
        rng = np.random.default_rng(seed)
        lens = [1, 300, 2, k, 2 * k + 1] + [int(x) for x in rng.integers(1, 301, 35)]
        lines, contigs = contigs_text(k, lens, seed)
        _cache[(k, seed)] = {"k": k, "lines": lines, "recs": records_from_lines(k, lines), "contigs": contigs,
                             "truth": contigs_truth(contigs)}
    return _cache[(k, seed)]


def neighbour_answers(k, text):
    """What a contig text's own k-mers answer: the bytes before and after each window, 'F' at the
    ends of a line (and of the text)."""
    buf = as_buf(text)
    n = len(buf)
    ext = np.full((n, 2), TEXT_NONE, np.uint8)
    for i in np.flatnonzero(window_mask(k, buf)):
        b = buf[i - 1] if i > 0 and buf[i - 1] != 10 else ord("F")
        f = buf[i + k] if i + k < n and buf[i + k] != 10 else ord("F")
        ext[i] = (b, f)
    return ext


def mutated_text(text, every=97, first=50):
    """The text with one base changed at every `every`-th position (where a base stands there)."""
    buf = as_buf(text).copy()
    nxt = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
    for i in range(first, len(buf), every):
        if int(buf[i]) in nxt:
            buf[i] = nxt[int(buf[i])]
    return buf.tobytes()


def dirty_text(k, contigs, seed=7):
    """Every way a text can be untidy around k-mers the table holds (contigs: strings, at least six
    of them with 3k bases or more)."""
    c = [x.encode() for x in contigs if len(x) >= 3 * k][:6]
    assert len(c) == 6
    rng = np.random.default_rng(seed)
    stranger = bytes(b"ACGT"[x] for x in rng.integers(0, 4, k + 5))  # k-mers the table does not hold
    parts = [
        b">read1 ACGT len=" + c[0][:k + 5] + b" x\n",       # a header line: its letters form windows
        b"\n", b"\n",                                        # empty lines
        c[0][:k - 1] + b"\n",                                # lines of k-1, k and k+1 bases
        c[0][:k] + b"\n",
        c[0][:k + 1] + b"\r\n",
        c[1][:10] + b"N" + c[1][11:2 * k + 10] + b"\n",      # N inside a line
        c[1][:k + 3].lower() + c[1][k + 3:2 * k + 8] + b"\n",  # lower case, then upper
        c[2][:k + 2] + b"F" + c[2][k + 3:3 * k] + b"\r\n",   # the extension alphabet's F is no base
        c[2][:k] + b" " + c[2][k:2 * k + 2] + b"  \n",       # spaces
        c[3][:k + 4] + b"\x00" + c[3][k + 5:2 * k + 9] + b"\xff" + c[3][2 * k + 10:3 * k] + b"\n",
        stranger + b"\n",
        b"n" + c[4][1:k + 3] + b"\n",                        # a bad byte at the first base of a present window
        c[4][:k - 1] + b"x" + c[4][k:2 * k + 1] + b"\n",     # ... and at the last
        c[5][:k + 7] + b"\n",
        c[5][3:k + 1],                                       # no trailing newline: ends mid-window (k-2 bases)
    ]
    return b"".join(parts)


def length_texts(k, contig):
    """Texts of 0, 1, k-1, k and k+1 bytes (bases of a contig the table holds)."""
    c = contig.encode()
    assert len(c) >= k + 1
    return [c[:n] for n in (0, 1, k - 1, k, k + 1)]


def tile_case(k, seed=None):
    """One contig of at least 3 tiles (20 000 bases when the tile is at most 4096 bytes): {"k",
    "lines", "recs", "contig"}."""
    bases = 20000 if TEXT_TILE <= 4096 else 3 * TEXT_TILE + 977
    seed = 5200 + k if seed is None else seed
    key = ("tile", k, seed)
    if key not in _cache:
        lines, contigs = contigs_text(k, [bases - k + 1], seed)
        _cache[key] = {"k": k, "lines": lines, "recs": records_from_lines(k, lines), "contig": contigs[0]}
    return _cache[key]


def tile_texts(case):
    """The long line preceded by 0..3 newline bytes."""
    return [b"\n" * pre + case["contig"].encode() for pre in range(4)]


POINTER_OFFSETS = (0, 1, 7, 15)

HOT_ARGS = dict(k=51, n=200_000, hot_permille=500, n_motifs=2, hot_flank=True, seed=1)


def hot_case(SyntheticKmers):
    """The hot-region set (the generator class is passed in: no product import here): {"k", "recs",
    "truth"}."""
    if "hot" not in _cache:
        a = dict(HOT_ARGS)
        g = SyntheticKmers(a.pop("k"), a.pop("n"), **a)
        _cache["hot"] = {"k": 51, "recs": g.records(), "truth": g.truth()}
        g.close()
    return _cache["hot"]


def shard_texts(k):
    """The four texts the sharded test hands round the ranks: dirty, mutated, empty, shorter than k."""
    case = contig_case(k)
    return [dirty_text(k, case["contigs"]), mutated_text(case["truth"]), b"", case["contigs"][0].encode()[:k - 1]]
