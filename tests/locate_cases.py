"""Locate: the expected answers and the case builders of test_locate_cpu.py and test_gpu_locate.py
(test infrastructure; numpy only, no GPU, no product import).

Semantics (include/kmer_hash_amd.h kh_locate_*): after kh_locate_build every k-mer of the table's
contig text answers the smallest byte offset at which it stands in that text; a text position
without a window, a k-mer the table lacks and a k-mer on no contig answer KH_LOC_NONE. Everything
here comes from the text alone: text_cases.window_mask / pack_windows and a Python dict."""
import numpy as np

import text_cases as tc
from cases import RecordDict

LOC_NONE = 0xFFFFFFFFFFFFFFFF
_cache = {}


def position_dict(k, text):
    """packed k-mer bytes -> the smallest position of the k-mer in the text."""
    buf = tc.as_buf(text)
    pos = np.flatnonzero(tc.window_mask(k, buf))
    keys = tc.pack_windows(k, buf, pos)
    d = {}
    for key, p in zip(keys, pos):  # ascending: the first seen is the minimum
        d.setdefault(key.tobytes(), int(p))
    return d


def expected_locate(k, d, keys):
    """uint64 [m]: d's position of each packed key, LOC_NONE when it has none."""
    KP = (k + 3) // 4
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, KP)
    return np.array([d.get(key.tobytes(), LOC_NONE) for key in keys], dtype=np.uint64).reshape(-1)


def expected_locate_text(k, d, text):
    """(pos uint64 [len], windows, located) of a query text against the dict."""
    buf = tc.as_buf(text)
    out = np.full(len(buf), LOC_NONE, np.uint64)
    at = np.flatnonzero(tc.window_mask(k, buf))
    got = expected_locate(k, d, tc.pack_windows(k, buf, at))
    out[at] = got
    return out, len(at), int((got != LOC_NONE).sum())


def expected_lines(text, pos):
    """(line, col) uint64 of positions in a newline-terminated text, LOC_NONE for LOC_NONE."""
    buf = tc.as_buf(text)
    starts = np.concatenate([[0], np.flatnonzero(buf == 10)[:-1] + 1]).astype(np.uint64) if len(buf) else \
        np.zeros(0, np.uint64)
    pos = np.asarray(pos, dtype=np.uint64)
    none = pos == LOC_NONE
    line = np.searchsorted(starts, pos, side="right").astype(np.int64) - 1
    line[none] = 0
    col = pos - (starts[line] if len(starts) else 0)
    line = line.astype(np.uint64)
    line[none] = LOC_NONE
    col[none] = LOC_NONE
    return line, col


def record_of(k, recs, kmer):
    """The input record [R] of a k-mer string."""
    key = tc.pack_windows(k, np.frombuffer(kmer.encode(), np.uint8), [0])
    rec, hit = RecordDict(k, recs).lookup(key)
    assert hit[0]
    return rec[0]


def overlap_case(k):
    """Explicit starts whose walks overlap: the start record of the longest contig of contig_case(k)
    and the record of the k-mer `along` k-mers into it, so the second line is a suffix of the first.
    {"k", "recs", "starts" [2, R], "text" (the expected contig text), "along"}."""
    if ("overlap", k) not in _cache:
        case = tc.contig_case(k)
        c = max(case["contigs"], key=len)
        along = (len(c) - k + 1) // 3
        starts = np.stack([record_of(k, case["recs"], c[:k]), record_of(k, case["recs"], c[along:along + k])])
        _cache[("overlap", k)] = {"k": k, "recs": case["recs"], "starts": np.ascontiguousarray(starts),
                                  "text": (c + "\n" + c[along:] + "\n").encode(), "along": along}
    return _cache[("overlap", k)]


def subset_case(k):
    """Explicit starts for every second contig of contig_case(k): {"k", "recs", "starts", "text" (the
    expected contig text), "off_text" (the other contigs, one per line: k-mers on no contig)}."""
    if ("subset", k) not in _cache:
        case = tc.contig_case(k)
        on, off = case["contigs"][0::2], case["contigs"][1::2]
        starts = np.stack([record_of(k, case["recs"], c[:k]) for c in on])
        _cache[("subset", k)] = {"k": k, "recs": case["recs"], "starts": np.ascontiguousarray(starts),
                                 "text": "".join(c + "\n" for c in on).encode(),
                                 "off_text": "".join(c + "\n" for c in off).encode()}
    return _cache[("subset", k)]
