"""CPU: the seed calls' interface (include/kmer_hash_amd.h kh_seed_*, _lib's binding, the null-table
answers, which need no device), read_offsets, the model of seed_cases.py on hand-written position
arrays, and the case builders of test_gpu_seed.py, which must not be vacuous."""
import ctypes
import re

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import locate_cases as lc
import seed_cases as sc
import text_cases as tc

SEED = ("kh_seed_runs_dev", "kh_seed_text_dev", "kh_seed_text", "kh_seed_coverage_dev")
NONE = sc.LOC_NONE


def test_header_declares_and_lib_binds():
    declared = _lib.declared_symbols()
    hdr = open(_lib.HEADER_PATH).read()
    for name in SEED:
        assert name in declared, name
        assert name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
    m = re.search(r"#define KH_SEED_WORDS (\d+)\b", hdr)
    assert m and int(m.group(1)) == sc.SEED_WORDS == _lib.SEED_WORDS == 4
    assert _lib.lib().kh_abi_version() == 3


def test_null_table_is_an_argument_error():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "kh_seed_runs_dev": (None, p, 8, p, 1, p), "kh_seed_text_dev": (None, p, 8, p, 1, p, p),
        "kh_seed_text": (None, p, 8, p, 1, p), "kh_seed_coverage_dev": (None, p, 1, p, p),
    }
    assert set(calls) == set(SEED)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == _lib.KH_ERR_ARG, name
        assert b"null table" in L.kh_last_error(), name
    assert list(buf) == [0] * 8


@pytest.mark.parametrize("text,want", [
    (b"", [0]),
    (b"ACGT", [0, 4]),                           # one unterminated line
    (b"ACGT\n", [0, 5]),
    (b"AC\n\n\nGT\n", [0, 3, 4, 5, 8]),          # blank lines are (empty) reads
    (b"\n", [0, 1]),
    (b"AC\r\nGT\r\nA", [0, 4, 8, 9]),            # '\r' stays in its read; the tail is a last read
])
def test_read_offsets(text, want):
    for form in (text, np.frombuffer(text, np.uint8)):
        off = kh.read_offsets(form)
        assert off.dtype == np.uint64 and off.tolist() == want


# ---- the model on hand-written position arrays ---------------------------------------------------
def seeds(k, pos, off):
    return sc.expected_seeds(k, np.array(pos, np.uint64), off).tolist()


def test_model_tie_goes_to_the_first_run():
    k = 3
    pos = [10, 11, 12, NONE, 50, 51, 52, NONE, NONE]  # 9 bytes: 7 counted windows
    assert seeds(k, pos, [0, 9]) == [[0, 10, 3, 6]]
    pos[3] = 13
    assert seeds(k, pos, [0, 9]) == [[0, 10, 4, 7]]
    pos[:4] = [10, 11, NONE, NONE]
    assert seeds(k, pos, [0, 9]) == [[4, 50, 3, 5]]  # the longer one, wherever it lies


def test_model_none_never_continues():
    k = 2
    pos = [2 ** 64 - 2, NONE, 0, 1, 7]
    assert seeds(k, pos, [0, 6]) == [[2, 0, 2, 3]]  # ...FFFE + 1 is NONE: no continuation; NONE + 1 = 0 neither
    assert seeds(k, [NONE] * 5, [0, 6]) == [list(sc.EMPTY)]
    assert seeds(k, [2 ** 64 - 3, 2 ** 64 - 2, NONE], [0, 4]) == [[0, 2 ** 64 - 3, 2, 2]]


def test_model_descending_and_equal_values_are_runs_of_one():
    assert seeds(2, [9, 8, 7, 7, 7], [0, 6]) == [[0, 9, 1, 4]]


def test_model_window_past_the_read_end_is_not_counted():
    k = 3
    pos = list(range(100, 110))  # ten located windows in a row
    assert seeds(k, pos, [0, 10]) == [[0, 100, 8, 8]]
    # cut in two with no separator: each read answers only the windows that end inside it
    assert seeds(k, pos, [0, 5, 10]) == [[0, 100, 3, 3], [0, 105, 3, 3]]
    assert seeds(k, pos, [0, 2, 2, 10]) == [list(sc.EMPTY), list(sc.EMPTY), [0, 102, 6, 6]]
    assert seeds(k, pos, [4, 8]) == [[0, 104, 2, 2]]                  # bytes outside every read are ignored
    assert seeds(k, pos, [0, 50, 90]) == [[0, 100, 8, 8], list(sc.EMPTY)]  # offsets past the text clamp
    assert sc.expected_seeds(k, pos, [0]).shape == (0, 4)


def test_model_coverage():
    text = b"ACGTACGT\nAC\nACGTA\n"
    s = np.array([[0, 0, 3, 3], [1, 9, 1, 1], sc.EMPTY, [0, 12, 2, 2], [0, 18, 1, 1], [0, 3, 0, 0]], np.uint64)
    reads, bases = sc.expected_coverage(3, text, s)
    assert reads.tolist() == [1, 1, 1] and bases.tolist() == [5, 3, 4]  # 18 is past the text, run 0 is no seed
    again = sc.expected_coverage(3, text, s, reads, bases)
    assert again[0].tolist() == [2, 2, 2] and again[1].tolist() == [10, 6, 8]


# ---- the case builders ---------------------------------------------------------------------------
def model_runs(k, read):
    d = lc.position_dict(k, tc.contig_case(k)["truth"])
    pos = lc.expected_locate_text(k, d, read)[0]
    return sc.runs_of(k, pos, 0, len(read))


@pytest.mark.parametrize("k", [19, 51])
def test_two_run_reads_have_the_intended_runs(k):
    for name, cases in (("carry", sc.carry_reads(k)), ("tie", sc.tie_reads(k)), ("chimeric", sc.chimeric_reads(k))):
        for read, (a, b) in cases:
            runs = model_runs(k, read)
            assert [x[2] for x in runs] == [x for x in (a, b) if x], (name, a, b, runs)
    ends = [model_runs(k, read)[0][2] - 1 for read, _ in sc.carry_reads(k)[:3]]
    begins = [model_runs(k, read)[-1][0] for read, _ in sc.carry_reads(k)[3:]]
    assert ends == [62, 63, 64] and begins == [62, 63, 64]
    a, b = model_runs(k, sc.tie_reads(k)[0][0])
    assert a[2] == b[2] and a[0] < b[0]


@pytest.mark.parametrize("k", [19, 51, 60])
def test_length_reads_have_the_chunk_edge_window_counts(k):
    d = lc.position_dict(k, tc.contig_case(k)["truth"])
    for (read, at), w in zip(sc.length_reads(k), sc.WINDOW_COUNTS):
        assert len(read) == w + k - 1
        want = [[0, at, w, w]] if w else [list(sc.EMPTY)]
        assert sc.expected_for(k, d, read, [0, len(read)]).tolist() == want


def test_long_read_has_four_runs():
    k = 51
    read, lens = sc.long_read(k)
    case = tc.tile_case(k)
    d = lc.position_dict(k, case["contig"].encode() + b"\n")
    pos = lc.expected_locate_text(k, d, read)[0]
    assert tuple(x[2] for x in sc.runs_of(k, pos, 0, len(read))) == lens and len(read) == 20000
    assert max(lens) > 64 * 100 and len(set(lens)) == 4
