"""CPU: the position index's interface (include/kmer_hash_amd.h kh_locate_*, _lib's binding, the
null-table answers, which need no device) and the case builders of test_gpu_locate.py, which must
not be vacuous."""
import ctypes
import re

import numpy as np
import pytest

from cs267_hw3_amd import _lib
import locate_cases as lc
import text_cases as tc

LOCATE = ("kh_locate_reset", "kh_locate_drop", "kh_locate_build", "kh_locate_set_dev", "kh_locate_dev", "kh_locate",
          "kh_locate_text_dev", "kh_locate_text", "kh_locate_lines_dev")


def test_header_declares_and_lib_binds():
    declared = _lib.declared_symbols()
    hdr = open(_lib.HEADER_PATH).read()
    for name in LOCATE:
        assert name in declared, name
        assert name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
    m = re.search(r"#define KH_LOC_NONE (0x[0-9A-Fa-f]+)ull", hdr)
    assert m and int(m.group(1), 16) == lc.LOC_NONE == _lib.LOC_NONE == 2 ** 64 - 1
    assert _lib.lib().kh_abi_version() == 3
    assert re.search(r"#define KH_ABI_VERSION 3\b", hdr)


def test_null_table_is_an_argument_error():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "kh_locate_reset": (None,), "kh_locate_drop": (None,), "kh_locate_build": (None,),
        "kh_locate_set_dev": (None, p, 1, p, p), "kh_locate_dev": (None, p, 1, p), "kh_locate": (None, p, 1, p),
        "kh_locate_text_dev": (None, p, 8, p, p), "kh_locate_text": (None, p, 8, p, p),
        "kh_locate_lines_dev": (None, p, 1, p, p),
    }
    assert set(calls) == set(LOCATE)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == _lib.KH_ERR_ARG, name
        assert b"null table" in L.kh_last_error(), name
    assert list(buf) == [0, 0, 0, 0]


def test_position_dict_is_the_minimum():
    k = 5
    text = b"ACGTACGTAC\nNNACGTA\n"
    d = lc.position_dict(k, text)
    key = lambda s: tc.pack_windows(k, np.frombuffer(s, np.uint8), [0])[0].tobytes()  # noqa: E731
    assert d[key(b"ACGTA")] == 0 and d[key(b"CGTAC")] == 1 and d[key(b"GTACG")] == 2
    assert len(d) == 4  # ACGTA, CGTAC, GTACG, TACGT: the second line adds none
    pos, windows, located = lc.expected_locate_text(k, d, b"ACGTAxTTTTT\n")
    assert windows == 2 and located == 1 and pos[0] == 0 and (pos[1:] == lc.LOC_NONE).all()
    line, col = lc.expected_lines(text, np.array([0, 5, 10, 11, 17, lc.LOC_NONE], np.uint64))
    assert line.tolist() == [0, 0, 0, 1, 1, lc.LOC_NONE] and col.tolist() == [0, 5, 10, 0, 6, lc.LOC_NONE]


@pytest.mark.parametrize("k", [19, 51])
def test_overlap_case_has_a_kmer_at_two_positions(k):
    case = lc.overlap_case(k)
    buf = tc.as_buf(case["text"])
    pos = np.flatnonzero(tc.window_mask(k, buf))
    keys = [x.tobytes() for x in tc.pack_windows(k, buf, pos)]
    d = lc.position_dict(k, case["text"])
    twice = [x for x in set(keys) if keys.count(x) == 2]
    assert case["along"] >= 10 and len(twice) >= 50 and len(d) == len(keys) - len(twice)
    first_line = buf.tolist().index(10)
    assert all(d[x] < first_line for x in twice)  # the minimum is the position in the first line
    assert (case["starts"][0, -2], case["starts"][1, -2]) != (ord("F"), ord("F"))  # the second is no start k-mer


@pytest.mark.parametrize("k", [19, 51])
def test_subset_case_leaves_kmers_off_every_contig(k):
    case = lc.subset_case(k)
    d = lc.position_dict(k, case["text"])
    off = lc.position_dict(k, case["off_text"])
    assert len(off) >= 100 and not set(off) & set(d)
    assert len(d) + len(off) == len(case["recs"])
    assert (case["starts"][:, -2] == ord("F")).all()


@pytest.mark.parametrize("k", [19, 51])
def test_tile_case_crosses_every_tile_edge(k):
    case = tc.tile_case(k)
    for text in tc.tile_texts(case):
        assert tc.crosses_every_tile_edge(k, text)
    assert len(case["contig"]) > 3 * tc.TEXT_TILE
