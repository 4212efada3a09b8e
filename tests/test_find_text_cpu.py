"""CPU: the find-over-text test helper against a naive loop, non-vacuity of every case the GPU file
uses (so a case can never pass empty), and the new C-ABI symbols (no kernel is launched)."""
import ctypes

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import text_cases as tc
from cases import RecordDict


def naive_find_text(k, recs, text):
    """One Python step per window: slice, check the alphabet, pack, look up."""
    KP = (k + 3) // 4
    table = {bytes(r[:KP]): bytes(r[KP:KP + 2]) for r in recs}
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    out = np.full((len(text), 2), 0xFF, np.uint8)
    windows = found = 0
    for i in range(len(text) - k + 1):
        w = text[i:i + k]
        if any(b not in code for b in w):
            continue
        windows += 1
        key = bytearray(KP)
        for j, b in enumerate(w):
            key[j // 4] |= code[b] << (6 - 2 * (j % 4))
        e = table.get(bytes(key))
        found += e is not None
        out[i] = tuple(e) if e else (0, 0)
    return out, windows, found


@pytest.mark.parametrize("k", [19, 51])
def test_helper_agrees_with_naive_loop(k):
    case = tc.contig_case(k)
    longest = max(case["contigs"], key=len).encode()
    text = tc.dirty_text(k, case["contigs"])[:150] + tc.mutated_text(longest)[:150]
    assert len(text) == 300
    want = naive_find_text(k, case["recs"], text)
    got = tc.expected_find_text(k, case["recs"], text)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert tc.classes(got[0]) == {"found", "absent", "none"}


def test_records_from_lines_is_the_host_codec():
    case = tc.contig_case(51)
    assert np.array_equal(case["recs"], kh.pack_text(51, case["lines"]))


@pytest.mark.parametrize("k", tc.K_COVER)
def test_contig_case_not_vacuous(k):
    case = tc.contig_case(k)
    lens = sorted(len(c) - k + 1 for c in case["contigs"])
    assert len(lens) == 40 and lens[0] == 1 and lens[-1] == 300
    ext, windows, found = tc.expected_find_text(k, case["recs"], case["truth"])
    assert windows == found == len(case["recs"]) and tc.classes(ext) == {"found", "none"}
    assert np.array_equal(ext, tc.neighbour_answers(k, case["truth"]))
    # mutated: at least 100 absent windows, and still some found
    mext, mw, mf = tc.expected_find_text(k, case["recs"], tc.mutated_text(case["truth"]))
    assert mw == windows and mw - mf >= 100 and tc.classes(mext) == {"found", "absent", "none"}
    assert int((mext == 0).all(axis=1).sum()) == mw - mf


@pytest.mark.parametrize("k", tc.K_COVER)
def test_dirty_case_not_vacuous(k):
    case = tc.contig_case(k)
    text = tc.dirty_text(k, case["contigs"])
    for b in (b"N", b"F", b"\r\n", b" ", b"\x00", b"\xff", b"\n\n", b">"):
        assert b in text
    assert any(c in text for c in (b"a", b"c", b"g", b"t")) and not text.endswith(b"\n")
    lines = text.split(b"\n")
    assert {k - 1, k, k + 1} <= {len(ln.rstrip(b"\r")) for ln in lines} and len(lines[-1]) == k - 2
    ext, windows, found = tc.expected_find_text(k, case["recs"], text)
    assert tc.classes(ext) == {"found", "absent", "none"} and 0 < found < windows
    # the header's letters form present windows
    assert (ext[:lines[0].index(b"len=") + 4 + 6] != 0xFF).any()
    # a bad byte at the first / last base of an otherwise present window kills exactly that window
    at = text.index(b"\nn") + 1
    assert (ext[at] == 0xFF).all() and (ext[at + 1] != 0xFF).all() and (ext[at + 1] != 0).all()
    at = text.index(b"x", text.index(b"\nn") + 2) - (k - 1)
    assert (ext[at] == 0xFF).all() and (ext[at + k] != 0xFF).all()


@pytest.mark.parametrize("k", [19, 51])
def test_length_cases_not_vacuous(k):
    case = tc.contig_case(k)
    long = max(case["contigs"], key=len)
    texts = tc.length_texts(k, long)
    assert [len(t) for t in texts] == [0, 1, k - 1, k, k + 1]
    res = [tc.expected_find_text(k, case["recs"], t) for t in texts]
    assert [r[1:] for r in res] == [(0, 0), (0, 0), (0, 0), (1, 1), (2, 2)]
    assert tc.classes(res[1][0]) == tc.classes(res[2][0]) == {"none"}
    assert tc.classes(res[3][0]) == tc.classes(res[4][0]) == {"found", "none"}


@pytest.mark.parametrize("k", [19, 51])
def test_tile_case_not_vacuous(k):
    assert tc.TEXT_TILE == _lib.TEXT_TILE
    case = tc.tile_case(k)
    assert len(case["contig"]) >= 3 * tc.TEXT_TILE and (tc.TEXT_TILE > 4096 or len(case["contig"]) == 20000)
    for pre, text in enumerate(tc.tile_texts(case)):
        assert text[:pre] == b"\n" * pre and b"\n" not in text[pre:]
        assert tc.crosses_every_tile_edge(k, text)
        ext, windows, found = tc.expected_find_text(k, case["recs"], text)
        assert windows == found == len(case["recs"])
        assert tc.classes(ext) == {"found", "none"}
    # the check itself: a text whose bad bytes sit on the tile edges does not pass it
    buf = np.frombuffer(text, np.uint8).copy()
    buf[tc.TEXT_TILE] = ord("N")
    assert not tc.crosses_every_tile_edge(k, buf)


def test_hot_case_not_vacuous():
    case = tc.hot_case(kh.SyntheticKmers)
    ext, windows, found = tc.expected_find_text(51, RecordDict(51, case["recs"]), case["truth"])
    assert windows == found == 200_000 and tc.classes(ext) == {"found", "none"}


def test_shard_texts_not_vacuous():
    k = 51
    case = tc.contig_case(k)
    dirty, mutated, empty, short = tc.shard_texts(k)
    assert empty == b"" and 0 < len(short) < k
    assert tc.classes(tc.expected_find_text(k, case["recs"], dirty)[0]) == {"found", "absent", "none"}
    assert tc.classes(tc.expected_find_text(k, case["recs"], mutated)[0]) == {"found", "absent", "none"}
    assert tc.classes(tc.expected_find_text(k, case["recs"], short)[0]) == {"none"}


def test_new_symbols_exist_and_reject_a_null_table():
    L = _lib.lib()
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define KH_TEXT_NONE 0xFF" in hdr and f"#define KH_TEXT_TILE {_lib.TEXT_TILE}" in hdr
    assert _lib.TEXT_NONE == 0xFF
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.kh_find_text_dev(None, p, 8, p, p) == _lib.KH_ERR_ARG
    assert L.kh_find_text(None, p, 8, p, p) == _lib.KH_ERR_ARG
    assert L.kh_text_keys_dev(None, p, 8, p, p, p) == _lib.KH_ERR_ARG
    assert L.kh_abi_version() == 3
    for name in ("find_text", "find_text_dev"):
        assert callable(getattr(kh.KmerHashTable, name))
