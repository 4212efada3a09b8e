"""CPU: the interface of the calls over both strands (include/kmer_hash_amd.h kh_locate_text_rc*,
kh_seed_strand_*; _lib's binding; the null-table answers, which need no device), reverse_complement,
the model of strand_cases.py on hand-written arrays, and the case builders of test_gpu_strand.py,
which must not be vacuous."""
import ctypes
import re

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import locate_cases as lc
import seed_cases as sc
import strand_cases as st
import text_cases as tc

STRAND = ("kh_locate_text_rc_dev", "kh_locate_text_rc", "kh_seed_strand_runs_dev", "kh_seed_strand_text_dev",
          "kh_seed_strand_text")
NONE = st.LOC_NONE


# ---- the interface -------------------------------------------------------------------------------
def test_header_declares_and_lib_binds():
    declared = _lib.declared_symbols()
    hdr = open(_lib.HEADER_PATH).read()
    for name in STRAND:
        assert name in declared, name
        assert name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
    m = re.search(r"#define KH_SEED_STRAND_WORDS (\d+)\b", hdr)
    assert m and int(m.group(1)) == st.STRAND_WORDS == _lib.SEED_STRAND_WORDS == 6
    assert _lib.lib().kh_abi_version() == 3  # entry points and one define only


def test_null_table_is_an_argument_error():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "kh_locate_text_rc_dev": (None, p, 8, p, p), "kh_locate_text_rc": (None, p, 8, p, p),
        "kh_seed_strand_runs_dev": (None, p, p, 8, p, 1, p), "kh_seed_strand_text_dev": (None, p, 8, p, 1, p, p),
        "kh_seed_strand_text": (None, p, 8, p, 1, p),
    }
    assert set(calls) == set(STRAND)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == _lib.KH_ERR_ARG, name
        assert b"null table" in L.kh_last_error(), name
    assert list(buf) == [0] * 8


def test_strands_argument():
    """Anything but "+" and "both" is refused before the table is touched (a closed handle would fail
    otherwise)."""
    import inspect
    from cs267_hw3_amd.dist import DistributedKmerHashMap, GpuShard
    t = object.__new__(kh.KmerHashTable)
    for bad in ("x", "-", "", None, "Both"):
        with pytest.raises(ValueError):
            kh.KmerHashTable.seed_reads(t, b"ACGT\n", strands=bad)
        with pytest.raises(ValueError):
            DistributedKmerHashMap.seed_reads(object.__new__(DistributedKmerHashMap), b"ACGT\n", strands=bad)
    assert inspect.signature(kh.KmerHashTable.seed_reads).parameters["strands"].default == "+"
    assert inspect.signature(DistributedKmerHashMap.seed_reads).parameters["strands"].default == "+"
    for cls, names in ((kh.KmerHashTable, ("locate_text_rc_dev", "seed_strand_text_dev", "seed_strand_runs_dev")),
                       (GpuShard, ("seed_strand_runs", "seed_strand_text"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    for cls in (kh.KmerHashTable, GpuShard, DistributedKmerHashMap):
        assert inspect.signature(cls.locate_text).parameters["rc"].default is False


@pytest.mark.parametrize("text,want", [
    (b"", b""),
    (b"A", b"T"),
    (b"ACGT", b"ACGT"),
    (b"AACG", b"CGTT"),
    (b"AAC\nGT\n", b"\nAC\nGTT"),               # lines stay lines
    (b"acgtNn-\r\x00\xffAC", b"GT\xff\x00\r-nNtgca"),  # everything but A C G T is kept
])
def test_reverse_complement(text, want):
    assert st.revcomp(text) == want
    for form in (text, np.frombuffer(text, np.uint8)):
        got = kh.reverse_complement(form)
        assert isinstance(got, bytes) and got == want
    assert kh.reverse_complement(kh.reverse_complement(text)) == text


def test_reverse_complement_against_the_model_on_dirty_text():
    k = 31
    text = tc.dirty_text(k, tc.contig_case(k)["contigs"])
    assert kh.reverse_complement(text) == st.revcomp(text) != text
    rng = np.random.default_rng(5)
    blob = rng.integers(0, 256, 4096).astype(np.uint8)
    assert kh.reverse_complement(blob) == st.revcomp(blob)


# ---- the model on hand-written arrays -------------------------------------------------------------
def seeds(k, v, w, off):
    return st.expected_strand_seeds(k, np.array(v, np.uint64), np.array(w, np.uint64), off).tolist()


N = NONE


def test_model_ascending_and_descending_runs():
    k = 3
    v = [10, 11, 12, N, N, N, N, N, N]  # 9 bytes: 7 counted windows
    w = [N, N, N, 53, 52, 51, 50, N, N]
    assert seeds(k, v, w, [0, 9]) == [[3, 50, 4, 1, 3, 4]]           # the longer one; its value is its smallest
    assert seeds(k, v, [N] * 9, [0, 9]) == [[0, 10, 3, 0, 3, 0]]
    assert seeds(k, [N] * 9, w, [0, 9]) == [[3, 50, 4, 1, 0, 4]]
    assert seeds(k, [N] * 9, [N] * 9, [0, 9]) == [list(st.EMPTY)]
    # an ascending run in w and a descending one in v are runs of one
    assert seeds(2, [9, 8, 7, 7, 7], [1, 2, 3, 3, 3], [0, 6]) == [[0, 9, 1, 0, 4, 4]]


def test_model_zero_is_never_continued_and_none_neighbours():
    k = 2
    assert seeds(k, [N] * 4, [2, 1, 0, N], [0, 5]) == [[0, 0, 3, 1, 0, 3]]       # down to 0
    # (k = 2: the last byte holds no counted window)
    assert seeds(k, [N] * 5, [1, 0, N, N - 1, N], [0, 6]) == [[0, 0, 2, 1, 0, 3]]  # 0 - 1 is NONE: no continuation
    assert seeds(k, [N] * 4, [N, N - 1, N - 2, N], [0, 5]) == [[1, N - 2, 2, 1, 0, 2]]  # NONE is not ...FFFE + 1
    assert seeds(k, [N] * 4, [N - 1, N, N - 1, N], [0, 5]) == [[0, N - 1, 1, 1, 0, 2]]


def test_model_tie_between_strands_goes_forward():
    k = 3
    v = [5, 6, 7, N, N, N, N, N]
    w = [N, N, N, 9, 8, 7, N, N]
    assert seeds(k, v, w, [0, 8]) == [[0, 5, 3, 0, 3, 3]]
    # the reverse run first in the read, the forward one after it: still forward
    v2 = [N, N, N, 5, 6, 7, N, N]
    w2 = [9, 8, 7, N, N, N, N, N]
    assert seeds(k, v2, w2, [0, 8]) == [[3, 5, 3, 0, 3, 3]]
    w2[3] = 6  # the reverse run one longer
    assert seeds(k, v2, w2, [0, 8]) == [[0, 6, 4, 1, 3, 4]]


def test_model_tie_within_a_strand_goes_to_the_first():
    k = 3
    w = [30, 29, 28, N, 70, 69, 68, N, N]
    assert seeds(k, [N] * 9, w, [0, 9]) == [[0, 28, 3, 1, 0, 6]]
    w[3] = 27
    assert seeds(k, [N] * 9, w, [0, 9]) == [[0, 27, 4, 1, 0, 7]]
    w[:4] = [30, 29, N, N]
    assert seeds(k, [N] * 9, w, [0, 9]) == [[4, 68, 3, 1, 0, 5]]


def test_model_reads_and_counted_windows():
    k = 3
    w = list(range(109, 99, -1))  # ten located windows in a row, descending
    v = [N] * 10
    assert seeds(k, v, w, [0, 10]) == [[0, 102, 8, 1, 0, 8]]
    assert seeds(k, v, w, [0, 5, 10]) == [[0, 107, 3, 1, 0, 3], [0, 102, 3, 1, 0, 3]]
    assert seeds(k, v, w, [0, 2, 2, 10]) == [list(st.EMPTY), list(st.EMPTY), [0, 102, 6, 1, 0, 6]]
    assert seeds(k, v, w, [0, 50, 90]) == [[0, 102, 8, 1, 0, 8], list(st.EMPTY)]
    assert st.expected_strand_seeds(k, v, w, [0]).shape == (0, 6)
    # with w all NONE the answer is seed_cases' with strand 0 and located_rc 0
    pos = np.array([10, 11, 12, N, 50, 51, 52, N, N], np.uint64)
    old = sc.expected_seeds(k, pos, [0, 4, 9])
    new = st.expected_strand_seeds(k, pos, np.full(9, N, np.uint64), [0, 4, 9])
    assert np.array_equal(new[:, :3], old[:, :3]) and np.array_equal(new[:, 4], old[:, 3])
    assert not new[:, 3].any() and not new[:, 5].any()
    assert np.array_equal(st.repacked(new), old)


def test_model_made_up_arrays_hold_what_they_claim():
    k = 19
    v, w = st.made_up_arrays()
    assert len(v) == len(w)
    got = st.expected_strand_seeds(k, v, w, [0, len(v)])
    assert got[0, 2] == 300 and got[0, 3] == 1
    lens = {r[2] for r in st.rev_runs_of(1, w, 0, len(w))}
    assert {1, 2, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193, 300} <= lens
    assert (w >= np.uint64(1 << 48)).any() and (w == 0).any() and (w == NONE - 1).any()


# ---- the mirror identity -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [19, 32, 51])
def test_mirror_identity(k):
    case = tc.contig_case(k)
    d = lc.position_dict(k, case["truth"])
    hits = 0
    for text in (tc.dirty_text(k, case["contigs"]), st.revcomp(tc.dirty_text(k, case["contigs"])),
                 st.revcomp(case["truth"])[:3000], b"", b"ACG"):
        w, windows, located = st.expected_locate_text_rc(k, d, text)
        u, uw, ul = lc.expected_locate_text(k, d, st.revcomp(text))
        assert np.array_equal(w, st.mirrored(k, u)) and (windows, located) == (uw, ul)
        n = len(text)
        for i in range(0, max(n - k + 1, 0)):
            assert w[i] == u[n - k - i]
        hits += located
    assert hits > 1000


# ---- the case builders ---------------------------------------------------------------------------
def dict_of(k):
    return lc.position_dict(k, tc.contig_case(k)["truth"])


@pytest.mark.parametrize("k", [19, 31, 32, 51, 60])
def test_rc_length_reads_have_the_claimed_reverse_seed(k):
    d = dict_of(k)
    for read, at, w in st.rc_length_reads(k):
        assert len(read) == w + k - 1
        got = st.expected_for(k, d, read, [0, len(read)])
        if w == 0:
            assert got.tolist() == [list(st.EMPTY)]
            continue
        assert got[0, :4].tolist() == [0, at, w, 1] and int(got[0, 5]) == w and int(got[0, 4]) <= 2, (w, got)


@pytest.mark.parametrize("k", [19, 51])
def test_rc_carry_reads_have_the_intended_runs(k):
    d = dict_of(k)
    ends, begins = [], []
    for j, (read, (a, b)) in enumerate(st.rc_carry_reads(k)):
        w = st.expected_locate_text_rc(k, d, read)[0]
        runs = st.rev_runs_of(k, w, 0, len(read))
        assert [x[2] for x in runs] == [x for x in (a, b) if x], (j, a, b, runs)
        (ends if j < 3 else begins).append(runs[0][2] - 1 if j < 3 else runs[-1][0])
        got = st.expected_for(k, d, read, [0, len(read)])
        assert int(got[0, 3]) == 1 and int(got[0, 2]) == max(a, b)
    assert ends == [62, 63, 64] and begins == [62, 63, 64]


@pytest.mark.parametrize("k", [19, 51])
def test_choice_reads_have_one_run_on_each_strand(k):
    d = dict_of(k)
    cases = st.choice_reads(k)
    assert [(ab, o) for _, ab, o in cases] == [(ab, o) for ab in st.CHOICES for o in ("fr", "rf")]
    for read, (a, b), order in cases:
        got = st.expected_for(k, d, read, [0, len(read)])[0]
        assert int(got[2]) == max(a, b) and int(got[3]) == (1 if b > a else 0), (a, b, order, got)
        assert int(got[4]) == a and int(got[5]) == b
        assert int(got[0]) == (0 if (order == "fr") == (a >= b) else (a if order == "fr" else b) + k - 1)


@pytest.mark.parametrize("k", [19, 51])
def test_both_strands_case_shares_no_kmer(k):
    case = st.both_strands_case(k)
    lines = [c.encode() for c in case["contigs"]]
    assert len(lines) == 8 and st.shares_no_kmer(k, lines)
    assert sorted(lines) == sorted(st.revcomp(x) for x in lines)  # the set is closed under revcomp
    assert not st.shares_no_kmer(k, lines + [lines[0][5:5 + k]])
    d = lc.position_dict(k, case["truth"])
    read = lines[0][3:3 + k + 70]
    got = st.expected_for(k, d, read, [0, len(read)])[0]
    assert got[2:].tolist() == [71, 0, 71, 71]
