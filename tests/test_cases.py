"""The input builders of cases.py against the oracle (no GPU): the oracle's assembly of
contigs_text(...) is the truth the builder returns, for the values of k and the length mixes the
GPU tests of small inputs use (test_gpu_small.py, test_gpu_dist.py)."""
import pytest

import cases
import oracle_bind as ob

KS = [12, 19, 31, 52, 60]


def check_oracle(k, lens, seed, order="shuffled"):
    text, contigs = cases.contigs_text(k, lens, seed, order)
    n = sum(lens)
    assert len(text) == n * (k + 4) and len(contigs) == len(lens)
    assert sorted(len(c) - k + 1 for c in contigs) == sorted(lens)
    recs = ob.parse_text(k, text)
    rc, got, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nc == len(lens) and nl == n - nc
    assert got == cases.contigs_truth(contigs)
    return text, contigs


@pytest.mark.parametrize("order", ["shuffled", "first", "last"])
@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("k", KS)
def test_deferred_shapes_vs_oracle(k, shape, order):
    text, contigs, f = cases.deferred_case(k, shape, order)
    recs = ob.parse_text(k, text)
    rc, got, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and got == cases.contigs_truth(contigs)
    assert nc == f["ns"] and nl == f["n"] - nc
    # the longest contig's start record is where `order` says
    long = max(contigs, key=len)
    if order != "shuffled":
        line = text[:k + 4] if order == "first" else text[-(k + 4):]
        assert line == f"{long[:k]} F{long[k]}\n".encode()
        assert (contigs[0] if order == "first" else contigs[-1]) == long


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("k", [19, 31, 51])
def test_deferred_preconditions(k, shape):
    """The committed seed list gives the one-reservation shapes their preconditions (deferred_ok)
    at every k the GPU test runs; the first seed does at each."""
    _, contigs, f = cases.deferred_case(k, shape)
    assert cases.deferred_ok(shape, f)
    assert f["ns"] == (31 if shape == "A" else 91)
    assert f["seed"] == (100 if shape == "A" else 200) + k
    assert f["n_all"] == f["ns"] + cases.count_walk_splitters(k, contigs, 4)


@pytest.mark.parametrize("extra", [0, 300])
@pytest.mark.parametrize("ns", [1, 65, 513])
@pytest.mark.parametrize("k", KS)
def test_short_mixes_vs_oracle(k, ns, extra):
    check_oracle(k, cases.short_lens(ns, 7 * k + ns, extra), seed=k + ns + extra)


@pytest.mark.parametrize("k", KS)
def test_equal_contigs_vs_oracle(k):
    check_oracle(k, [40] * 3, seed=k)


@pytest.mark.parametrize("long_tail", [False, True])
@pytest.mark.parametrize("T", [1023, 2049])
@pytest.mark.parametrize("k", KS)
def test_text_size_lens_vs_oracle(k, T, long_tail):
    lens = cases.lens_for_text_bytes(k, T, seed=k + T, long_tail=long_tail)
    assert sum(L + k for L in lens) == T
    assert lens[-1] >= 300 if long_tail else all(L <= k + 4 for L in lens)
    _, contigs = check_oracle(k, lens, seed=k + T, order="last" if long_tail else "shuffled")
    assert len(cases.contigs_truth(contigs)) == T
    if long_tail:  # the text ends with the contig of >= 300 k-mers
        assert len(contigs[-1]) - k + 1 == lens[-1] and all(len(c) - k + 1 <= 3 for c in contigs[:-1])


def test_text_size_unreachable_and_smallest():
    assert cases.lens_for_text_bytes(31, 32, seed=1) == [1]
    assert cases.lens_for_text_bytes(31, 32, seed=1, long_tail=True) is None


def test_small_k_redraws_repeated_kmers():
    """k = 6: 2,000 k-mers of 4,096 possible; every k-mer of the text is distinct."""
    text, contigs = cases.contigs_text(6, [20] * 100, seed=3)
    kmers = [line[:6] for line in text.splitlines()]
    assert len(kmers) == len(set(kmers)) == 2000


def test_split_hash_mirror():
    """split_hash (kh_codec.hpp) on hand-computed values: the low 62 bits of the 2-bit packing,
    folded to 32 bits and multiplied by 0x9E3779B1."""
    assert cases.split_hash("A" * 19) == 0
    assert cases.split_hash("A" * 18 + "C") == 0x9E3779B1
    assert cases.split_hash("C" + "A" * 31) == 0           # the 32nd base from the end: bit 62, not in lo
    assert cases.split_hash("C" + "A" * 16) == 0x9E3779B1  # bit 32 folds onto bit 0
    c = "ACGT" * 5
    assert cases.walk_splitter_indices(4, c, 0) == []      # split_test: 0 bits = off
    assert cases.walk_splitter_indices(4, "AAAAA", 4) == [1] and cases.count_walk_splitters(4, ["AAAAA", c], 0) == 0
