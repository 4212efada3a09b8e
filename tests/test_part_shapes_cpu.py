"""CPU tests of part_shapes.py (no GPU): the mirror against figures computed from the C++ formulas
and against the product's own host code where that runs without a GPU, and the preconditions of
every case of test_gpu_part_shapes.py, so that none of them is vacuous. What needs a table
(kh_capacity) is asserted by the GPU tests themselves."""
import os
import subprocess

import pytest

import part_shapes as ps
from cs267_hw3_amd import _lib

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")

# n, load -> cap, rbits, RC, variant: part_region_cap / size_table / set_region_bits run on the CPU
FIGURES = [(60_000, 0.5, 120_000, 9, 548, "pf4"), (486_000, 0.5, 972_000, 9, 2146, "pf6"),
           (786_000, 0.5, 1_572_000, 9, 3053, "pf6"), (1_400_000, 0.9, 1_555_556, 9, 4755, "pf12"),
           (1_500_000, 0.9, 1_666_667, 10, 2948, "pf6"), (3_000_000, 0.5, 6_000_000, 11, 2948, "pf6")]


@pytest.mark.parametrize("n,load,cap,rbits,RC,variant", FIGURES)
@pytest.mark.parametrize("k", [19, 31, 51])
def test_mirror_figures(k, n, load, cap, rbits, RC, variant):
    s = ps.shape(k, n, load, n)
    assert (s.cap, s.rbits, s.b2, s.RC, s.variant) == (cap, rbits, rbits - 9, RC, variant)
    assert s.balanced == (load > 0.6)


def test_mirror_more_figures():
    # the large configs at load 0.85 sit at 1526 k-mers per region, just under the 12-word build
    assert ps.build_variant(ps.region_cap(1526 * 512, 9)) == "pf6"
    s = ps.shape(51, 1_300_000, 0.85, 1_300_000)
    assert (s.cap, s.rbits, s.RC, s.variant, s.balanced) == (1_529_412, 9, 4487, "pf12", True)
    assert s.CAP1 == 769  # 317.38 + 10 sqrt(317.38 * 4.75) + 64 = 769.7
    assert ps.shape(51, 800_000, 0.51, 800_000).variant == "pf12"
    assert ps.shape(60, 1_200_000, 0.25, 1_200_000).RC == 1530
    assert [ps.build_variant(rc) for rc in (2048, 2049, 3072, 3073, 6144, 6145)] == \
        ["pf4", "pf6", "pf6", "pf12", "pf12", "plain"]
    assert ps.win1_cap(20_000) == 117  # test_win1_window_spill's "about 117 words"
    assert [ps.default_split_bits(n) for n in (1, 1 << 23, (1 << 24) - 1, 1 << 24, 1 << 40)] == [4, 4, 4, 5, 12]
    assert ps.capacity(0, 0.5) == 2 and ps.capacity(1, 0.9) == 2 and ps.capacity(3, 0.5) == 6


def run_tool(*args):
    exe = os.path.join(CPP, "test_region_bits")
    subprocess.run(["make", "-s", "-C", CPP, exe], check=True)
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, check=True)
    return [[int(x) for x in line.split()] for line in r.stdout.splitlines()]


def test_region_bits_against_the_header():
    """set_region_bits of kh_codec.hpp itself (tests/cpp/test_region_bits.cpp) at both sides of every
    region-count edge. A table gets bit b + 1 once the floor of cap / 2^b passes 3072, so the
    smallest capacity with rbits = r is 3073 << (r - 1): 201,392,128 at r = 17. (3072 << (r - 1)) + 1
    still has r - 1."""
    caps = [2, 3072 << 9, 1 << 40] + [f[2] for f in FIGURES]
    for r in range(10, 18):
        caps += [(3072 << (r - 1)) + 1, ps.min_cap(r) - 1, ps.min_cap(r)]
    got = run_tool(*[f"c{c}" for c in caps])
    assert [c for c, _ in got] == caps
    assert [b for _, b in got] == [ps.region_bits(c) for c in caps]
    assert ps.min_cap(17) == 201_392_128
    for r in range(10, 18):
        assert ps.region_bits(ps.min_cap(r)) == r and ps.region_bits(ps.min_cap(r) - 1) == r - 1
        assert ps.region_bits((3072 << (r - 1)) + 1) == r - 1
    assert ps.region_bits(1 << 40) == 17 and ps.region_bits(2) == 9


def test_key_shape_against_the_header_and_library():
    """make_params / kt_of of kh_codec.hpp, and the library's kh_word_count / kh_record_size, for every
    k a GPU case uses and both sides of the one-word | two-word boundary."""
    ks = sorted({k for k, _ in ps.SWEEP} | set(ps.PAD_KS) | set(ps.BUILD_KS) | {20, 29, 30, 52, 60})
    L = _lib.lib()
    for K, P, R, pad, W, KT in run_tool(*[f"k{k}" for k in ks]):
        s = ps.shape(K, 1000, 0.5, 1000)
        assert (s.P, s.R, s.pad, s.W, s.KT) == (P, R, pad, W, KT)
        assert L.kh_word_count(K) == W and L.kh_record_size(K) == R and L.kh_packed_size(K) == P


def test_searches():
    for r in range(9, 18):
        for load in (0.5, 0.51, 0.85):
            n = ps.n_kmers_for(r, load)
            assert ps.shape(19, n, load, 1).rbits == r and n >= ps.ROOM
            if r > 9 and n > ps.ROOM:
                assert ps.shape(19, n - 1, load, 1).rbits == r - 1
    n = ps.smallest_n(51, 0.5, 9, 2049)
    assert ps.region_cap(n, 9) == 2049 and ps.region_cap(n - 1, 9) == 2048
    with pytest.raises(AssertionError):  # at load 0.5 a table of 512 regions has no room for RC = 3073
        ps.smallest_n(51, 0.5, 9, 3073)


# ---- preconditions of the GPU cases -----------------------------------------------------------------
@pytest.mark.parametrize("k,rbits", ps.SWEEP + [(k, r) for k in ps.PAD_KS for r in ps.PAD_RBITS])
def test_sweep_preconditions(k, rbits):
    """a, d: the table has 2^rbits regions and room for two batches; every record count is small
    against the regions (the 4-word build, most regions empty above rbits 13) and crosses a wave
    or 1, 2, 3 tiles of the records pass by one record."""
    nk = ps.n_kmers_for(rbits, 0.5)
    assert nk >= sum(ps.SECOND_SIZES) and nk >= max(ps.SWEEP_SIZES)
    assert ps.SWEEP_SIZES == (65, 3585, 7169, 10753)
    assert set(ps.SECOND_SIZES) <= set(ps.SWEEP_SIZES)  # each batch of the two-batch cases is a build
    for n in ps.SWEEP_SIZES:
        s = ps.shape(k, nk, 0.5, n)
        assert s.rbits == rbits and s.b2 == rbits - 9 and s.variant == "pf4" and not s.balanced
        assert s.rec_pass == (k in (17, 18, 19, 49, 50, 51)) and s.KT == (k if k in (19, 51) else 0)
    if k in ps.PAD_KS:
        s = ps.shape(k, nk, 0.5, 65)
        assert s.KT == 0 and s.rec_pass and s.pad in (2, 3) and s.P in (5, 13)
    if k == 31:
        s = ps.shape(k, nk, 0.5, 65)
        assert s.KT == 0 and s.W == 2 and not s.rec_pass


def test_sweep_covers_every_region_count():
    assert sorted(r for k, r in ps.SWEEP if k == 19) == list(range(9, 18))
    assert sorted(r for k, r in ps.SWEEP if k == 51) == [10, 11, 13, 17]
    assert sorted(r for k, r in ps.SWEEP if k == 31) == [10, 14]
    assert set(ps.SWEEP_WAYS) <= set(ps.SWEEP) and sorted(k for k, _ in ps.SWEEP_WAYS) == [19, 31, 51]
    assert all(r > 9 for _, r in ps.SWEEP_WAYS)
    assert set(ps.SWEEP_SECOND) <= set(ps.SWEEP) and {r for _, r in ps.SWEEP_SECOND} == {11, 14}
    assert {ps.shape(k, 1, 0.5, 1).W for k, _ in ps.SWEEP_SECOND} == {1, 2}
    assert set(ps.PAD_RBITS) == {9, 11}


@pytest.mark.parametrize("rbits", ps.SPILL_RBITS)
def test_spill_preconditions(rbits):
    """b: the hot batch goes into a non-empty table (no sampling before pass 1), pass 2 really sorts,
    and one bucket's 8 pass-1 windows and one region window hold a fraction of the hot set."""
    nk = ps.n_kmers_for(rbits, 0.5)
    s = ps.shape(ps.SPILL_K, nk, 0.5, ps.SPILL_HOT)
    assert s.rbits == rbits and s.b2 > 0 and ps.SPILL_FIRST > 0
    assert nk >= ps.SPILL_FIRST + ps.SPILL_HOT
    assert ps.S1 * s.CAP1 < ps.SPILL_HOT // 4 and s.RC < ps.SPILL_HOT // 4


@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("k", ps.BUILD_KS)
@pytest.mark.parametrize("name", sorted(ps.BUILD_CASES))
def test_build_preconditions(name, k, fresh):
    """c: the big batch's window is exactly the RC the case names, one k-mer fewer gives RC - 1, the
    table keeps its region count with the first batch added, and the variant is the one the case
    is there for."""
    load, rbits, RC, variant = ps.BUILD_CASES[name]
    nk, n, s = ps.build_case(name, k, fresh)
    assert nk == n + (0 if fresh else ps.BUILD_FIRST)
    assert (s.rbits, s.RC, s.variant, s.balanced) == (rbits, RC, variant, load > 0.6)
    assert ps.region_cap(n - 1, rbits) == RC - 1
    assert n >= 400_000  # more than 800 k-mers per region: no window of the build is close to empty
    if not fresh:  # the first batch is a build of its own, the smallest variant
        assert ps.shape(k, nk, load, ps.BUILD_FIRST).variant == "pf4"
    assert s.sorted_fresh == (k > 29)


def test_build_cases_cover_the_edges():
    by = {name: c for name, c in ps.BUILD_CASES.items()}
    assert (by["rc2048"][2], by["rc2049"][2]) == (4 * 512, 4 * 512 + 1)
    assert (by["rc3072"][2], by["rc3073"][2]) == (6 * 512, 6 * 512 + 1)
    assert {c[3] for c in by.values()} == {"pf4", "pf6", "pf12"}
    assert by["bal4487"][0] > 0.6 and by["bal4487"][3] == "pf12"
    assert by["r10"][1] == 10 and by["r10"][3] == "pf6"
