"""The input builders of cases.py against the oracle (no GPU): the oracle's assembly of
contigs_text(...) is the truth the builder returns, for the values of k and the length mixes the
GPU tests of small inputs use (test_gpu_small.py, test_gpu_dist.py, test_gpu_route.py)."""
import numpy as np
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


# ---- chains of an exact splitter-segment count (test_gpu_segments.py, test_gpu_dist.py) ------------
def check_chain_oracle(k, text, contigs, f):
    """The oracle's assembly of a chain case is the builder's truth, with the facts' counts."""
    recs = ob.parse_text(k, text)
    assert len(recs) == f["n"] and len(contigs) == f["ns"]
    rc, got, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nc == f["ns"] and nl == f["n"] - nc
    assert got == cases.contigs_truth(contigs)
    assert f["nsp"] == cases.count_walk_splitters(k, contigs, f["bits"])


@pytest.mark.parametrize("tail", ["on", "after"])
@pytest.mark.parametrize("first", [1, 4])
@pytest.mark.parametrize("S", [1, 2, 33])
@pytest.mark.parametrize("k", [19, 51])
def test_chain_contig_exact(k, S, first, tail):
    """Exactly S splitters at index >= first; tail "on": the last k-mer is the S-th, "after": two
    k-mers follow it and neither is a splitter."""
    c = cases.chain_contig(k, 2, S, seed=k + S + first, tail=tail, first=first)
    L = len(c) - k + 1
    sp = [i for i in cases.walk_splitter_indices(k, c, 2) if i >= first]
    assert len(sp) == S and len({c[i:i + k] for i in range(L)}) == L
    assert sp[-1] == (L - 1 if tail == "on" else L - 3)
    assert cases.chain_contig(k, 2, S, seed=k + S + first, tail=tail, first=first) == c  # (seeded)


def test_chain_facts_by_hand():
    """chain_facts on splitter positions read off the mirror: counts, the deferred rule (index >=
    2^bits), adjacency and the longest segment."""
    k, bits = 19, 2
    c = cases.chain_contig(k, bits, 40, seed=5, tail="after")
    sp = cases.walk_splitter_indices(k, c, bits)
    L = len(c) - k + 1
    f = cases.chain_facts(k, bits, [c], 0)
    assert (f["ns"], f["n"], f["nsp"], f["S"]) == (1, L, 40, [40]) and not f["deferred"] and f["serial"] == 128
    assert f["S_deferred"] == [sum(i >= 4 for i in sp)]
    assert f["adjacent"] == any(b == a + 1 for a, b in zip(sp, sp[1:])) and not f["adjacent_jumped"]
    assert f["max_seg"] == max(b - a for a, b in zip([0] + sp, sp + [L]))
    g = cases.chain_facts(k, bits, [c], 80)  # 80 one-k-mer contigs: deferred, few splitters per start
    assert (g["ns"], g["n"], g["nsp"]) == (81, L + 80, 40) and g["deferred"] and g["serial"] == 32
    ch = [i for i in sp if i >= 4]
    assert g["adjacent_jumped"] == any(ch[j + 1] == ch[j] + 1 for j in range(31, len(ch) - 1))


@pytest.mark.parametrize("k,regime,S,tail", cases.SEG_SINGLE_PARAMS)
def test_segment_cases_vs_oracle(k, regime, S, tail):
    """Every single-chain case of test_gpu_segments.py: the regime's serial prefix, eager or deferred,
    exactly S splitter segments in that mode, the tail as asked."""
    text, contigs, f = cases.segment_case(k, regime, [S], tail)
    check_chain_oracle(k, text, contigs, dict(f, bits=cases.SEG_BITS))
    serial = cases.SEG_REGIMES[regime]
    assert f["serial"] == serial and f["deferred"] == (regime == "few-deferred")
    assert f["S_deferred" if f["deferred"] else "S"] == [S]
    assert (f["nsp"] >= 16 * f["ns"]) == (regime == "many")
    assert (f["n"] // f["ns"] <= 4) == (regime == "few-deferred")
    assert f["n"] < 3000 and max(f["long_lens"]) < 2000
    long = max(contigs, key=len)
    sp = [i for i in cases.walk_splitter_indices(k, long, cases.SEG_BITS) if i >= (4 if f["deferred"] else 1)]
    assert len(sp) == S and sp[-1] == len(long) - k + 1 - (1 if tail == "on" else 3)


@pytest.mark.parametrize("regime", list(cases.SEG_REGIMES))
def test_segment_cases_adjacent_in_jumped_part(regime):
    """Each regime has cases with two neighbouring splitters past the serial prefix (a one-k-mer
    segment the jump and fill passes rank): the longest target does at both k."""
    S = cases.seg_targets(cases.SEG_REGIMES[regime])[-1]
    for k in (19, 51):
        assert cases.segment_case(k, regime, [S], "after")[2]["adjacent_jumped"]


@pytest.mark.parametrize("k,regime,order", cases.SEG_MULTI_PARAMS)
def test_segment_multi_cases_vs_oracle(k, regime, order):
    serial = cases.SEG_REGIMES[regime]
    text, contigs, f = cases.segment_case(k, regime, cases.seg_multi(serial), "after", order)
    check_chain_oracle(k, text, contigs, dict(f, bits=cases.SEG_BITS))
    assert f["serial"] == serial and f["deferred"] == (regime == "few-deferred")
    assert f["S_deferred" if f["deferred"] else "S"] == cases.seg_multi(serial) and f["n"] < 3000
    long = max(contigs, key=len)
    if order != "shuffled":
        line = text[:k + 4] if order == "first" else text[-(k + 4):]
        assert line == f"{long[:k]} F{long[k]}\n".encode()
    assert cases.segment_case(k, regime, cases.seg_multi(serial))[2]["seed"] == f["seed"]  # the same contigs


@pytest.mark.parametrize("regime,S", cases.SEG_CHUNK_PARAMS)
def test_segment_chunk_cases_vs_oracle(regime, S):
    """KH_SPLIT_BITS=6: a chain one segment past the serial prefix with a segment of more than 256
    k-mers (more than one 256-base chunk)."""
    text, contigs, f = cases.segment_chunk_case(regime, S)
    check_chain_oracle(51, text, contigs, dict(f, bits=cases.SEG_CHUNK_BITS))
    assert f["S"] == [S] == [cases.SEG_REGIMES[regime] + 1] and not f["deferred"]
    assert f["serial"] == cases.SEG_REGIMES[regime] and f["max_seg"] > 256 and f["n"] < 10_000


@pytest.mark.parametrize("S_list", [(S,) for S in cases.RES_TARGETS] + [cases.RES_MULTI])
@pytest.mark.parametrize("k", sorted({k for k, _ in cases.RES_PARAMS}))
def test_sharded_chain_cases_vs_oracle(k, S_list):
    """The sharded chain cases: the eager counts, k-mers / starts <= 4 (the short walk is armed) and
    every long contig past the short walk's 16-base limit with room to spare (it is abandoned)."""
    text, contigs, f = cases.sharded_chain_case(k, S_list)
    check_chain_oracle(k, text, contigs, dict(f, bits=cases.SEG_BITS))
    assert f["S"] == list(S_list) and f["n"] // f["ns"] <= 4 and min(f["long_lens"]) >= 20
    assert f["n"] < 10_000


# ---- the route inputs of test_gpu_route.py --------------------------------------------------------
@pytest.mark.parametrize("n", cases.ROUTE_SIZES)
@pytest.mark.parametrize("k", [12, 13, 19, 22, 32, 51, 60])
def test_route_inputs_vs_oracle(k, n):
    """Exactly n distinct k-mers, the oracle's assembly is the builder's truth (in start-record
    order, after the two lines changed places), starts in the first and in the last mask word, a
    last word that is not full where n says so, a word without starts from one tile on."""
    if k <= 13 and n > 2000:
        n = 2000 - (n % 7)  # (test_gpu_route.py keeps to 2,000 records there)
    text, contigs, seed = cases.route_text(k, n)
    assert len(text) == n * (k + 4)
    recs = ob.parse_text(k, text)
    assert len(recs) == n and len(np.unique(recs[:, :(k + 3) // 4], axis=0)) == n
    cases.RecordDict(k, recs)  # (asserts distinct keys as well)
    rc, got, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nc == len(contigs) and nl == n - nc
    assert got == cases.contigs_truth(contigs)
    assert sorted(len(c) - k + 1 for c in contigs) == sorted(cases.route_lens(n, seed))
    words = cases.start_mask_words(k, text)
    assert len(words) == (n + 63) // 64 and words[0] and words[-1]
    assert sum(bin(w).count("1") for w in words) == nc
    assert words[0] & 1 and words[-1] >> ((n - 1) & 63) == 1  # the first and the last record are starts
    if n >= 2047:
        assert not all(words)
        assert max(len(c) - k + 1 for c in contigs) >= 40 and min(len(c) - k + 1 for c in contigs) <= 4


def test_route_lens_exact():
    for n in cases.ROUTE_SIZES:
        lens = cases.route_lens(n, n)
        assert sum(lens) == n and min(lens) >= 1 and max(lens) <= 300
        assert n < 2 or len(lens) >= 2


def test_chunk_bounds():
    assert cases.chunk_bounds(7169, 2) == [0, 3584, 7169]
    assert cases.chunk_bounds(7169, 5, 2) == [0, 1792, 3584, 3584, 5376, 7169]
    assert cases.chunk_bounds(1, 2, 0) == [0, 0, 1]
    assert cases.chunk_bounds(257, 5) == [0, 48, 96, 144, 192, 257]
    for n in cases.ROUTE_SIZES:
        for calls, empty in ((2, None), (2, 0), (5, None), (5, 2)):
            b = cases.chunk_bounds(n, calls, empty)
            assert b[0] == 0 and b[-1] == n and len(b) == calls + 1
            assert empty is None or b[empty] == b[empty + 1]


def test_record_dict():
    recs = ob.parse_text(19, cases.route_text(19, 257)[0])
    d = cases.RecordDict(19, recs)
    q = np.concatenate([recs[5:8, :5], np.zeros((1, 5), np.uint8) + 0xFF])
    r, f = d.lookup(q)
    assert f.tolist() == [1, 1, 1, 0] and np.array_equal(r[:3], recs[5:8]) and not r[3].any()
    assert d.lookup(recs[:0, :5])[0].shape == (0, 7)
    with pytest.raises(AssertionError):
        cases.RecordDict(19, np.concatenate([recs, recs[:1]]))


@pytest.mark.parametrize("k", [19, 51])
def test_owned_subset_vs_oracle(k):
    """The selection builder of the skewed route input with a stand-in owner function (the real one
    needs a device table): a closed input whose oracle assembly is the kept contigs, nearly all of
    its k-mers with the hot owner."""
    _, contigs = cases.contigs_text(k, cases.short_lens(3000, k), seed=k)

    def owner_of(kmer):  # consecutive k-mers mostly agree, as with a minimizer
        return min(cases.split_hash(kmer[i:i + 8]) for i in range(k - 7)) % 8

    text, kept, hot = cases.owned_subset_text(k, contigs, owner_of, 150, seed=k)
    n = len(text) // (k + 4)
    recs = ob.parse_text(k, text)
    rc, got, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nc == len(kept) and got == cases.contigs_truth(kept)
    assert len(np.unique(recs[:, :(k + 3) // 4], axis=0)) == n
    own = [owner_of(text[i * (k + 4):i * (k + 4) + k].decode()) for i in range(n)]
    assert own.count(hot) >= 0.9 * n and own.count(hot) < n
