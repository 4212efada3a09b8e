"""GPU parity on small inputs and at the values of k where the key / slot layout changes: a few
contigs to a few thousand k-mers, where one work-queue reservation of k_walk_q holds the last
start walker and every splitter walker, where a wave or a reservation is just (not) full, and
where the text ends just before / at / after a line writer's block. Every case is compared byte
for byte with the oracle (oracle_bind.assemble); the builders are checked against the oracle on the
CPU in test_cases.py."""
import functools

import numpy as np
import pytest

import cs267_hw3_amd as kh
import oracle_bind as ob
import cases
from walk_checks import first_attempt

pytestmark = pytest.mark.gpu


def oracle(k, recs):
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == len(recs) - nc
    return want, nc


def check_table(t, n, want, nc):
    """One assemble of table t (n k-mers in): text, contig count and lookups are the oracle's; first
    from the walk alone (walk_checks.first_attempt: no second attempt behind it)."""
    first_attempt(t, n, want, nc)
    got_nc, nb = t.assemble()
    got = t.contigs_text()
    s = t.stats()
    assert got_nc == nc == s["n_contigs"] == s["n_starts"]
    assert len(got) == nb == len(want)
    assert got == want
    assert s["n_lookups"] == n - nc
    assert s["n_missing"] == s["n_cycle"] == s["n_bad_ext"] == s["n_dup"] == s["n_full"] == 0
    return got


def check(k, recs, want, nc, load=0.5):
    with kh.KmerHashTable(k, max(len(recs), 1), load, device=0) as t:
        t.insert_all(recs)
        return check_table(t, len(recs), want, nc)


def check_contigs(k, lens, seed, load=0.5, order="shuffled"):
    text, contigs = cases.contigs_text(k, lens, seed, order)
    recs = kh.pack_text(k, text)
    want, nc = oracle(k, recs)
    assert want == cases.contigs_truth(contigs) and nc == len(lens)
    if order == "last":  # the text ends with the longest contig
        assert len(contigs[-1]) - k + 1 == max(lens) and want.endswith(contigs[-1].encode() + b"\n")
    return check(k, recs, want, nc, load)


# ---- a. deferred splitter segments within one reservation ---------------------------------------
@pytest.mark.parametrize("order", ["first", "last", "shuffled"])
@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("bits", [None, "4"])
@pytest.mark.parametrize("k", [19, 31, 51])
def test_deferred_segments_one_reservation(monkeypatch, k, bits, shape, order):
    """The reservation of the walker queue that crosses n_starts also reaches the queue's end
    (shape A: the first reservation, n_starts + n_splits <= 64; shape B: the second, <= 128): the
    wave that holds it defers every splitter walker while no contig has stopped at a splitter yet,
    then the 120-k-mer contig stops at one after >= 16 bases, and the second launch has to walk the
    splitter segments. (The deferring wave used to record the deferral only if the queue head was
    still below n_all when it moved it, which it never is here: the second launch returned at once
    and the long contig was cut short.) The preconditions are asserted from the Python mirror of
    split_hash before the GPU is touched. Default splitter density (2^4 at this size, taken by
    kh_assemble_dev) and KH_SPLIT_BITS=4 (forced: no filter pass); the eager walk
    (KH_DEBUG=seg_eager: every walker stops at every splitter) gives the same text."""
    text, contigs, f = cases.deferred_case(k, shape, order)
    ns, n_all = f["ns"], f["n_all"]
    assert f["n"] // ns <= 16 and f["nsp"] >= 1 and f["stops"] and min(f["stops"]) >= 16
    if shape == "A":
        assert ns == 31 and n_all <= 64
    else:
        assert 64 < ns < 128 and n_all <= 128
    monkeypatch.delenv("KH_SPLIT_BITS", raising=False)
    if bits is not None:
        monkeypatch.setenv("KH_SPLIT_BITS", bits)
    monkeypatch.delenv("KH_DEBUG", raising=False)
    recs = kh.pack_text(k, text)
    assert len(recs) == f["n"]
    want, nc = oracle(k, recs)
    assert want == cases.contigs_truth(contigs) and nc == ns
    got = check(k, recs, want, nc)
    monkeypatch.setenv("KH_DEBUG", "seg_eager")
    assert check(k, recs, want, nc) == got


# ---- b. queue and wave edges ------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 300])
@pytest.mark.parametrize("ns", cases.WALKER_COUNTS)
@pytest.mark.parametrize("k", [19, 51, 31])
def test_walker_count_edges(k, ns, extra):
    """ns contigs of 1-4 k-mers, alone and with one contig of 300 k-mers that stops at splitters:
    walker counts one below / at / one above a wave (64), a block (256 with the splitter walkers)
    and the reservation sizes. The walk is in deferred mode (mean contig <= 16 k-mers) in every
    case but ns = 1 and 2 with the long contig (means of ~150 and ~100 k-mers): those two walk
    eagerly (split_min = 0)."""
    check_contigs(k, cases.short_lens(ns, 7 * k + ns, extra), seed=k + ns + extra)


@pytest.mark.parametrize("ns", [1, 3, 64])
@pytest.mark.parametrize("k", [19, 51, 31])
def test_walker_count_edges_eager(k, ns):
    """Contigs of 40 k-mers (mean above the splitter spacing: the eager walk, split_min = 0)."""
    check_contigs(k, [40] * ns, seed=3 * k + ns)


# ---- c. key-layout boundaries -------------------------------------------------------------------
K_BOUNDARIES = [12, 13, 14, 19, 20, 21, 22, 29, 30, 31, 32, 40, 41, 52, 53, 60]


@functools.lru_cache(maxsize=None)
def boundary_case(k):
    """Records, the oracle's text and table, and 300 random keys with the oracle's answer."""
    if k >= 14:
        recs = kh.SyntheticKmers(k, 60_000, 1, 300, 50, seed=k).records()
    else:
        rng = np.random.default_rng(k)
        lens = []
        while len(lens) < 64 and sum(lens) <= 1940:  # at most 2,000 k-mers
            lens.append(int(rng.integers(1, 60)))
        recs = kh.pack_text(k, cases.contigs_text(k, lens, seed=k)[0])
    want, nc = oracle(k, recs)
    ot = ob.Table(k, 2 * len(recs))
    for r in recs:
        assert ot.insert(r)
    rng = np.random.default_rng(1000 + k)
    probes = np.stack([kh.pack_kmer(k, "".join("ACGT"[x] for x in rng.integers(0, 4, k))) for _ in range(300)])
    answers = [ot.find(p) for p in probes]
    return recs, want, nc, probes, answers


@pytest.mark.parametrize("load", [0.5, 0.9])
@pytest.mark.parametrize("insert", ["cas", "part"])
@pytest.mark.parametrize("k", K_BOUNDARIES)
def test_k_boundaries(monkeypatch, k, insert, load):
    """Both sides of every k at which make_params / kh_kernels.hip change the layout: chain links
    on / off (13|14, 21|22, 52|53), the minimizer length (13|14, 19|20, 30|31), one or two words
    per slot (29|30), the first non-zero hi_mask (31|32), the successor field entirely in the upper
    dword (40|41: k_rec_succ beside or before the walk). Two walks of one table (the second reads
    resolved records only), then find of every inserted key and of 300 random keys against the
    oracle's table."""
    monkeypatch.setenv("KH_INSERT", insert)
    recs, want, nc, probes, answers = boundary_case(k)
    P = kh.packed_size(k)
    with kh.KmerHashTable(k, len(recs), load, device=0) as t:
        t.insert_all(recs)
        for _ in range(2):
            check_table(t, len(recs), want, nc)
        got, found = t.find(recs[:, :P])
        assert found.all() and np.array_equal(got, recs)
        got, found = t.find(probes)
        for i, (ok, rec) in enumerate(answers):
            assert found[i] == ok
            if ok:
                assert np.array_equal(got[i], rec)
        assert np.all(got[~found] == 0)


# ---- d. text-size edges for the two line writers ------------------------------------------------
TEXT_SIZES = [1023, 1024, 1025, 2047, 2048, 2049, 4096]


# (K + 1 bytes hold no contig of 300 k-mers: that size has no long_tail variant)
@pytest.mark.parametrize("T,long_tail", [("K+1", False)] + [(T, lt) for T in TEXT_SIZES for lt in (False, True)])
@pytest.mark.parametrize("K", [15, 16, 31, 32, 51])
def test_text_size_edges(K, T, long_tail):
    """Texts of exactly T bytes: one single k-mer (K + 1), and one byte below / at / above the
    1-KiB block of k_write_lines (16 <= K < 32), the 2-KiB block of k_write_lines32 (K >= 32) and
    their multiples; K = 15 keeps the heads writer. Contigs of 1-3 k-mers (a contig boundary in most
    16-B lanes), one of them sized to make the text T bytes; with long_tail that one has >= 300
    k-mers and its start record is the input's last, so it is the last contig and the text ends
    in bytes the chunk writer owns (its bases past the first 256 appended ones)."""
    T = K + 1 if T == "K+1" else T
    lens = cases.lens_for_text_bytes(K, T, seed=K + T, long_tail=long_tail)
    if long_tail:
        assert lens[-1] >= 300 and max(lens[:-1], default=0) <= 3
    got = check_contigs(K, lens, seed=K + T, order="last" if long_tail else "shuffled")
    assert len(got) == T
    if long_tail:  # (check_contigs: the longest contig is the last one of the oracle's text)
        assert len(got.splitlines()[-1]) == lens[-1] + K - 1 > 256 + K
