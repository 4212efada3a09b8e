"""GPU parity of the partitioned insert (KH_INSERT=part) over its dispatch space: every region count
2^9 .. 2^17 (pass 2, k_win2, sorts by rbits - 9 bits: none in a table below about 786k k-mers), the
three prefetching builds and both edges between them (RC 2048 | 2049 and 3072 | 3073), fresh and
non-fresh builds, one- and two-word slots, the compiled and the generic instances, and the generic
records pass with padded keys. part_shapes.py mirrors the dispatch and holds the cases;
test_part_shapes_cpu.py proves that every case sits where it claims to.

Every case compares with the oracle: the contig text, contig count and lookup count byte for byte
(the walk alone first: walk_checks.first_attempt), find of every inserted key record for record and
of 300 random keys, every error counter zero, and the table's capacity against the mirror's. The
capacity comes from n_kmers, not from what is inserted, so the region-count sweep costs a few
thousand records in a large, mostly empty table. All comparisons are exact."""
import ctypes
import functools

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import oracle_bind as ob
import locate_cases as lc
import part_shapes as ps
from cases import RecordDict
from test_gpu_win1 import SIZES, check_find, check_walk, dev_records, random_probes, small_case

pytestmark = pytest.mark.gpu

assert set(ps.SWEEP_SIZES) <= set(SIZES) and ps.SWEEP_SIZES[-1] == SIZES[-1]


def device_peak(reset=False):
    """Peak of the library's own device allocations (kh_device_bytes), in bytes."""
    now, peak = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().kh_device_bytes(ctypes.byref(now), ctypes.byref(peak), 1 if reset else 0))
    return peak.value


def check_part_table(t, sh):
    """The table is the one the mirror describes and its last insert was a partitioned build. (An
    earlier batch of the same table took the same path: under KH_INSERT=part use_part_build depends
    only on region_slots_fit(capacity) and n > 0, the same for every batch.)"""
    s = t.stats()
    assert t.capacity == sh.cap == s["capacity"]
    assert s["ms_build"] > 0  # only a partitioned build is timed (kh_get_stats)
    return s


def records_case(monkeypatch, k, rbits, n):
    """One batch of small_case(k, n) through kh_insert_dev into a fresh table of 2^rbits regions."""
    monkeypatch.setenv("KH_INSERT", "part")
    sh = ps.shape(k, ps.n_kmers_for(rbits, 0.5), 0.5, n)
    assert sh.rbits == rbits
    recs, want, nc, probes, answers = small_case(k, n)
    buf = dev_records(recs)
    assert buf.numel() == (n * kh.record_size(k) + 15) // 16 * 16
    device_peak(reset=True)
    with kh.KmerHashTable(k, sh.n_kmers, device=0) as t:
        t.insert_dev(buf.data_ptr(), n)
        t.sync()
        check_part_table(t, sh)
        check_walk(t, n, want, nc)
        check_find(t, k, recs, probes, answers)
        assert t.stats()["n_inserted"] == n
    print(f"k={k} rbits={rbits} n={n}: peak device bytes {device_peak()}")


# ---- a. region-count sweep ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.SWEEP_SIZES)
@pytest.mark.parametrize("k,rbits", ps.SWEEP)
def test_region_count_sweep(monkeypatch, k, rbits, n):
    """k = 19 (one word, KT 19) at every region count, k = 51 (KT 51) and k = 31 (generic two-word,
    convert pass) at some: the tile edges of pass 1 with a pass 2 that sorts. Most regions are empty
    and the rest hold one or two minimizer runs."""
    records_case(monkeypatch, k, rbits, n)


def find_all(t, q):
    got, found = t.find(q)
    return got.copy(), found.copy()


@pytest.mark.parametrize("k,rbits", ps.SWEEP_WAYS)
def test_sweep_entry_ways(monkeypatch, k, rbits):
    """The entry points of test_gpu_insert_paths.py where pass 2 sorts: records, routed words in one
    call, the same words staged in three chunks with an empty one between, and the records again, each
    after kh_clear on the one table. The records way answers as the oracle does and assembles to its
    text; every other way answers find exactly as the records way."""
    import torch
    from cs267_hw3_amd.dist import GpuShard
    monkeypatch.setenv("KH_INSERT", "part")
    n = ps.SWEEP_SIZES[2]
    sh_ = ps.shape(k, ps.n_kmers_for(rbits, 0.5), 0.5, n)
    recs, want, nc, probes, answers = small_case(k, n)
    q = np.ascontiguousarray(np.concatenate([recs[:, :kh.packed_size(k)], probes]))
    sh = GpuShard(k, sh_.n_kmers)
    try:
        assert sh.table.capacity == sh_.cap
        drecs = torch.from_numpy(np.array(recs)).to(sh.dev)
        W, a = sh.W, ps.REC_TILE + 1

        def way_records():
            sh.insert_records(drecs)

        def way_words():
            words, _ = sh.route(drecs, 1, starts=True)
            sh.insert_words(words, n)

        def way_staged():
            words, _ = sh.route(drecs, 1, starts=True)
            sh.stage_words(words, a, n)
            sh.stage_words(words[a * W:], 0, n)
            sh.stage_words(words[a * W:], n - a, n)
            sh.finish_words()

        first = None
        for name, way in (("records", way_records), ("words", way_words), ("staged", way_staged),
                          ("records_again", way_records)):
            with torch.cuda.stream(sh.stream):
                if first is not None:
                    sh.clear()
                way()
                sh.sync()
                check_part_table(sh.table, sh_)
                got = find_all(sh.table, q)
                if first is None:
                    first = got
                    check_find(sh.table, k, recs, probes, answers)
                assert np.array_equal(got[1], first[1]), f"{name}: found flags differ from the records way"
                assert np.array_equal(got[0], first[0]), f"{name}: records differ from the records way"
                s = sh.stats()
                assert s["n_inserted"] == n and s["n_dup"] == s["n_full"] == s["n_bad_ext"] == 0
                if name.startswith("records"):
                    check_walk(sh.table, n, want, nc)
    finally:
        sh.table.close()


@functools.lru_cache(maxsize=None)
def two_batch_case(k):
    """small_case of SECOND_SIZES[0] then of SECOND_SIZES[1] records as one input: the oracle's text,
    its table's answers and the locate model's positions."""
    n1, n2 = ps.SECOND_SIZES
    r1, r2 = small_case(k, n1)[0], small_case(k, n2)[0]
    recs = np.concatenate([r1, r2])
    n = len(recs)
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == n - nc
    ot = ob.Table(k, 2 * n)
    for r in recs:
        assert ot.insert(r)  # (no k-mer in both batches)
    probes = random_probes(k, 13 * k)
    want_pos = lc.expected_locate_text(k, lc.position_dict(k, want), want)
    return r1, r2, recs, want, nc, probes, [ot.find(p) for p in probes], want_pos


@pytest.mark.parametrize("k,rbits", ps.SWEEP_SECOND)
def test_sweep_second_batch_and_locate(monkeypatch, k, rbits):
    """A second batch into the non-empty table (the non-fresh build: slices read back, chains
    rebuilt) where pass 2 sorts, then the position index, one word per slot of the same placement:
    locate_text of the contig text against locate_cases' model."""
    monkeypatch.setenv("KH_INSERT", "part")
    r1, r2, recs, want, nc, probes, answers, (pos, windows, located) = two_batch_case(k)
    n = len(recs)
    sh = ps.shape(k, ps.n_kmers_for(rbits, 0.5), 0.5, len(r2))
    b1, b2 = dev_records(r1), dev_records(r2)
    with kh.KmerHashTable(k, sh.n_kmers, device=0) as t:
        t.insert_dev(b1.data_ptr(), len(r1))
        t.insert_dev(b2.data_ptr(), len(r2))
        t.sync()
        check_part_table(t, sh)
        check_walk(t, n, want, nc)
        check_find(t, k, recs, probes, answers)
        t.locate_build()
        got_pos, got_windows, got_located = t.locate_text(want)
        assert (got_windows, got_located) == (windows, located) and located == n
        assert np.array_equal(got_pos, pos)


# ---- b. window spill with a pass 2 that sorts ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spill_case():
    k = ps.SPILL_K
    first = small_case(k, ps.SPILL_FIRST)[0]
    hot = kh.SyntheticKmers(k, ps.SPILL_HOT, 8, 200, 0, seed=3, hot_permille=1000, n_motifs=1).records()
    recs = np.concatenate([first, hot])
    n = len(recs)
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == n - nc
    ot = ob.Table(k, 2 * n)
    for r in recs:
        assert ot.insert(r)
    probes = random_probes(k, 11)
    return first, hot, recs, want, nc, probes, [ot.find(p) for p in probes]


@pytest.mark.parametrize("rbits", ps.SPILL_RBITS)
def test_window_spill_with_sorting_pass2(monkeypatch, rbits):
    """test_win1_window_spill's one-motif hot set as a second batch (no sampling, no remap before
    pass 1) into a table of 2^11 and 2^15 regions: one bucket's pass-1 windows and one region window
    take a fraction of it, the rest goes through the overflow list."""
    monkeypatch.setenv("KH_INSERT", "part")
    k = ps.SPILL_K
    first, hot, recs, want, nc, probes, answers = spill_case()
    n = len(recs)
    sh = ps.shape(k, ps.n_kmers_for(rbits, 0.5), 0.5, len(hot))
    b0, b1 = dev_records(first), dev_records(hot)
    with kh.KmerHashTable(k, sh.n_kmers, device=0) as t:
        t.insert_dev(b0.data_ptr(), len(first))
        t.insert_dev(b1.data_ptr(), len(hot))
        t.sync()
        s = check_part_table(t, sh)
        assert s["n_overflow"] > 0
        check_walk(t, n, want, nc)
        check_find(t, k, recs, probes, answers)


# ---- c. build variants at their edges -----------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def big_set(k, n):
    """n synthetic k-mers, shared by the fresh and the non-fresh case of one build (neighbours in
    BUILD_PARAMS; one set is kept): the records, the oracle's text (the generator's truth) and contig
    count, 300 probes (200 random keys, 100 of the set) and a dictionary of the records: too many keys
    for the Python loop over the oracle's table."""
    g = kh.SyntheticKmers(k, n, 8, 300, 10, seed=k + n % 97)
    big = g.records()
    assert len(big) == n
    rc, want, nc, nl, _, _ = ob.assemble(k, big)  # rc 0: no duplicate, every walk ends
    assert rc == 0 and nl == n - nc and want == g.truth() and nc == g.num_contigs
    probes = np.concatenate([random_probes(k, n % 1000, 200), big[::n // 100, :kh.packed_size(k)][:100]])
    return big, want, nc, probes, RecordDict(k, big)


def big_case(k, n, first):
    """big_set(k, n) after small_case(k, first)'s records when first > 0: (first batch, big batch, all
    records, text, contigs, probes, their records and found flags). The two sets share no k-mer
    (asserted) and each is closed under its extensions, and the oracle walks the starts in record
    order: its text of the concatenation is the first set's text followed by the big set's."""
    big, want, nc, probes, d = big_set(k, n)
    p_recs, p_found = d.lookup(probes)
    if not first:
        return big[:0], big, big, want, nc, probes, (p_recs, p_found)
    head, head_want, head_nc = small_case(k, first)[:3]
    P = kh.packed_size(k)
    assert not d.lookup(head[:, :P])[1].any()
    h_recs, h_found = RecordDict(k, head).lookup(probes)
    assert not (h_found & p_found).any()
    return (head, big, np.concatenate([head, big]), head_want + want, head_nc + nc, probes,
            (p_recs | h_recs, p_found | h_found))


BUILD_PARAMS = [(name, k, fresh) for k in ps.BUILD_KS for name in ps.BUILD_CASES for fresh in (True, False)]


@pytest.mark.parametrize("name,k,fresh", BUILD_PARAMS)
def test_build_variant_edges(monkeypatch, name, k, fresh):
    """Each build of part_shapes.BUILD_CASES (the windows of 2048 | 2049 and 3072 | 3073 words
    between the 4-, 6- and 12-word prefetching builds, a 12-word build on balanced bounds, a 6-word
    one behind a sorting pass 2), into a fresh table and as a second batch after 65 records, at
    k = 19, 31 and 51; then the same input under KH_DEBUG=plain_build: the one-region-at-a-time kernel
    must give the same text and answer every find the same."""
    monkeypatch.setenv("KH_INSERT", "part")
    n_kmers, n, sh = ps.build_case(name, k, fresh)
    assert sh.variant == ps.BUILD_CASES[name][3]
    head, big, recs, want, nc, probes, (p_recs, p_found) = big_case(k, n, 0 if fresh else ps.BUILD_FIRST)
    assert len(big) == sh.n_batch and len(recs) == n_kmers
    bufs = [dev_records(b) for b in (head, big) if len(b)]
    counts = [len(b) for b in (head, big) if len(b)]
    P = kh.packed_size(k)
    answers = []
    for debug in ("", "plain_build"):
        monkeypatch.setenv("KH_DEBUG", debug)
        with kh.KmerHashTable(k, n_kmers, sh.load, device=0) as t:
            for buf, m in zip(bufs, counts):
                t.insert_dev(buf.data_ptr(), m)
            t.sync()
            check_part_table(t, sh)
            check_walk(t, len(recs), want, nc)
            got, found = t.find(recs[:, :P])
            assert found.all() and np.array_equal(got, recs)
            got, found = t.find(probes)
            assert np.array_equal(found, p_found.astype(bool)) and np.array_equal(got, p_recs)
            answers.append((got, found))
    assert np.array_equal(answers[0][0], answers[1][0]) and np.array_equal(answers[0][1], answers[1][1])


# ---- d. generic records pass with padded keys ---------------------------------------------------------
@pytest.mark.parametrize("n", ps.SWEEP_SIZES)
@pytest.mark.parametrize("rbits", ps.PAD_RBITS)
@pytest.mark.parametrize("k", ps.PAD_KS)
def test_generic_records_pass_padding(monkeypatch, k, rbits, n):
    """k = 17, 18 (5 packed bytes) and 49, 50 (13): k_win1_rec's generic instance with 3 and 2 padding
    bases, from a buffer of exactly n * R bytes rounded up to 16, without and with a sorting pass 2."""
    records_case(monkeypatch, k, rbits, n)
