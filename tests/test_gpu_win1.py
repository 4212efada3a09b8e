"""GPU parity of the partitioned insert's pass 1 at the record counts where it can go wrong: the
records pass (k_win1_rec: k = 51 and 19, the compile-time packed sizes) stages each wave's 16-B
blocks in LDS and reads every record from there, and the windowed sort shared by the three passes
(sort_reserve_write; k = 31 takes the convert pass and the words pass 1 through it) writes each run
from one LDS word per item. Every case inserts device records with insert_dev under KH_INSERT=part
from a buffer of exactly n * R bytes rounded up to 16 (at k = 51 the last record's 16-B block is
the buffer's last), compares the contig text, n_contigs and n_lookups byte for byte with the
oracle, and runs find for every key and for 300 random keys against the oracle's table."""
import functools

import numpy as np
import pytest

import cs267_hw3_amd as kh
import oracle_bind as ob
import cases
from walk_checks import first_attempt

pytestmark = pytest.mark.gpu

REC_TILE = 3584  # records per tile of k_win1_rec (kh_build.hip)
# one below / at / one above a wave, one, two and three tiles
SIZES = (1, 63, 64, 65, 3583, 3584, 3585, 7167, 7168, 7169, 3 * REC_TILE + 1)


def dev_records(recs):
    """The records in a device buffer of exactly their bytes rounded up to 16."""
    import torch
    flat = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1)
    buf = torch.zeros((flat.size + 15) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    buf[:flat.size] = torch.from_numpy(flat)
    return buf


def random_probes(k, seed, m=300):
    rng = np.random.default_rng(seed)
    return np.stack([kh.pack_kmer(k, "".join("ACGT"[x] for x in rng.integers(0, 4, k))) for _ in range(m)])


@functools.lru_cache(maxsize=None)
def small_case(k, n):
    recs = kh.pack_text(k, cases.contigs_text(k, cases.route_lens(n, seed=n), seed=1000 * k + n)[0])
    assert len(recs) == n
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == n - nc
    ot = ob.Table(k, 2 * n)
    for r in recs:
        assert ot.insert(r)
    probes = random_probes(k, 7 * k + n)
    return recs, want, nc, probes, [ot.find(p) for p in probes]


def check_walk(t, n, want, nc):
    first_attempt(t, n, want, nc)  # the walk alone: kh_assemble's second attempt cannot repair it
    got_nc, nb = t.assemble()
    s = t.stats()
    assert got_nc == nc == s["n_contigs"]
    assert s["n_lookups"] == n - nc
    assert nb == len(want) and t.contigs_text() == want
    assert s["n_missing"] == s["n_cycle"] == s["n_bad_ext"] == s["n_dup"] == s["n_full"] == 0
    return s


def check_find(t, k, recs, probes, answers):
    P = kh.packed_size(k)
    got, found = t.find(recs[:, :P])
    assert found.all() and np.array_equal(got, recs)
    got, found = t.find(probes)
    for i, (ok, rec) in enumerate(answers):
        assert found[i] == ok
        if ok:
            assert np.array_equal(got[i], rec)
    assert np.all(got[~found] == 0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", [51, 19, 31])
def test_win1_record_counts(monkeypatch, k, n):
    monkeypatch.setenv("KH_INSERT", "part")
    recs, want, nc, probes, answers = small_case(k, n)
    buf = dev_records(recs)
    assert buf.numel() == (n * kh.record_size(k) + 15) // 16 * 16
    with kh.KmerHashTable(k, n, device=0) as t:
        t.insert_dev(buf.data_ptr(), n)
        t.sync()
        check_walk(t, n, want, nc)
        check_find(t, k, recs, probes, answers)


def test_win1_block_with_odd_tile_count(monkeypatch):
    """k_win1_rec runs round_up(2 * CUs, 8) persistent blocks (two resident per CU) over tiles
    t, t + grid, ...: 2 * grid tiles plus one record give block 0 three tiles and every other block
    two, so a block parses a tile into the LDS its previous tile's write-out just left, and block
    0's last tile has no partner. Too many keys for the Python loop over the oracle's table: the
    oracle's assemble accepted every record (no duplicate), so find of a key is its record, and a
    random 51-mer is absent."""
    import torch
    monkeypatch.setenv("KH_INSERT", "part")
    k = 51
    grid = (2 * torch.cuda.get_device_properties(0).multi_processor_count + 7) // 8 * 8
    n = 2 * grid * REC_TILE + 1
    recs = kh.SyntheticKmers(k, n, 8, 200, 10, seed=n).records()
    assert len(recs) == n
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == n - nc
    buf = dev_records(recs)
    with kh.KmerHashTable(k, n, device=0) as t:
        t.insert_dev(buf.data_ptr(), n)
        t.sync()
        check_walk(t, n, want, nc)
        got, found = t.find(recs[:, :kh.packed_size(k)])
        assert found.all() and np.array_equal(got, recs)
        got, found = t.find(random_probes(k, 5))
        assert not found.any() and not got.any()


def test_win1_window_spill(monkeypatch):
    """More than CAP1 words in one pass-1 window: 20,000 k-mers sharing one minimizer motif, inserted
    into a table that already holds a batch (only an empty table samples and remaps hot regions
    before pass 1), all fall into the 8 windows of one bucket (CAP1 is about 117 words at this size), so
    the sort's spill branch sends most of every tile to the overflow list."""
    monkeypatch.setenv("KH_INSERT", "part")
    k = 51
    first = small_case(k, 65)[0]
    hot = kh.SyntheticKmers(k, 20_000, 8, 200, 0, seed=3, hot_permille=1000, n_motifs=1).records()
    recs = np.concatenate([first, hot])
    n = len(recs)
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == n - nc
    ot = ob.Table(k, 2 * n)
    for r in recs:
        assert ot.insert(r)
    probes = random_probes(k, 11)
    b0, b1 = dev_records(first), dev_records(hot)
    with kh.KmerHashTable(k, n, device=0) as t:
        t.insert_dev(b0.data_ptr(), len(first))
        t.insert_dev(b1.data_ptr(), len(hot))
        t.sync()
        assert t.stats()["n_overflow"] > 0
        check_walk(t, n, want, nc)
        check_find(t, k, recs, probes, [ot.find(p) for p in probes])
