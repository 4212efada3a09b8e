"""GPU: find over text (kh_find_text_dev / kh_find_text / kh_text_keys_dev, KmerHashTable.find_text,
GpuShard.find_text / text_keys, DistributedKmerHashMap.find_text).

Expected answers come from the input records alone (text_cases.expected_find_text: numpy window
mask, its own packer, cases.RecordDict), never from the code under test; answers are compared byte
for byte and counts exactly. test_find_text_cpu.py checks that no case used here is vacuous."""
import ctypes

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import text_cases as tc
from cases import RecordDict
from test_gpu_find_dist import insert_block, run_ranks

pytestmark = pytest.mark.gpu

_want = {}


def want_of(k, recs, text, tag):
    """expected_find_text, computed once per (case, text)."""
    key = (k, tag, hash(bytes(text)))
    if key not in _want:
        _want[key] = tc.expected_find_text(k, recs, text)
    return _want[key]


def table_of(k, recs, load=0.5):
    t = kh.KmerHashTable(k, max(len(recs), 1), load_factor=load)
    if len(recs):
        t.insert_all(recs)
    return t


def assert_same(got, want, what=""):
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    assert got[0].shape == want[0].shape and got[0].dtype == np.uint8, what
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert not len(bad), (what, len(bad), bad[:8], got[0][bad[:8]].tolist(), want[0][bad[:8]].tolist())


# ---- 1, 2, 3, 4: k coverage, absent k-mers, dirty text, lengths ---------------------------------
@pytest.mark.parametrize("k", tc.K_COVER)
def test_contig_text_every_window_found(k):
    """The walk's own output queried against the table it came from: every window found, every
    answer the neighbouring text bytes ('F' at line ends)."""
    case = tc.contig_case(k)
    with table_of(k, case["recs"]) as t:
        t.assemble()
        text = t.contigs_text()
        assert text == case["truth"]
        got = t.find_text(text)
    assert got[1] == got[2] == len(case["recs"])
    assert np.array_equal(got[0], tc.neighbour_answers(k, text))
    assert_same(got, want_of(k, case["recs"], text, "truth"))


@pytest.mark.parametrize("k", tc.K_COVER)
def test_absent_kmers(k):
    case = tc.contig_case(k)
    text = tc.mutated_text(case["truth"])
    with table_of(k, case["recs"]) as t:
        got = t.find_text(np.frombuffer(text, np.uint8))  # a numpy array this time
    assert got[1] - got[2] >= 100
    assert_same(got, want_of(k, case["recs"], text, "mutated"))


@pytest.mark.parametrize("k", tc.K_COVER)
def test_dirty_text(k):
    case = tc.contig_case(k)
    text = tc.dirty_text(k, case["contigs"])
    with table_of(k, case["recs"]) as t:
        got = t.find_text(text)
    assert_same(got, want_of(k, case["recs"], text, "dirty"))


@pytest.mark.parametrize("k", tc.K_COVER)
def test_lengths(k):
    case = tc.contig_case(k)
    long = max(case["contigs"], key=len)
    with table_of(k, case["recs"]) as t:
        for text in tc.length_texts(k, long):
            got = t.find_text(text)
            assert got[0].shape == (len(text), 2)
            assert_same(got, tc.expected_find_text(k, case["recs"], text), len(text))


# ---- 5: tile edges and alignment ----------------------------------------------------------------
@pytest.mark.parametrize("k", [19, 51])
def test_tile_edges_and_alignment(k):
    """A line of several tiles, shifted by 0..3 bytes against the tile grid, the device text and the
    output each at 0, 1, 7 and 15 bytes from a 16-byte boundary; nothing outside the output range
    is written."""
    import torch
    case = tc.tile_case(k)
    G = 32  # guard bytes on each side of the output
    with table_of(k, case["recs"]) as t:
        for pre, text in enumerate(tc.tile_texts(case)):
            want = want_of(k, case["recs"], text, f"tile{pre}")
            n = len(text)
            for j, to in enumerate(tc.POINTER_OFFSETS):
                eo = tc.POINTER_OFFSETS[(j + pre) % 4]
                tbuf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
                tbuf[to:to + n] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
                obuf = torch.full((2 * n + 2 * G + 16,), 0xA5, dtype=torch.uint8, device="cuda")
                counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
                assert tbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                t.find_text_dev(tbuf.data_ptr() + to, n, obuf.data_ptr() + G + eo, counts.data_ptr())
                t.sync()
                out = obuf.cpu().numpy()
                assert (out[:G + eo] == 0xA5).all() and (out[G + eo + 2 * n:] == 0xA5).all(), (pre, to, eo)
                got = (out[G + eo:G + eo + 2 * n].reshape(n, 2), *counts.cpu().tolist())
                assert_same(got, want, (pre, to, eo))


# ---- 6: NULL arguments --------------------------------------------------------------------------
def test_null_arguments():
    import torch
    k = 51
    case = tc.contig_case(k)
    text = tc.dirty_text(k, case["contigs"])
    want = want_of(k, case["recs"], text, "dirty")
    n = len(text)
    with table_of(k, case["recs"]) as t:
        dtext = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
        ext = torch.full((n, 2), 0x5A, dtype=torch.uint8, device="cuda")
        counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t.find_text_dev(dtext.data_ptr(), n, None, counts.data_ptr())  # counts only
        t.sync()
        assert tuple(counts.cpu().tolist()) == want[1:] and (ext.cpu().numpy() == 0x5A).all()
        counts.fill_(-1)
        torch.cuda.synchronize()
        t.find_text_dev(dtext.data_ptr(), n, ext.data_ptr(), None)  # answers only
        t.sync()
        assert np.array_equal(ext.cpu().numpy(), want[0]) and counts.cpu().tolist() == [-1, -1]
        for args in ((dtext.data_ptr(), n, None, None), (None, n, ext.data_ptr(), counts.data_ptr())):
            with pytest.raises(kh.KmerHashError) as e:
                t.find_text_dev(*args)
            assert e.value.code == _lib.KH_ERR_ARG
        # the host form takes the same holes
        L = _lib.lib()
        buf = np.frombuffer(text, np.uint8)
        hc = np.zeros(2, np.uint64)
        he = np.empty((n, 2), np.uint8)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        assert L.kh_find_text(t._h, p(buf), n, None, p(hc)) == _lib.KH_OK and tuple(int(x) for x in hc) == want[1:]
        assert L.kh_find_text(t._h, p(buf), n, p(he), None) == _lib.KH_OK and np.array_equal(he, want[0])
        assert L.kh_find_text(t._h, p(buf), n, None, None) == _lib.KH_ERR_ARG
        assert L.kh_find_text(t._h, None, n, p(he), p(hc)) == _lib.KH_ERR_ARG
        # len == 0: nothing written
        hc[:] = 7
        assert L.kh_find_text(t._h, None, 0, p(he), p(hc)) == _lib.KH_OK and list(hc) == [7, 7]


# ---- 7: table states ----------------------------------------------------------------------------
def test_empty_and_cleared_table():
    k = 51
    case = tc.contig_case(k)
    text = case["truth"]
    want = tc.expected_find_text(k, case["recs"][:0], text)
    assert want[1] == len(case["recs"]) and want[2] == 0
    with kh.KmerHashTable(k, len(case["recs"])) as t:
        assert_same(t.find_text(text), want, "empty")
        t.insert_all(case["recs"])
        assert t.find_text(text)[2] == want[1]
        t.clear()
        assert_same(t.find_text(text), want, "cleared")


def test_open_staged_insert_is_a_state_error():
    import torch
    from cs267_hw3_amd.dist import GpuShard
    k = 51
    case = tc.contig_case(k)
    recs, n = case["recs"], len(case["recs"])
    text = case["truth"]
    sh = GpuShard(k, n)
    with torch.cuda.stream(sh.stream):
        dev = torch.from_numpy(recs).to(sh.dev)
        dtext = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(sh.dev)
        words, _ = sh.route(dev, 1)
        sh.stage_words(words, n, n)
        with pytest.raises(kh.KmerHashError) as e:
            sh.find_text(dtext)
        assert e.value.code == _lib.KH_ERR_STATE
        sh.finish_words()
        ext, counts = sh.find_text(dtext)
        sh.sync()
        assert_same((ext.cpu().numpy(), *counts.cpu().tolist()), want_of(k, recs, text, "truth"))
    sh.table.close()


@pytest.mark.parametrize("k", [19, 51])
def test_table_at_load_085(k):
    case = tc.contig_case(k)
    text = tc.mutated_text(case["truth"])
    with table_of(k, case["recs"], load=0.85) as t:
        assert t.capacity < len(case["recs"]) / 0.84
        assert_same(t.find_text(text), want_of(k, case["recs"], text, "mutated"))


def test_hot_regions():
    """Keys placed by the hot-region remap are found through the same place / home_of."""
    case = tc.hot_case(kh.SyntheticKmers)
    with table_of(51, case["recs"]) as t:
        assert t.stats()["n_hot_regions"] > 0
        got = t.find_text(case["truth"])
    assert got[1] == got[2] == 200_000
    assert_same(got, want_of(51, RecordDict(51, case["recs"]), case["truth"], "hot"))


# ---- 8: no side effects -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [19, 51])
def test_no_side_effects(k):
    case = tc.contig_case(k)
    query = tc.dirty_text(k, case["contigs"]) + b"\n" + tc.mutated_text(case["truth"])
    with table_of(k, case["recs"]) as t:
        t.assemble()
        plain = t.contigs_text()
    with table_of(k, case["recs"]) as t:
        before = t.find_text(query)
        t.assemble()
        after = t.find_text(query)
        text = t.contigs_text()
    assert text == plain == case["truth"]
    assert_same(before, want_of(k, case["recs"], query, "both"))
    assert_same(after, before)


# ---- 9: kh_text_keys_dev ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [19, 30, 51, 60])
def test_text_keys(k):
    import torch
    from cs267_hw3_amd.dist import GpuShard
    case = tc.contig_case(k)
    KP = (k + 3) // 4
    texts = [tc.dirty_text(k, case["contigs"])] + tc.length_texts(k, max(case["contigs"], key=len))
    if k in (19, 51):
        texts += tc.tile_texts(tc.tile_case(k))
    sh = GpuShard(k, 16)  # an empty table: the keys need none
    with torch.cuda.stream(sh.stream):
        for j, text in enumerate(texts):
            buf = np.frombuffer(text, np.uint8)
            pos = np.flatnonzero(tc.window_mask(k, buf))
            to = tc.POINTER_OFFSETS[j % 4]
            tbuf = torch.zeros(len(buf) + 16, dtype=torch.uint8, device=sh.dev)
            tbuf[to:to + len(buf)] = torch.from_numpy(buf.copy()).to(sh.dev)
            keys, gpos, count = sh.text_keys(tbuf[to:to + len(buf)])
            sh.sync()
            m = int(count.cpu()[0])
            assert m == len(pos), (j, m, len(pos))
            assert keys.shape == (max(len(buf) - k + 1, 0), KP)
            assert np.array_equal(gpos[:m].cpu().numpy().view(np.uint32), pos.astype(np.uint32)), j
            assert np.array_equal(keys[:m].cpu().numpy(), tc.pack_windows(k, buf, pos)), j
        # 32-bit positions: refused before anything is launched
        p = sh._p
        assert sh.L.kh_text_keys_dev(sh.h, p(tbuf), 1 << 32, p(keys), p(gpos), p(count)) == _lib.KH_ERR_ARG
        assert sh.L.kh_text_keys_dev(sh.h, p(tbuf), 64, p(keys), p(gpos), None) == _lib.KH_ERR_ARG
        # the count alone
        count.fill_(-1)
        assert sh.L.kh_text_keys_dev(sh.h, p(tbuf[to:]), len(buf), None, None, p(count)) == _lib.KH_OK
        sh.sync()
        assert int(count.cpu()[0]) == len(pos)
    sh.table.close()


# ---- 10: sharded --------------------------------------------------------------------------------
@pytest.mark.parametrize("P,self_exchange", [(1, False), (1, True), (2, False), (3, False)])
def test_sharded_find_text(P, self_exchange):
    """The four texts (dirty, mutated, empty, shorter than k) go round the ranks: in round j rank r
    asks text (r + j) % 4, as a device tensor in the first four rounds and as host bytes / numpy in
    the last two. One rank: the fused kernel, or (forced self-exchange) the keys path."""
    import torch
    k = 51
    case = tc.contig_case(k)
    recs = case["recs"]
    texts = tc.shard_texts(k)
    wants = [want_of(k, recs, x, f"shard{i}") for i, x in enumerate(texts)]

    def body(r, dm, shard, comm):
        if self_exchange:
            dm.SELF_EXCHANGE = True
        insert_block(dm, shard, comm, recs, P, r)
        out = []
        for j in range(6):
            i = (r + j) % 4
            if j < 4:
                dev = torch.from_numpy(np.frombuffer(texts[i], np.uint8).copy()).to(shard.dev)
                ext, counts = dm.find_text(dev)
                assert torch.is_tensor(ext) and ext.dtype == torch.uint8 and tuple(ext.shape) == (len(texts[i]), 2)
                shard.sync()
                out.append((i, (ext.cpu().numpy(), *counts.cpu().tolist())))
            else:
                ext, windows, found = dm.find_text(texts[i] if j == 4 else np.frombuffer(texts[i], np.uint8))
                assert isinstance(ext, np.ndarray) and isinstance(windows, int) and isinstance(found, int)
                out.append((i, (ext, windows, found)))
        return out

    for r, out in enumerate(run_ranks(k, P, len(recs), body)):
        assert len(out) == 6
        for i, got in out:
            assert_same(got, wants[i], f"rank {r} text {i}")
