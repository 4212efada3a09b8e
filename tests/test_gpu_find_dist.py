"""GPU: the batched find across shards (kh_find_route_dev / kh_find_answer_dev / kh_find_gather_dev,
DistributedKmerHashMap.find) with P logical ranks on one GPU (ThreadComm).

Expected answers come from the input records themselves (key bytes -> record, cases.RecordDict),
never from the code under test: a present key gives its record and found = 1, an absent key a
zeroed record and found = 0, byte for byte."""
import ctypes
import gc
import json
import os
import threading

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cases import RecordDict

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))


def absent_keys(k, d, present, limit=None):
    """Present keys with one base changed (base i % k of key i; the pad bits stay 0), without those
    that are keys of the set."""
    q = np.array(present[:limit] if limit else present, dtype=np.uint8, copy=True)
    i = np.arange(len(q))
    base = i % k
    q[i, base // 4] ^= (1 << (6 - 2 * (base % 4))).astype(np.uint8)
    return q[d.lookup(q)[1] == 0]


def query_mix(k, d, recs, rank, n_absent=None, size=None):
    """Rank `rank`'s seeded shuffle of every present key, absent keys and a few repeats, cut to
    `size` keys when given; never a multiple of 64 unless `size` says so."""
    KP = (k + 3) // 4
    present = recs[:, :KP]
    q = np.concatenate([present, absent_keys(k, d, present, n_absent), present[:7], present[:3]])
    q = q[np.random.default_rng(1000 + rank).permutation(len(q))]
    if size is not None:
        return np.ascontiguousarray(q[:size])
    if len(q) % 64 == 0:
        q = q[:-1]
    return np.ascontiguousarray(q)


def rank_sizes(P, r):
    """One rank asks nothing, one asks one key, the others their whole mix (None)."""
    if P >= 3:
        return 0 if r == P - 1 else 1 if r == P - 2 else None
    if P == 2:
        return 1 if r == 1 else None
    return None


def run_ranks(k, P, n_hint, body, device=0):
    """P logical ranks as threads: body(r, dm, shard, comm) under the shard's stream; returns the
    per-rank results (the map itself is needed, which dist.run_threaded does not expose)."""
    import torch
    from cs267_hw3_amd.dist import DistributedKmerHashMap, GpuShard, ThreadComm
    gc.collect()
    torch.cuda.empty_cache()
    comms = ThreadComm.group(P)
    out, errs = [None] * P, []

    def run(r):
        try:
            torch.cuda.set_device(device)
            shard = GpuShard(k, max(n_hint // P, 1), device=device)
            with torch.cuda.stream(shard.stream):
                dm = DistributedKmerHashMap(comms[r], shard)
                out[r] = body(r, dm, shard, comms[r])
                shard.sync()
            shard.table.close()
        except BaseException as ex:
            errs.append(ex)
            comms[r].sh.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        errs.sort(key=lambda e: isinstance(e, threading.BrokenBarrierError))
        raise errs[0]
    return out


def insert_block(dm, shard, comm, recs, P, r):
    import torch
    n = len(recs)
    split = (n + P - 1) // P
    b = min(r * split, n)
    mine = torch.from_numpy(np.ascontiguousarray(recs[b:min(b + split, n)])).to(shard.dev)
    dm.insert_all(mine)
    comm.barrier()


def find_np(dm, shard, q):
    import torch
    recs, found = dm.find(torch.from_numpy(q).to(shard.dev))
    assert recs.dtype == torch.uint8 and found.dtype == torch.uint8
    assert tuple(recs.shape) == (len(q), shard.R) and tuple(found.shape) == (len(q),)
    return recs.cpu().numpy(), found.cpu().numpy()


def assert_answers(d, q, got, what=""):
    want_r, want_f = d.lookup(q)
    assert np.array_equal(got[1], want_f), what
    assert np.array_equal(got[0], want_r), what


def load_golden(name):
    m = MANIFEST[name]
    return m, kh.pack_text(m["k"], open(os.path.join(GOLDEN, f"{name}.txt"), "rb").read())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["tiny19", "small51", "k29", "k30", "k32", "k60"])
def test_find_golden(name, P):
    """Both slot widths, the W boundary (k = 29 / 30) and the widest key; every rank another shuffle
    of present, absent and repeated keys; ranks with n = 0, n = 1 and n not a multiple of 64."""
    m, recs = load_golden(name)
    k = m["k"]
    d = RecordDict(k, recs)
    qs = [query_mix(k, d, recs, r, size=rank_sizes(P, r)) for r in range(P)]
    assert len(qs[0]) % 64 and (qs[0].shape[0] > len(recs))

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        s0 = dm.host_syncs()
        got = find_np(dm, shard, qs[r])
        return got, dm.host_syncs() - s0

    for r, (got, syncs) in enumerate(run_ranks(k, P, len(recs), body)):
        assert_answers(d, qs[r], got, f"rank {r}")
        assert syncs == 1, f"rank {r}: {syncs} blocking reads"  # the counts
    if P == 1:
        with kh.KmerHashTable(k, len(recs)) as t:
            t.insert_all(recs)
            one_r, one_f = t.find(qs[0])
        got = run_ranks(k, 1, len(recs), lambda r, dm, sh, c: (insert_block(dm, sh, c, recs, 1, 0),
                                                              find_np(dm, sh, qs[0]))[1])[0]
        assert np.array_equal(got[0], one_r) and np.array_equal(got[1].astype(bool), one_f)


def test_find_host_keys():
    """A host numpy array goes up and comes back as numpy (records, found bool)."""
    m, recs = load_golden("small51")
    d = RecordDict(51, recs)
    q = query_mix(51, d, recs, 0)

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, 2, r)
        return dm.find(q if r == 0 else q[:0])

    out = run_ranks(51, 2, len(recs), body)
    assert isinstance(out[0][0], np.ndarray) and out[0][1].dtype == bool
    assert_answers(d, q, (out[0][0], out[0][1].astype(np.uint8)))
    assert out[1][0].shape == (0, 15) and out[1][1].shape == (0,)


def test_find_all_queries_to_one_owner():
    """Only keys owned by rank 1 at P = 3: skewed splits, zero-length peers in both exchanges."""
    from cs267_hw3_amd import _lib
    m, recs = load_golden("small51")
    k, P = 51, 3
    d = RecordDict(k, recs)
    L = _lib.lib()
    with kh.KmerHashTable(k, 16) as t:
        def owner(key):
            return L.kh_key_owner(t._h, key.ctypes.data_as(_lib.c_u8p), P)
        qs = []
        for r in range(P):
            q = query_mix(k, d, recs, r)
            q = q[np.array([owner(np.ascontiguousarray(x)) == 1 for x in q])]
            qs.append(np.ascontiguousarray(q))
    assert all(len(q) > 100 for q in qs)

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        return find_np(dm, shard, qs[r])

    for r, got in enumerate(run_ranks(k, P, len(recs), body)):
        assert_answers(d, qs[r], got, f"rank {r}")
        assert got[1].sum() > 0 and (got[1] == 0).sum() > 0


def test_find_chunked_exchange():
    """A2A_CHUNK_BYTES = 4096: both exchanges run in several rounds; same answers; the return
    exchange carries 2 bytes per key."""
    m, recs = load_golden("small51")
    k, P = 51, 3
    d = RecordDict(k, recs)
    qs = [query_mix(k, d, recs, r) for r in range(P)]

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        dm.A2A_CHUNK_BYTES = 4096
        calls = [0]
        inner = comm.all_to_all

        def counting(*a):
            calls[0] += 1
            return inner(*a)
        comm.all_to_all = counting
        got = find_np(dm, shard, qs[r])
        return got, calls[0], dm.find_key_bytes, dm.find_answer_bytes

    out = run_ranks(k, P, len(recs), body)
    for r, (got, calls, kb, ab) in enumerate(out):
        assert_answers(d, qs[r], got, f"rank {r}")
        assert calls > 3  # counts + more than one round for the keys
        assert kb == len(qs[r]) * 13
    # every key asked by any rank is answered by exactly one owner with 2 bytes
    assert sum(o[3] for o in out) == 2 * sum(len(q) for q in qs)


def test_find_hash_owner(monkeypatch):
    monkeypatch.setenv("KH_OWNER", "hash")
    k, P, n = 51, 4, 500_000
    g = kh.SyntheticKmers(k, n, 8, 200, 10, seed=123)
    recs = g.records()
    d = RecordDict(k, recs)
    qs = [query_mix(k, d, recs, r, n_absent=50_000) for r in range(P)]

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        return find_np(dm, shard, qs[r]), shard.inserted

    out = run_ranks(k, P, n, body)
    for r, (got, _) in enumerate(out):
        assert_answers(d, qs[r], got, f"rank {r}")
    ins = [o[1] for o in out]
    assert sum(ins) == n and min(ins) > n // 8  # hash owners: an even split


@pytest.mark.parametrize("mode", ["cas", "part"])
def test_find_large_both_insert_paths(monkeypatch, mode):
    """>= 2.5M k-mers per shard, built by global CAS or by the partitioned region build (chain bits
    in word 0, overflow keys); 1M present + 100k absent keys per rank."""
    monkeypatch.setenv("KH_INSERT", mode)
    k, P = 51, 2
    g = kh.SyntheticKmers(k, 2_500_000 * 2, 8, 200, 0)
    recs = g.records()
    d = RecordDict(k, recs)
    qs = []
    for r in range(P):
        rng = np.random.default_rng(50 + r)
        pres = recs[rng.choice(len(recs), 1_000_000, replace=False), :13]
        q = np.concatenate([pres, absent_keys(k, d, pres, 100_000)])
        qs.append(np.ascontiguousarray(q[rng.permutation(len(q))]))

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        return find_np(dm, shard, qs[r]), shard.stats()

    out = run_ranks(k, P, len(recs), body)
    for r, (got, st) in enumerate(out):
        assert_answers(d, qs[r], got, f"rank {r}")
        assert st["n_dup"] == st["n_full"] == 0


def test_find_hot_regions():
    """Hot-motif set with flanks: 200 permille of the contigs share 4 minimizer windows (150k k-mers
    per window against ~3k-slot regions, so their regions are remapped), and the flank makes ~40 %
    of a family share the neighbour window too (the remap target overfills and is spread)."""
    k, P, n = 51, 2, 3_000_000
    g = kh.SyntheticKmers(k, n, 8, 200, 0, seed=9, hot_permille=200, n_motifs=4, hot_flank=True)
    recs = g.records()
    d = RecordDict(k, recs)
    qs = []
    for r in range(P):
        rng = np.random.default_rng(70 + r)
        pres = recs[rng.choice(len(recs), 600_000, replace=False), :13]
        q = np.concatenate([pres, absent_keys(k, d, pres, 60_000)])
        qs.append(np.ascontiguousarray(q[rng.permutation(len(q))]))

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        return find_np(dm, shard, qs[r]), shard.stats()

    out = run_ranks(k, P, n, body)
    for r, (got, st) in enumerate(out):
        assert_answers(d, qs[r], got, f"rank {r}")
    assert sum(o[1]["n_hot_regions"] for o in out) > 0, [o[1] for o in out]
    assert sum(o[1]["n_spread_regions"] for o in out) > 0, [o[1] for o in out]


def test_find_then_assemble_then_find():
    """find between insert_all and assemble changes no contig text; a find after the walk gives the
    same answers as the one before it."""
    k, P, n = 51, 3, 300_000
    g = kh.SyntheticKmers(k, n, 8, 200, 10, seed=31)
    recs = g.records()
    d = RecordDict(k, recs)
    qs = [query_mix(k, d, recs, r, n_absent=20_000) for r in range(P)]

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        before = find_np(dm, shard, qs[r])
        dm.assemble(n)
        text = dm.contigs_text()
        after = find_np(dm, shard, qs[r])
        dm.assemble(n)  # and a walk after a find after a walk
        return before, after, text, dm.contigs_text()

    for r, (before, after, text, text2) in enumerate(run_ranks(k, P, n, body)):
        assert_answers(d, qs[r], before, f"rank {r} before")
        assert_answers(d, qs[r], after, f"rank {r} after")
        b, e = g.block(P, r)
        assert text == g.truth(b, e) and text2 == text, f"rank {r}"


def test_find_after_clear():
    m, recs = load_golden("small51")
    d = RecordDict(51, recs)
    P = 2
    qs = [query_mix(51, d, recs, r) for r in range(P)]

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        first = find_np(dm, shard, qs[r])
        shard.clear()
        comm.barrier()
        return first, find_np(dm, shard, qs[r])

    for r, (first, cleared) in enumerate(run_ranks(51, P, len(recs), body)):
        assert_answers(d, qs[r], first)
        assert not cleared[1].any() and not cleared[0].any()


# ---------------------------------------------------------------------------------------------
def _check_route(sh, keys_np, P):
    import torch
    from cs267_hw3_amd import _lib
    n, KP = keys_np.shape
    # a view at an odd byte offset: key buffers may have any alignment
    buf = torch.zeros(n * KP + 3, dtype=torch.uint8, device=sh.dev)
    keys = buf[3:].view(n, KP)
    keys.copy_(torch.from_numpy(keys_np))
    out, index, counts = sh.find_route(keys, P)
    sh.sync()
    out, index, counts = out.cpu().numpy()[:n], index.cpu().numpy()[:n], counts.cpu().numpy()
    assert np.array_equal(np.sort(index), np.arange(n))         # a permutation
    assert np.array_equal(out, keys_np[index])                  # keys_out[j] == keys[index[j]]
    L = _lib.lib()
    base = out.ctypes.data
    own = np.fromiter((L.kh_key_owner(sh.h, ctypes.cast(base + j * KP, _lib.c_u8p), P) for j in range(n)),
                      dtype=np.int64, count=n)
    assert (np.diff(own) >= 0).all()                            # grouped by ascending owner
    assert counts[P] == n
    assert np.array_equal(counts[:P], np.bincount(own, minlength=P))


@pytest.mark.parametrize("P", [1, 3, 8, 64])
def test_find_route_small51(P):
    import torch
    from cs267_hw3_amd.dist import GpuShard
    m, recs = load_golden("small51")
    sh = GpuShard(51, len(recs))
    with torch.cuda.stream(sh.stream):
        _check_route(sh, np.ascontiguousarray(recs[:, :13]), P)
    sh.table.close()


def test_find_route_1m_k19():
    import torch
    from cs267_hw3_amd.dist import GpuShard
    g = kh.SyntheticKmers(19, 1_000_000, 8, 400, 10, seed=19)
    keys = np.ascontiguousarray(g.records()[:, :5])
    sh = GpuShard(19, 1024)
    with torch.cuda.stream(sh.stream):
        _check_route(sh, keys, 5)
    sh.table.close()


def test_find_argument_and_state_errors():
    import torch
    from cs267_hw3_amd import _lib
    from cs267_hw3_amd.dist import GpuShard
    m, recs = load_golden("small51")
    n = len(recs)
    sh = GpuShard(51, n)
    L, h = sh.L, sh.h
    with torch.cuda.stream(sh.stream):
        dev = torch.from_numpy(recs).to(sh.dev)
        keys = torch.from_numpy(np.ascontiguousarray(recs[:, :13])).to(sh.dev)
        out, index, counts = sh.find_route(keys, 2)
        ext = sh.find_answer(keys, n)
        p = sh._p
        r, f = torch.empty((n, 15), dtype=torch.uint8, device=sh.dev), torch.empty(n, dtype=torch.uint8, device=sh.dev)
        route = lambda nn, P, k_=p(keys), o=p(out), i=p(index), c=p(counts): L.kh_find_route_dev(h, k_, nn, P, o, i, c)  # noqa: E731
        gather = lambda nn, k_=p(keys), i=p(index), e=p(ext), rr=p(r), ff=p(f): L.kh_find_gather_dev(h, k_, nn, i, e, rr, ff)  # noqa: E731
        # n == 0 / m == 0: nothing to do, whatever the pointers
        assert route(0, 2, None, None, None, None) == _lib.KH_OK
        assert L.kh_find_answer_dev(h, None, 0, None) == _lib.KH_OK
        assert gather(0, None, None, None, None, None) == _lib.KH_OK
        # 32-bit positions, rank range, null buffers
        assert route(1 << 32, 2) == _lib.KH_ERR_ARG
        assert gather(1 << 32) == _lib.KH_ERR_ARG
        for bad in (0, -1, 65):
            assert route(n, bad) == _lib.KH_ERR_ARG
        assert route(n, 64) == _lib.KH_OK
        assert route(n, 2, None) == _lib.KH_ERR_ARG
        assert route(n, 2, p(keys), None) == _lib.KH_ERR_ARG
        assert route(n, 2, p(keys), p(out), None) == _lib.KH_ERR_ARG
        assert route(n, 2, p(keys), p(out), p(index), None) == _lib.KH_ERR_ARG
        assert L.kh_find_route_dev(None, p(keys), n, 2, p(out), p(index), p(counts)) == _lib.KH_ERR_ARG
        assert L.kh_find_answer_dev(h, None, n, p(ext)) == _lib.KH_ERR_ARG
        assert L.kh_find_answer_dev(h, p(keys), n, None) == _lib.KH_ERR_ARG
        assert L.kh_find_answer_dev(None, p(keys), n, p(ext)) == _lib.KH_ERR_ARG
        for hole in range(5):
            a = [p(keys), p(index), p(ext), p(r), p(f)]
            a[hole] = None
            assert gather(n, *a) == _lib.KH_ERR_ARG
        # a staged insert left open
        words, _ = sh.route(dev, 1)
        sh.stage_words(words, n, n)
        assert route(n, 2) == _lib.KH_ERR_STATE
        assert L.kh_find_answer_dev(h, p(keys), n, p(ext)) == _lib.KH_ERR_STATE
        assert gather(n) == _lib.KH_ERR_STATE
        sh.finish_words()
        # ... and the table answers once the build is finished
        out, index, counts = sh.find_route(keys, 1)
        recs_out, found = sh.find_gather(keys, index, sh.find_answer(out, n))
        sh.sync()
        assert found.cpu().numpy().all() and np.array_equal(recs_out.cpu().numpy(), recs)
        assert L.kh_abi_version() == 3
    sh.table.close()
