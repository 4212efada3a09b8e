"""GPU: the insert entry points of the C ABI agree with each other.

One record set goes into a fresh table five ways (kh_insert; kh_insert_dev in three batches; routed
words through kh_insert_words_dev; the same words through kh_insert_words_stage_dev ..
kh_insert_words_finish with an empty batch between; the device and the staged way again after
kh_clear on the same table). Every way must answer a find of every key plus 64 changed keys exactly
as the first way does, the record ways must assemble to the oracle's text byte for byte, and every
way must cost the blocking host waits (kh_host_syncs) it cost before the entry points shared one
pipeline.

N = 3 * 8192 + 77 is no multiple of 64 or of the 8192-record convert tile, and the batch sizes
8192 + 1, 1, rest split mask words and tiles across batches."""
import functools

import numpy as np
import pytest

import cs267_hw3_amd as kh
import oracle_bind as ob

pytestmark = pytest.mark.gpu

N = 3 * 8192 + 77
CUTS = (0, 8192 + 1, 8192 + 2, N)

# kh_host_syncs after each way (insert calls, sync, find; the record ways: + assemble, contigs_text),
# in the order of WAYS below. Recorded once from the build of the commit before the entry points
# were folded into one pipeline (kh_capi.cpp in one file); the same at k = 19 and 51, cas and part.
HOST_SYNCS = {"host": 9, "dev": 12, "words": 4, "staged": 4, "dev_again": 6, "staged_again": 2}


@functools.lru_cache(maxsize=None)
def dataset(k):
    """(records, queries, oracle text): shared by the cases, never written to."""
    recs = kh.SyntheticKmers(k, N, 20, 400, 10, seed=9).records()
    rc, text, _, _, _, _ = ob.assemble(k, recs)
    assert rc == 0
    keys = recs[:, :kh.packed_size(k)]
    changed = keys[:64].copy()  # base i of key i changed: absent (or not: every way must agree)
    i = np.arange(64) % k
    changed[np.arange(64), i // 4] ^= (1 << (6 - 2 * (i % 4))).astype(np.uint8)
    q = np.ascontiguousarray(np.concatenate([keys, changed]))
    for a in (recs, q):
        a.setflags(write=False)
    return recs, q, text


def to_dev(sh, a):
    import torch
    return torch.from_numpy(np.array(a)).to(sh.dev)  # its own allocation: 16-byte aligned


def way_host(sh, recs):
    sh.table.insert_all(recs)


def way_dev(sh, recs):
    for a, b in zip(CUTS, CUTS[1:]):
        sh.insert_records(to_dev(sh, recs[a:b]))


def way_words(sh, recs):
    words, _ = sh.route(to_dev(sh, recs), 1, starts=True)
    sh.insert_words(words, N)


def way_staged(sh, recs):
    words, _ = sh.route(to_dev(sh, recs), 1, starts=True)
    a, W = CUTS[1], sh.W
    sh.stage_words(words, a, N)
    sh.stage_words(words[a * W:], 0, N)
    sh.stage_words(words[a * W:], N - a, N)
    sh.finish_words()


# name, insert, the table of an earlier way to clear and reuse, assemble too
WAYS = (("host", way_host, None, True), ("dev", way_dev, None, True), ("words", way_words, None, False),
        ("staged", way_staged, None, False), ("dev_again", way_dev, "dev", True),
        ("staged_again", way_staged, "staged", False))


@pytest.mark.parametrize("mode", ["cas", "part"])
@pytest.mark.parametrize("k", [19, 51])
def test_insert_ways_agree(monkeypatch, k, mode):
    import torch
    from cs267_hw3_amd.dist import GpuShard
    monkeypatch.setenv("KH_INSERT", mode)
    recs, q, text = dataset(k)
    shards, syncs, first = {}, {}, None
    for name, insert, reuse, walk in WAYS:
        sh = shards[name] = shards[reuse] if reuse else GpuShard(k, N)
        with torch.cuda.stream(sh.stream):
            if reuse:
                sh.clear()
            before = sh.host_syncs()
            insert(sh, recs)
            sh.sync()
            got = sh.table.find(q)
            if first is None:
                first = got
                assert got[1][:N].all() and np.array_equal(got[0][:N], recs), "the host insert lost k-mers"
            assert np.array_equal(got[1], first[1]), f"{name}: found flags differ from the host insert"
            assert np.array_equal(got[0], first[0]), f"{name}: extensions differ from the host insert"
            if walk:
                sh.table.assemble()
                assert sh.table.contigs_text() == text, f"{name}: text differs from the oracle"
            syncs[name] = sh.host_syncs() - before
            assert sh.stats()["n_inserted"] == N
    print(f"host_syncs k={k} {mode}: {syncs}")
    assert syncs == HOST_SYNCS
