"""DistributedKmerHashMap.find (cs267_hw3_amd.dist) over real torch.distributed gloo groups on CPU:
the driver logic -- route, count exchange, key exchange, answer, return exchange with the splits
swapped, gather -- with a numpy test double of the three shard calls. Expected answers come from
the input records (key bytes -> record)."""
import json
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
NAME = "tiny19"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _queries(k, recs, rank, world):
    """Rank `rank`'s seeded shuffle of every present key, absent keys (one base of a present key
    changed; the parent filters its expectation through the dictionary, so a changed key that
    happens to be in the set is simply expected present) and a few repeats; the last rank of a
    world >= 2 asks nothing."""
    KP = (k + 3) // 4
    if world >= 2 and rank == world - 1:
        return np.zeros((0, KP), np.uint8)
    present = recs[:, :KP]
    changed = np.array(present[::3], dtype=np.uint8, copy=True)
    i = np.arange(len(changed))
    base = i % k
    changed[i, base // 4] ^= (1 << (6 - 2 * (base % 4))).astype(np.uint8)
    q = np.concatenate([present, changed, present[:5]])
    q = q[np.random.default_rng(7 + rank).permutation(len(q))]
    return np.ascontiguousarray(q[:-1] if len(q) % 64 == 0 else q)


def _rank_main(rank, world, port, outdir, chunk_bytes):
    import sys
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    import torch.distributed as dist
    import cs267_hw3_amd as kh
    from cs267_hw3_amd.dist import DistributedKmerHashMap, TorchComm
    from dist_fake_shard import FakeShard

    class FindShard(FakeShard):
        """FakeShard + numpy versions of find_route / find_answer / find_gather (kh_find_*_dev)."""

        def find_route(self, keys, nranks):
            rows = [bytes(r) for r in keys.numpy()]
            payloads, order, counts = self._group([(self._owner(r, nranks), r) for r in rows], nranks)
            out = np.zeros((max(len(rows), 1), self.P), np.uint8)
            for j, r in enumerate(payloads):
                out[j] = np.frombuffer(r, np.uint8)
            index = np.zeros(max(len(rows), 1), np.int32)
            index[:len(rows)] = order
            return torch.from_numpy(out), torch.from_numpy(index), counts

        def find_answer(self, keys, m):
            a = keys.numpy().reshape(-1)[:m * self.P].reshape(m, self.P)
            ext = np.zeros((max(m, 1), 2), np.uint8)
            for i in range(m):
                rec = self.table.get(bytes(a[i]))
                if rec is not None:
                    ext[i] = [rec[self.P], rec[self.P + 1]]
            return torch.from_numpy(ext)

        def find_gather(self, keys, index, ext):
            n = keys.shape[0]
            k_, e, idx = keys.numpy(), ext.numpy().reshape(-1, 2), index.numpy()
            recs = np.zeros((n, self.R), np.uint8)
            found = np.zeros(n, np.uint8)
            for j in range(n):
                if e[j].any():
                    i = idx[j]
                    recs[i, :self.P] = k_[i]
                    recs[i, self.P:] = e[j]
                    found[i] = 1
            return torch.from_numpy(recs), torch.from_numpy(found)

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    k = MANIFEST[NAME]["k"]
    path = os.path.join(GOLDEN, f"{NAME}.txt")
    recs = kh.read_kmers(path, k, world, rank)
    every = kh.read_kmers(path, k)
    dm = DistributedKmerHashMap(TorchComm(), FindShard(k))
    if chunk_bytes:
        dm.A2A_CHUNK_BYTES = chunk_bytes
    dm.insert_all(torch.from_numpy(recs))
    q = _queries(k, every, rank, world)
    x0, s0, phase0 = dm.xbytes, dm.host_syncs(), dm.phase
    got_r, got_f = dm.find(torch.from_numpy(q))
    stats = [dm.xbytes - x0, dm.host_syncs() - s0, dm.find_key_bytes, dm.find_answer_bytes]
    host_r, host_f = dm.find(q)                      # a host array: numpy back, found as bool
    assert isinstance(host_r, np.ndarray) and host_f.dtype == bool
    assert np.array_equal(host_r, got_r.numpy()) and np.array_equal(host_f, got_f.numpy().astype(bool))
    assert dm.phase == phase0                        # the step's open phase is resumed
    rounds = dm.assemble(MANIFEST[NAME]["n"])        # the walk after the finds is the usual one
    np.save(os.path.join(outdir, f"recs_{rank}.npy"), got_r.numpy())
    np.save(os.path.join(outdir, f"found_{rank}.npy"), got_f.numpy())
    np.save(os.path.join(outdir, f"stats_{rank}.npy"), np.array(stats, np.int64))
    with open(os.path.join(outdir, f"test_{rank}.dat"), "wb") as f:
        f.write(dm.contigs_text())
    assert rounds > 0
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,chunk", [(2, None), (3, None), (3, 96), (1, None)])
def test_find_driver_gloo(tmp_path, world, chunk):
    mp.start_processes(_rank_main, args=(world, _free_port(), str(tmp_path), chunk),
                       nprocs=world, join=True, start_method="spawn")
    import cs267_hw3_amd as kh
    m = MANIFEST[NAME]
    k = m["k"]
    KP, R = (k + 3) // 4, (k + 3) // 4 + 2
    every = kh.read_kmers(os.path.join(GOLDEN, f"{NAME}.txt"), k)
    table = {bytes(r[:KP]): r for r in every}
    g = kh.SyntheticKmers(k, m["n"], m["len_min"], m["len_max"], m["single_permille"], seed=m["seed"])
    asked = answered = 0
    for r in range(world):
        q = _queries(k, every, r, world)
        want_r = np.zeros((len(q), R), np.uint8)
        want_f = np.zeros(len(q), np.uint8)
        for i, key in enumerate(q):
            rec = table.get(bytes(key))
            if rec is not None:
                want_r[i], want_f[i] = rec, 1
        assert np.array_equal(np.load(tmp_path / f"found_{r}.npy"), want_f), f"rank {r}"
        assert np.array_equal(np.load(tmp_path / f"recs_{r}.npy"), want_r), f"rank {r}"
        if len(q):
            assert 0 < want_f.sum() < len(q)            # present and absent keys were asked
        xbytes, syncs, key_bytes, answer_bytes = np.load(tmp_path / f"stats_{r}.npy")
        assert syncs == 1                               # one blocking read: the counts
        if world > 1:
            assert key_bytes == len(q) * KP
            assert xbytes <= 32 * (world - 1) + key_bytes + answer_bytes
        else:
            assert xbytes == key_bytes == answer_bytes == 0  # one rank: no exchange
        asked += len(q)
        answered += answer_bytes
        b, e = g.block(world, r)
        assert open(tmp_path / f"test_{r}.dat", "rb").read() == g.truth(b, e)
    if world > 1:
        assert answered == 2 * asked                    # the return exchange: 2 bytes per key
    assert world == 1 or len(_queries(k, every, world - 1, world)) == 0
