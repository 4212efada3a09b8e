#!/usr/bin/env python3
"""Batched-find measurement on one GPU (a tool; bench.py is the project's benchmark).

k = 51, a table of --n k-mers (default 20M) and --queries keys (default 20M, 90 % present, the
rest a present key with one base changed), all in device memory. Prints ONE JSON line:
  kh_find_dev_keys_per_s      the single-table batched find (k_find), the baseline
  find_route_keys_per_s       kh_find_route_dev at 1 rank and at 8 ranks (owner grouping)
  find_answer_keys_per_s      kh_find_answer_dev (the owner's probe, 2 bytes per key out)
  find_gather_keys_per_s      kh_find_gather_dev (answers -> records in key order)
  dist_find_keys_per_s        DistributedKmerHashMap.find at one rank with the exchanges run
                              (KH_DIST_SELF_EXCHANGE=1 semantics), wall clock incl. its host read
  return_bytes_per_key        bytes the return exchange carried per key
Kernel times are HIP-event times on the table's stream: the median over --reps windows of --iters
back-to-back calls each, after a warm-up call (the table, 640 MB at the default size, does not fit
the cache, so repeating the same keys does not turn the probes into cache hits).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--queries", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per figure (the median is reported)")
    ap.add_argument("--iters", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--commit", default=None, help="commit the numbers are taken on (default: git rev-parse)")
    args = ap.parse_args()

    import torch
    import cs267_hw3_amd as kh
    from cs267_hw3_amd.dist import DistributedKmerHashMap, GpuShard, ThreadComm

    k, n, nq = 51, args.n, args.queries
    KP, R = 13, 15
    g = kh.SyntheticKmers(k, n, 8, 200, 10, seed=1)
    shard = GpuShard(k, n)
    L, h, p = shard.L, shard.h, shard._p
    with torch.cuda.stream(shard.stream):
        recs = g.records_dev(0, n, stream=shard.stream)
        dm = DistributedKmerHashMap(ThreadComm.group(1)[0], shard)
        dm.insert_all(recs)
        gen = torch.Generator(device="cuda").manual_seed(1)
        pick = torch.randint(0, n, (nq,), device="cuda", generator=gen)
        keys = recs[pick][:, :KP].contiguous()
        absent = torch.rand(nq, device="cuda", generator=gen) < 0.1
        keys[:, 0] ^= (absent.to(torch.uint8) << 6)  # base 1 of the k-mer changed
        del pick, recs
        shard.sync()

        def timed(f):
            f()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    f()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / args.iters)
            return statistics.median(ms)

        out = torch.empty((nq, R), dtype=torch.uint8, device="cuda")
        found = torch.empty(nq, dtype=torch.uint8, device="cuda")
        ms_base = timed(lambda: kh._lib.check(L.kh_find_dev(h, p(keys), nq, p(out), p(found))))
        res = {}
        for P in (1, 8):
            res[P] = [None]

            def route(P=P):
                res[P][0] = shard.find_route(keys, P)
            ms = timed(route)
            res[P].append(ms)
        gkeys, index, _ = res[1][0]
        ext = [None]

        def answer():
            ext[0] = shard.find_answer(gkeys, nq)
        ms_answer = timed(answer)
        got = [None]

        def gather():
            got[0] = shard.find_gather(keys, index, ext[0])
        ms_gather = timed(gather)
        shard.sync()
        same = bool(torch.equal(got[0][0], out) and torch.equal(got[0][1], found))
        present = float(found.float().mean())

        dm.SELF_EXCHANGE = True
        dm.find(keys)
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(max(args.iters // 5, 1)):
                r2, f2 = dm.find(keys)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / max(args.iters // 5, 1))
        ms_dist = 1e3 * statistics.median(wall)
        same = same and bool(torch.equal(r2, out) and torch.equal(f2, found))
        ret_bytes = dm.find_answer_bytes / nq
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True, timeout=10).stdout.strip() or "unknown"
        except Exception:
            commit = "unknown"
    rate = lambda ms: round(nq / (ms / 1e3))  # noqa: E731
    print(json.dumps({
        "tool": "find_bench", "k": k, "n_table": n, "n_queries": nq, "present_fraction": round(present, 4),
        "reps": args.reps, "iters": args.iters, "commit": commit, "device": torch.cuda.get_device_name(0),
        "kh_find_dev_keys_per_s": rate(ms_base), "kh_find_dev_ms": round(ms_base, 3),
        "find_route_keys_per_s": {"ranks_1": rate(res[1][1]), "ranks_8": rate(res[8][1])},
        "find_route_ms": {"ranks_1": round(res[1][1], 3), "ranks_8": round(res[8][1], 3)},
        "find_answer_keys_per_s": rate(ms_answer), "find_answer_ms": round(ms_answer, 3),
        "find_gather_keys_per_s": rate(ms_gather), "find_gather_ms": round(ms_gather, 3),
        "dist_find_keys_per_s": rate(ms_dist), "dist_find_ms": round(ms_dist, 3),
        "return_bytes_per_key": ret_bytes, "matches_kh_find_dev": same,
    }), flush=True)
    shard.table.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
