#!/usr/bin/env python3
"""Find-over-text measurement on one GPU (a tool; bench.py is the project's benchmark).

The C3 set (k = 51, --n k-mers, default 200M, contigs of 8..200 k-mers, seed 51) is generated in
device memory, inserted and assembled; the query is the walk's own contig text (kh_contigs_text_dev,
about 296 MB at 200M). Prints ONE JSON line:
  find_text_ms / _kmers_per_s   kh_find_text_dev over the contig text (answers + counts)
  find_dev_ms / _kmers_per_s    kh_find_dev over the same k-mers, pre-packed (PACKED bytes each) in
                                contig order: the yardstick, the API a caller had before
  text_keys_count_ms            kh_text_keys_dev's counting pass + scan over the text (no keys written)
  bytes_per_window              bytes each path reads and writes per k-mer, table probes aside
Times are HIP-event times on the table's stream: after --warmup calls, the median of --reps single
calls (one call is tens of milliseconds at the default size; the two paths alternate).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000_000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import cs267_hw3_amd as kh
    from cs267_hw3_amd._lib import check
    from cs267_hw3_amd.dist import GpuShard

    k, n = 51, args.n
    KP, R = 13, 15
    g = kh.SyntheticKmers(k, n, 8, 200, 0, seed=51)
    shard = GpuShard(k, n)
    L, h, p, t = shard.L, shard.h, shard._p, shard.table
    with torch.cuda.stream(shard.stream):
        recs = g.records_dev(0, n, stream=shard.stream)
        t.insert_dev(recs.data_ptr(), n)
        t.sync()
        del recs
        t.assemble()
        d, b = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(L.kh_contigs_text_dev(h, ctypes.byref(d), ctypes.byref(b)))
        nbytes = b.value
        text = ctypes.c_void_p(d.value)  # the walk's text, read where the library keeps it
        keys = torch.empty((n, KP), dtype=torch.uint8, device=shard.dev)
        pos = torch.empty(n, dtype=torch.int32, device=shard.dev)
        count = torch.zeros(1, dtype=torch.int64, device=shard.dev)
        assert nbytes - k + 1 >= n
        check(L.kh_text_keys_dev(h, text, nbytes, None, None, p(count)))  # the count first: it sizes the keys
        shard.sync()
        m = int(count.cpu()[0])
        assert m == n, (m, n)
        check(L.kh_text_keys_dev(h, text, nbytes, p(keys), p(pos), p(count)))
        shard.sync()
        del pos
        ext = torch.empty((nbytes, 2), dtype=torch.uint8, device=shard.dev)
        counts = torch.zeros(2, dtype=torch.int64, device=shard.dev)
        out = torch.empty((n, R), dtype=torch.uint8, device=shard.dev)
        found = torch.empty(n, dtype=torch.uint8, device=shard.dev)
        cnt1 = torch.zeros(1, dtype=torch.int64, device=shard.dev)

        calls = {
            "find_text": lambda: check(L.kh_find_text_dev(h, text, nbytes, p(ext), p(counts))),
            "find_dev": lambda: check(L.kh_find_dev(h, p(keys), n, p(out), p(found))),
            "text_keys": lambda: check(L.kh_text_keys_dev(h, text, nbytes, None, None, p(cnt1))),
        }
        ms = {name: [] for name in calls}
        for it in range(args.warmup + args.reps):
            for name, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        med = {name: statistics.median(v) for name, v in ms.items()}
        c = counts.cpu().tolist()
        ok = c == [n, n] and bool(found.all()) and bool((ext[:k] != 0xFF).any())
    rate = lambda x: round(n / (x / 1e3))  # noqa: E731
    print(json.dumps({
        "tool": "find_text_bench", "k": k, "n_kmers": n, "text_bytes": nbytes, "reps": args.reps,
        "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "find_text_ms": round(med["find_text"], 3), "find_text_kmers_per_s": rate(med["find_text"]),
        "find_text_ms_min_max": [round(min(ms["find_text"]), 3), round(max(ms["find_text"]), 3)],
        "find_dev_ms": round(med["find_dev"], 3), "find_dev_kmers_per_s": rate(med["find_dev"]),
        "find_dev_ms_min_max": [round(min(ms["find_dev"]), 3), round(max(ms["find_dev"]), 3)],
        "text_keys_count_ms": round(med["text_keys"], 3),
        "bytes_per_window": {"find_text": round(3 * nbytes / n, 2), "find_dev": KP + R + 1},
        "windows_found": c, "all_found": ok,
    }), flush=True)
    t.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
