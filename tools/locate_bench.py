#!/usr/bin/env python3
"""Position-index measurement on one GPU (a tool; bench.py is the project's benchmark).

The C3 set (k = 51, --n k-mers, default 200M, contigs of 8..200 k-mers, seed 51) is generated in
device memory, inserted and assembled; the text is the walk's own contig text (kh_contigs_text_dev,
about 296 MB at 200M). Prints ONE JSON line:
  locate_build_ms   kh_locate_build: the index's fill (capacity * 8 bytes) + one probe and one 8-byte
                    atomicMin per window of the text
  locate_text_ms    kh_locate_text_dev over the same text (positions + counts): one probe and one
                    dependent 8-byte load per window
  find_text_ms      kh_find_text_dev over the same text from the same process: the yardstick
  reset_ms          kh_locate_reset alone (the fill that is part of every build)
Times are HIP-event times on the table's stream: after --warmup rounds, the median, minimum and
maximum of --reps single calls (the three alternate within a round).
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
    g = kh.SyntheticKmers(k, n, 8, 200, 0, seed=51)
    shard = GpuShard(k, n)
    L, h, p, t = shard.L, shard.h, shard._p, shard.table
    with torch.cuda.stream(shard.stream):
        recs = g.records_dev(0, n, stream=shard.stream)
        t.insert_dev(recs.data_ptr(), n)
        t.sync()
        del recs
        torch.cuda.empty_cache()
        t.assemble()
        d, b = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(L.kh_contigs_text_dev(h, ctypes.byref(d), ctypes.byref(b)))
        nbytes = b.value
        text = ctypes.c_void_p(d.value)  # the walk's text, read where the library keeps it
        pos = torch.empty(nbytes, dtype=torch.int64, device=shard.dev)
        ext = torch.empty((nbytes, 2), dtype=torch.uint8, device=shard.dev)
        lcounts = torch.zeros(2, dtype=torch.int64, device=shard.dev)
        fcounts = torch.zeros(2, dtype=torch.int64, device=shard.dev)

        calls = {
            "locate_build": lambda: check(L.kh_locate_build(h)),
            "locate_text": lambda: check(L.kh_locate_text_dev(h, text, nbytes, p(pos), p(lcounts))),
            "find_text": lambda: check(L.kh_find_text_dev(h, text, nbytes, p(ext), p(fcounts))),
            "reset": lambda: check(L.kh_locate_reset(h)),
        }
        order = ("reset", "locate_build", "locate_text", "find_text")  # the reset first: the build refills it
        ms = {name: [] for name in calls}
        for it in range(args.warmup + args.reps):
            for name in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[name]()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        lc, fc = lcounts.cpu().tolist(), fcounts.cpu().tolist()
        # every k-mer of the set is unique: each window answers its own position
        at = torch.nonzero(pos[:1 << 20] != -1).view(-1)
        ok = lc == [n, n] and fc == [n, n] and bool((pos[:1 << 20][at] == at).all()) and at.numel() > 0
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}  # noqa: E731
    out = {"tool": "locate_bench", "k": k, "n_kmers": n, "text_bytes": nbytes, "capacity": t.capacity,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name in order:
        out[name + "_ms"] = stat(ms[name])
    fm = out["find_text_ms"]["median"]
    out["build_over_find_text"] = round(out["locate_build_ms"]["median"] / fm, 3)
    out["locate_text_over_find_text"] = round(out["locate_text_ms"]["median"] / fm, 3)
    out["windows_located"], out["windows_found"], out["all_located"] = lc, fc, ok
    print(json.dumps(out), flush=True)
    t.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
