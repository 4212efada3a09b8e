#!/usr/bin/env python3
"""Seed measurement on one GPU (a tool; bench.py is the project's benchmark).

The C3 set (k = 51, --n k-mers, default 200M, contigs of 8..200 k-mers, seed 51) is generated in
device memory, inserted, assembled and indexed; the text is the walk's own contig text
(kh_contigs_text_dev). The reads are its lines cut into --read 150-byte pieces with a '\\n' after each:
the read text and its offsets are made on the device with torch. Prints ONE JSON line:
  seed_text_ms    kh_seed_text_dev over the read text: kh_locate_text_dev into the scratch + k_seed_runs
  locate_text_ms  kh_locate_text_dev over the same text (positions only): code the parent has
  copy_ms         a device-to-device hipMemcpyAsync of the 8 * len byte position array
  yardstick_ms    locate_text + copy: the run kernel reads the array once and writes 32 B per read, a
                  copy reads it and writes it
  seed_runs_ms    kh_seed_runs_dev alone over the positions;  seed_cov_ms  kh_seed_coverage_dev
Times are HIP-event times on the table's stream: after --warmup rounds, the median, minimum and
maximum of --reps single calls (the calls alternate within a round).
"""
import argparse
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
    ap.add_argument("--read", type=int, default=150)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    import cs267_hw3_amd as kh
    from cs267_hw3_amd._lib import check
    from cs267_hw3_amd.dist import GpuShard

    k, n, RL = 51, args.n, args.read
    g = kh.SyntheticKmers(k, n, 8, 200, 0, seed=51)
    shard = GpuShard(k, n)
    L, h, p, t = shard.L, shard.h, shard._p, shard.table
    with torch.cuda.stream(shard.stream):
        recs = g.records_dev(0, n, stream=shard.stream)
        t.insert_dev(recs.data_ptr(), n)
        t.sync()
        del recs
        torch.cuda.empty_cache()
        nc, _ = t.assemble()
        t.locate_build()
        own = torch.from_numpy(np.frombuffer(t.contigs_text(), np.uint8).copy()).to(shard.dev)  # a copy to cut up
        nbytes = own.numel()
        nl = torch.nonzero(own == 10).view(-1)                      # the line ends
        start = torch.cat([nl.new_zeros(1), nl[:-1] + 1])           # line starts
        length = nl - start                                         # bases per line
        pieces = (length + RL - 1) // RL                            # reads per line
        first = torch.cumsum(pieces, 0) - pieces                    # a line's first read
        n_reads = int(pieces.sum())
        line = torch.repeat_interleave(torch.arange(nc, device=shard.dev), pieces)
        j = torch.arange(n_reads, device=shard.dev) - first[line]   # the read's number in its line
        src = start[line] + j * RL                                  # where it starts in the contig text
        rlen = torch.minimum(length[line] - j * RL, torch.full_like(j, RL))
        off = torch.zeros(n_reads + 1, dtype=torch.int64, device=shard.dev)
        off[1:] = torch.cumsum(rlen + 1, 0)                         # each read and its '\n'
        rbytes = int(off[-1])
        text = torch.full((rbytes,), 10, dtype=torch.uint8, device=shard.dev)
        r = torch.repeat_interleave(torch.arange(n_reads, device=shard.dev), rlen)
        at = torch.arange(r.numel(), device=shard.dev) - (off[:-1] - torch.arange(n_reads, device=shard.dev))[r]
        text[off[:-1][r] + at] = own[src[r] + at]
        del own, nl, line, j, r, at
        torch.cuda.empty_cache()
        pos = torch.empty(rbytes, dtype=torch.int64, device=shard.dev)
        pos2 = torch.empty(rbytes, dtype=torch.int64, device=shard.dev)
        seeds = torch.empty((n_reads, 4), dtype=torch.int64, device=shard.dev)
        cov = torch.zeros((2, nc), dtype=torch.int64, device=shard.dev)

        def copy():
            pos2.copy_(pos, non_blocking=True)  # hipMemcpyAsync device-to-device on the current stream

        calls = {
            "seed_text": lambda: check(L.kh_seed_text_dev(h, p(text), rbytes, p(off), n_reads, p(pos), p(seeds))),
            "locate_text": lambda: check(L.kh_locate_text_dev(h, p(text), rbytes, p(pos), None)),
            "copy": copy,
            "seed_runs": lambda: check(L.kh_seed_runs_dev(h, p(pos), rbytes, p(off), n_reads, p(seeds))),
            "seed_cov": lambda: check(L.kh_seed_coverage_dev(h, p(seeds), n_reads, p(cov[0]), p(cov[1]))),
        }
        order = ("seed_text", "locate_text", "copy", "seed_runs", "seed_cov")
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
        # every read is a piece of a contig line: one run over all its windows, at its place in the text
        want_run = torch.clamp(rlen - (k - 1), min=0)
        ok = bool((seeds[:, 2] == want_run).all()) and bool((seeds[:, 3] == want_run).all())
        has = want_run > 0
        ok = ok and bool((seeds[:, 1][has] == src[has]).all()) and bool((seeds[:, 0][has] == 0).all())
        ok = ok and bool((seeds[:, 0][~has] == -1).all())
        rounds = args.warmup + args.reps
        ok = ok and int(cov[0].sum()) == rounds * int(has.sum())
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}  # noqa: E731
    out = {"tool": "seed_bench", "k": k, "n_kmers": n, "contigs": nc, "contig_text_bytes": nbytes,
           "read_bytes": RL, "n_reads": n_reads, "text_bytes": rbytes, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    for name in order:
        out[name + "_ms"] = stat(ms[name])
    y = out["locate_text_ms"]["median"] + out["copy_ms"]["median"]
    out["yardstick_ms"] = round(y, 3)
    out["seed_over_yardstick"] = round(out["seed_text_ms"]["median"] / y, 3)
    out["reads_with_a_seed"] = int(has.sum())
    out["answers_ok"] = ok
    print(json.dumps(out), flush=True)
    t.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
