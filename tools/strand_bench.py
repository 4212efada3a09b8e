#!/usr/bin/env python3
"""Both-strand seed measurement on one GPU (a tool; bench.py is the project's benchmark).

The C3 set (k = 51, --n k-mers, default 200M, contigs of 8..200 k-mers, seed 51) is generated in
device memory, inserted, assembled and indexed. The reads are seed_bench.py's: the lines of the walk's
own contig text cut into --read 150-byte pieces with a '\\n' after each, made on the device with torch;
every second read is then reverse-complemented in place, on the device. Prints ONE JSON line:
  strand_text_ms     kh_seed_strand_text_dev: both locate passes into the scratch + k_seed_runs_strand
  locate_text_ms     kh_locate_text_dev over the read text;  locate_text_rc_ms  kh_locate_text_rc_dev
  strand_runs_ms     kh_seed_strand_runs_dev alone over the two position arrays
  yardstick_ms       what a caller of the forward calls must do for the same answer: kh_seed_text_dev
                     over the text, a torch reverse complement of the text (lookup table, flip) and of
                     the offsets, kh_seed_text_dev over that, and the mirror and merge of the two seed
                     arrays with torch, all on the device
Times are HIP-event times on the table's stream: after --warmup rounds, the median, minimum and
maximum of --reps single calls (the calls alternate within a round). Every read must answer one run
over all its windows, at its place in the contig text, with its strand, from both routes.
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
    dev = shard.dev
    with torch.cuda.stream(shard.stream):
        recs = g.records_dev(0, n, stream=shard.stream)
        t.insert_dev(recs.data_ptr(), n)
        t.sync()
        del recs
        torch.cuda.empty_cache()
        nc, _ = t.assemble()
        t.locate_build()
        own = torch.from_numpy(np.frombuffer(t.contigs_text(), np.uint8).copy()).to(dev)  # a copy to cut up
        nbytes = own.numel()
        nl = torch.nonzero(own == 10).view(-1)                      # the line ends
        start = torch.cat([nl.new_zeros(1), nl[:-1] + 1])           # line starts
        length = nl - start                                         # bases per line
        pieces = (length + RL - 1) // RL                            # reads per line
        first = torch.cumsum(pieces, 0) - pieces                    # a line's first read
        n_reads = int(pieces.sum())
        line = torch.repeat_interleave(torch.arange(nc, device=dev), pieces)
        j = torch.arange(n_reads, device=dev) - first[line]         # the read's number in its line
        src = start[line] + j * RL                                  # where it starts in the contig text
        rlen = torch.minimum(length[line] - j * RL, torch.full_like(j, RL))
        off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(rlen + 1, 0)                         # each read and its '\n'
        rbytes = int(off[-1])
        comp = torch.arange(256, dtype=torch.uint8, device=dev)     # the complement of A C G T, else the byte
        comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
        text = torch.full((rbytes,), 10, dtype=torch.uint8, device=dev)
        r = torch.repeat_interleave(torch.arange(n_reads, device=dev), rlen)
        at = torch.arange(r.numel(), device=dev) - (off[:-1] - torch.arange(n_reads, device=dev))[r]
        odd = (r & 1) == 1                                          # every second read: the other strand
        back = torch.where(odd, rlen[r] - 1 - at, at)
        b = own[src[r] + back]
        text[off[:-1][r] + at] = torch.where(odd, comp[b.long()], b)
        del own, nl, line, j, r, at, odd, back, b
        torch.cuda.empty_cache()
        pos = torch.empty(2 * rbytes, dtype=torch.int64, device=dev)
        seeds = torch.empty((n_reads, 6), dtype=torch.int64, device=dev)
        seeds_runs = torch.empty((n_reads, 6), dtype=torch.int64, device=dev)
        ypos = torch.empty(rbytes, dtype=torch.int64, device=dev)
        ys = [torch.empty((n_reads, 4), dtype=torch.int64, device=dev) for _ in range(2)]
        merged = {}

        def yardstick():
            check(L.kh_seed_text_dev(h, p(text), rbytes, p(off), n_reads, p(ypos), p(ys[0])))
            rtext = comp[text.long()].flip(0)
            roff = (rbytes - off).flip(0).contiguous()              # read r is read n_reads - 1 - r there
            check(L.kh_seed_text_dev(h, p(rtext), rbytes, p(roff), n_reads, p(ypos), p(ys[1])))
            f, m = ys[0], ys[1].flip(0)                             # m: back in read order
            rev = m[:, 2] > f[:, 2]                                 # equal runs: the forward one
            full = off[1:] - off[:-1]                               # the read's bytes, its '\n' included
            mstart = full - k - m[:, 0] - (m[:, 2] - 1)             # the run's first window, seen from this strand
            out = torch.empty((n_reads, 6), dtype=torch.int64, device=dev)
            out[:, 0] = torch.where(rev, mstart, f[:, 0])
            out[:, 1] = torch.where(rev, m[:, 1], f[:, 1])          # the flipped run's first value is its smallest
            out[:, 2] = torch.where(rev, m[:, 2], f[:, 2])
            out[:, 3] = rev.long()
            out[:, 4] = f[:, 3]
            out[:, 5] = m[:, 3]
            merged["seeds"] = out

        calls = {
            "strand_text": lambda: check(L.kh_seed_strand_text_dev(h, p(text), rbytes, p(off), n_reads, p(pos),
                                                                   p(seeds))),
            "yardstick": yardstick,
            "locate_text": lambda: check(L.kh_locate_text_dev(h, p(text), rbytes, p(pos), None)),
            "locate_text_rc": lambda: check(L.kh_locate_text_rc_dev(h, p(text), rbytes, p(pos[rbytes:]), None)),
            "strand_runs": lambda: check(L.kh_seed_strand_runs_dev(h, p(pos), p(pos[rbytes:]), rbytes, p(off), n_reads,
                                                                   p(seeds_runs))),
        }
        order = ("strand_text", "yardstick", "locate_text", "locate_text_rc", "strand_runs")
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
        # every read is a piece of a contig line or its reverse complement: one run over all its windows,
        # at its place in the contig text, on its strand
        want_run = torch.clamp(rlen - (k - 1), min=0)
        has = want_run > 0
        strand = (torch.arange(n_reads, device=dev) & 1)
        ok = {}
        for name, s in (("strand_text", seeds), ("strand_runs", seeds_runs), ("yardstick", merged["seeds"])):
            good = bool((s[:, 2] == want_run).all())
            good = good and bool((s[:, 3][has] == strand[has]).all()) and bool((s[:, 1][has] == src[has]).all())
            good = good and bool((s[:, 0][has] == 0).all()) and bool((s[:, 0][~has] == -1).all())
            good = good and bool((torch.where(strand == 1, s[:, 5], s[:, 4]) == want_run).all())
            ok[name] = good
        same = bool((seeds == merged["seeds"]).all()) and bool((seeds == seeds_runs).all())
        windows = int(torch.clamp(off[1:] - off[:-1] - k, min=0).sum())  # counted windows (the '\n' ends none)
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}  # noqa: E731
    out = {"tool": "strand_bench", "k": k, "n_kmers": n, "contigs": nc, "contig_text_bytes": nbytes,
           "read_bytes": RL, "n_reads": n_reads, "text_bytes": rbytes, "windows": windows, "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name in order:
        out[name + "_ms"] = stat(ms[name])
    out["strand_over_yardstick"] = round(out["strand_text_ms"]["median"] / out["yardstick_ms"]["median"], 3)
    out["rc_over_forward_locate"] = round(out["locate_text_rc_ms"]["median"] / out["locate_text_ms"]["median"], 3)
    out["locate_share_of_strand_text"] = round(
        (out["locate_text_ms"]["median"] + out["locate_text_rc_ms"]["median"]) / out["strand_text_ms"]["median"], 3)
    out["reads_with_a_seed"] = int(has.sum())
    out["answers_ok"] = ok
    out["routes_agree"] = same
    print(json.dumps(out), flush=True)
    t.close()
    return 0 if all(ok.values()) and same else 1


if __name__ == "__main__":
    sys.exit(main())
