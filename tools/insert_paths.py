#!/usr/bin/env python3
"""Every insert entry point of the C ABI once, for a kernel trace (profiles/r09): at k = 51 under
KH_INSERT=part the same 3 * 8192 + 77 records go in by kh_insert, by kh_insert_dev in three batches,
as routed words by kh_insert_words_dev and by kh_insert_words_stage_dev .. finish, the last two again
after kh_clear; then one kh_insert of 2^24 records (the chunked upload) and one assemble.

  rocprofv3 --kernel-trace -d OUT -o NAME --output-format csv -- python tools/insert_paths.py
  python tools/insert_paths.py --list OUT/.../NAME_kernel_trace.csv > launches.txt

--list prints (kernel, grid, workgroup, queue) per dispatch in dispatch order; queues are numbered
by first use, so the lists of two builds (KH_LIB) compare with diff."""
import csv
import os
import sys

os.environ["KH_INSERT"] = "part"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K, N = 51, 3 * 8192 + 77
CUTS = (0, 8192 + 1, 8192 + 2, N)


def launches(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    queues = {}
    for r in rows:
        q = queues.setdefault(r["Queue_Id"], len(queues))
        grid = "x".join(r[f"Grid_Size_{d}"] for d in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{d}"] for d in "XYZ")
        print(r["Kernel_Name"], grid, wg, f"q{q}")


def main():
    import numpy as np
    import torch
    import cs267_hw3_amd as kh
    from cs267_hw3_amd.dist import GpuShard

    recs = kh.SyntheticKmers(K, N, 20, 400, 10, seed=9).records()

    def dev(sh, a):
        return torch.from_numpy(np.array(a)).to(sh.dev)

    def by_dev(sh):
        for a, b in zip(CUTS, CUTS[1:]):
            sh.insert_records(dev(sh, recs[a:b]))

    def by_words(sh):
        words, _ = sh.route(dev(sh, recs), 1, starts=True)
        sh.insert_words(words, N)

    def by_stage(sh):
        words, _ = sh.route(dev(sh, recs), 1, starts=True)
        a, W = CUTS[1], sh.W
        sh.stage_words(words, a, N)
        sh.stage_words(words[a * W:], 0, N)
        sh.stage_words(words[a * W:], N - a, N)
        sh.finish_words()

    for way in (lambda sh: sh.table.insert_all(recs), by_dev, by_words, by_stage):
        sh = GpuShard(K, N)
        with torch.cuda.stream(sh.stream):
            way(sh)
            sh.sync()
            if way in (by_dev, by_stage):
                sh.clear()
                way(sh)
                sh.sync()
    big = kh.SyntheticKmers(K, 1 << 24, 8, 200, 0, seed=5).records()
    with kh.KmerHashTable(K, len(big)) as t:
        t.insert_all(big)
        print("contigs, bytes:", t.assemble())


if __name__ == "__main__":
    launches(sys.argv[2]) if sys.argv[1:2] == ["--list"] else main()
